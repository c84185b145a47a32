"""Box output: what `BoxOverlay.__call__` costs, beside the host path it replaces.

    python tools/box_output_timing.py [--n 30] [--reps 3]         # -> stdout; profiles/box_output.txt keeps a run
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o bo -- python tools/box_output_timing.py --trace
    python tools/box_output_timing.py --summarise DIR             # the kernels' own durations per case, from the trace

Cases: one scene of six views, 224 x 400 with 40 and with 200 boxes and 900 x 1600 with 40 boxes (boxes all around the
cameras, tests/box_output_reference.py: make_case), the frames, corners, labels and matrices resident on the device.
After a warm-up, per case and repetition:
  * launches: `BoxOverlay.__call__(check=False)` — the upload of the offsets, dd_box_edges, dd_box_draw_u8 —
              between a pair of device events, median of N.  The bracket holds the host side of the call too (argument
              checks, ctypes marshalling, the allocations), so for the small frames it measures launch latency;
  * call:     wall clock of `BoxOverlay.__call__` with check=True (the 4-byte flags readback), ending in a synchronise;
  * host:     wall clock of the path the feature replaces, on the same machine: `frames.cpu()`, the oracle of
              tests/box_output_reference.py (numpy float64 geometry, PIL's ImageDraw.line per edge) and the upload of the
              pictures, ending in a synchronise, median of max(3, N / 10) runs.  This is NOT the reference's cv2 path, which
              cannot run here; it draws the same thin lines with PIL's C loop.
Each figure is printed per repetition, with the spread (max - min) / median over the repetitions.  Opaque overlays;
--transparent measures the RGBA form (no frame is read).
--trace: per case WARM + N calls and nothing else, for a kernel trace; --summarise splits the trace's rows of the two
kernels, in time order, into the cases and prints the median and minimum of each kernel's own duration.
DD_HIP_LIB selects another build of the library (the tile shapes of csrc/box_overlay.hip: -DDD_BO_TILE_W=64 / 32).
Timing is reported, not gated.  Exits non-zero when there is no GPU."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(224, 400, 40), (224, 400, 200), (900, 1600, 40)]       # (H, W, boxes), six views each
KERNELS = ("dd_box_edges_kernel", "dd_box_draw_kernel")
VIEWS, WARM = 6, 3


def summarise(path, n):
    import csv
    import glob
    if os.path.isdir(path):
        found = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
        if not found:
            raise SystemExit("no *kernel_trace.csv under %s" % path)
        path = found[0]
    csv.field_size_limit(1 << 30)
    rows = {k: [] for k in KERNELS}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            for k in KERNELS:
                if k in r["Kernel_Name"]:
                    rows[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    print("# kernel durations from the trace, six views; median / min of %d launches; us" % n)
    for k in KERNELS:
        rows[k].sort()
        if len(rows[k]) != len(CASES) * (WARM + n):
            raise SystemExit("expected %d launches of %s in the trace, found %d" % (len(CASES) * (WARM + n), k, len(rows[k])))
    for i, (h, w, boxes) in enumerate(CASES):
        total = 0.0
        for k in KERNELS:
            d = [(e - s) / 1e3 for s, e in rows[k][i * (WARM + n) + WARM:(i + 1) * (WARM + n)]]
            total += statistics.median(d)
            print("%4d x %4d, %3d boxes  %-22s median %8.2f  min %8.2f" % (h, w, boxes, k, statistics.median(d), min(d)))
        print("%4d x %4d, %3d boxes  %-22s        %8.2f" % (h, w, boxes, "sum of the medians", total))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30, help="calls / runs per measurement")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--transparent", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarise", metavar="DIR_OR_KERNEL_TRACE_CSV")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.n)
    import torch
    if not torch.cuda.is_available():
        print("box_output_timing: no GPU", file=sys.stderr)
        return 2
    from dualdiff_amd import _build
    from dualdiff_amd.pipeline.box_output import BoxOverlay
    from tests import box_output_reference as R
    torch.set_num_threads(1)
    med = statistics.median
    overlay = BoxOverlay(R.OBJECT_CLASSES, transparent_bg=args.transparent)
    if not args.trace:
        print("# BoxOverlay (%s), one scene of %d views; library %s; median of %d, %d repetitions; us"
              % ("RGBA" if args.transparent else "opaque", VIEWS, os.path.basename(_build.lib_path()), args.n, args.reps))
    for h, w, boxes in CASES:
        case = R.make_case("timing", 7, (boxes,), VIEWS, h, w)
        frames = torch.from_numpy(case.frames).cuda()
        corners = torch.from_numpy(case.corners[0]).cuda()
        labels = torch.from_numpy(case.labels[0]).cuda()
        trans = torch.from_numpy(case.transforms).cuda()
        offsets = [0, boxes]
        src = None if args.transparent else frames

        def launches():
            return overlay(src, corners, labels, trans, offsets=offsets, check=False, size=(h, w))

        def call():
            out = overlay(src, corners, labels, trans, offsets=offsets, size=(h, w))
            torch.cuda.synchronize()
            return out

        def host():
            host_case = case._replace(frames=frames.cpu().numpy())
            out = torch.from_numpy(R.overlay(host_case, args.transparent)).cuda()
            torch.cuda.synchronize()
            return out

        if args.trace:
            for _ in range(WARM + args.n):
                launches()
            torch.cuda.synchronize()
            continue
        want, got = host(), call()
        same = torch.equal(got, want)
        drawn = int(overlay.edges(corners, labels, trans, offsets=offsets)[2].sum())
        for _ in range(WARM):
            launches(), call()
        torch.cuda.synchronize()
        rows = {"launches": [], "call": [], "host": []}
        for _ in range(args.reps):
            ts = []
            for _ in range(args.n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launches()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            rows["launches"].append(med(ts))
            for name, fn, n in (("call", call, args.n), ("host", host, max(3, args.n // 10))):
                ts = []
                for _ in range(n):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    ts.append((time.perf_counter() - t0) * 1e6)
                rows[name].append(med(ts))
        print("%d x %d, %d boxes (%d drawn over the six views), results equal: %s" % (h, w, boxes, drawn, same))
        for name, what in (("launches", "device events around BoxOverlay.__call__(check=False), 2 launches"),
                           ("call", "BoxOverlay.__call__, check=True, wall"),
                           ("host", "frames.cpu() + oracle (numpy, PIL) + upload, wall (median of %d)" % max(3, args.n // 10))):
            v = rows[name]
            print("    %-68s %s   spread %4.1f %%" % (what, "  ".join("%10.1f" % x for x in v), 100 * (max(v) - min(v)) / med(v)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
