"""Map output: what `MapRender.render` and `MapRender.__call__` cost, beside the host work they replace.

    python tools/map_output_timing.py [--n 30] [--reps 3]         # -> stdout; profiles/map_output.txt keeps a run
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mo -- python tools/map_output_timing.py --trace
    python tools/map_output_timing.py --summarise DIR             # the kernels' own durations per case, from the trace

Cases: 1 and 4 maps of 200 x 200 at target_size 400, with 8 layers (static only, what collate_fn produces) and 18 layers
(8 static + 10 dynamic): the `full` input of tests/golden/mint_map_output.py, uint8 and resident on the device.  After a
warm-up, per case and repetition:
  * render: the whole `MapRender.render` call (three launches: dd_map_render_u8, dd_image_resample_u8, dd_map_compose_u8)
            between a pair of device events, median of N.  The bracket holds the host side of the three calls too —
            argument checks, ctypes marshalling, the allocations, the gaps between the launches — so for kernels this short
            it measures LAUNCH LATENCY, not device time;
  * call:   wall clock of `MapRender.__call__` with a warm legend cache (render, the 4-byte-per-sample readback, one compose
            per distinct legend), ending in a device synchronise.  The legend function returns a constant 76 x 400 array (the
            size matplotlib's legend of the 18 classes has): its pixels do not enter the time;
  * host:   wall clock of the numpy restatement (tests/map_output_reference.py: vectorised colouring, the restated PIL
            resize, turn, legend paste) plus the upload of the pictures, ending in a device synchronise, median of N runs.
            This is NOT the reference's `visualize_map`, whose Python loop over the pixels takes 0.36-0.53 s a map.
Each figure is printed per repetition, with the spread (max - min) / median over the repetitions.
--trace: per case WARM + N `render` calls and nothing else, for a kernel trace; --summarise splits the trace's rows of the
three kernels, in time order, into the cases and prints the median and minimum of each kernel's own duration.
Timing is reported, not gated.  Exits non-zero when there is no GPU."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIDE, TARGET = 200, 400
CASES = [(1, 8), (1, 18), (4, 8), (4, 18)]                       # (maps, layers)
KERNELS = ("dd_map_render_kernel", "dd_image_resample_kernel", "dd_map_compose_kernel")
WARM = 3


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
    print("# kernel durations from the trace, %d x %d maps at target_size %d; median / min of %d launches; us"
          % (SIDE, SIDE, TARGET, n))
    for k in KERNELS:
        rows[k].sort()
        if len(rows[k]) != len(CASES) * (WARM + n):
            raise SystemExit("expected %d launches of %s in the trace, found %d" % (len(CASES) * (WARM + n), k, len(rows[k])))
    for i, (maps, layers) in enumerate(CASES):
        total = 0.0
        for k in KERNELS:
            d = [(e - s) / 1e3 for s, e in rows[k][i * (WARM + n) + WARM:(i + 1) * (WARM + n)]]
            total += statistics.median(d)
            print("%d map%s, %2d layers  %-26s median %6.2f  min %6.2f" % (maps, " " if maps == 1 else "s", layers, k,
                                                                         statistics.median(d), min(d)))
        print("%d map%s, %2d layers  %-26s        %6.2f" % (maps, " " if maps == 1 else "s", layers, "sum of the medians", total))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30, help="calls / runs per measurement")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarise", metavar="DIR_OR_KERNEL_TRACE_CSV")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.n)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("map_output_timing: no GPU", file=sys.stderr)
        return 2
    from dualdiff_amd.pipeline.map_output import COLORS, STATIC_PRIORITY, MapRender
    from tests import map_output_reference as R
    from tests.golden import mint_map_output as M
    torch.set_num_threads(1)
    med = statistics.median
    constant = np.zeros((76, TARGET, 3), dtype=np.uint8)
    constant[::2] = 255

    def legend(names, long_edge_size):
        return constant

    render = MapRender(M.MAP_CLASSES, M.OBJECT_CLASSES, target_size=TARGET)
    full = M.inputs("full")
    if not args.trace:
        print("# MapRender, %d x %d maps at target_size %d; median of %d, %d repetitions; us" % (SIDE, SIDE, TARGET, args.n, args.reps))
    for maps, layers in CASES:
        one = full[:layers]
        dev = torch.from_numpy(np.ascontiguousarray(np.repeat(one[None], maps, axis=0))).cuda()

        def kernel():
            return render.render(dev)

        def call():
            out = render(dev, legend=legend)
            torch.cuda.synchronize()
            return out

        def host():
            pics = []
            for _ in range(maps):
                frame, used = R.render(one, M.MAP_CLASSES, M.OBJECT_CLASSES, COLORS, STATIC_PRIORITY, TARGET)
                pics.append(torch.from_numpy(R.compose(frame, legend(used, TARGET))).cuda())
            torch.cuda.synchronize()
            return pics

        if args.trace:
            for _ in range(WARM + args.n):
                kernel()
            torch.cuda.synchronize()
            continue
        want, got = host(), call()
        same = all(torch.equal(g, w) for g, w in zip(got, want))
        for _ in range(3):
            kernel(), call()
        host()
        torch.cuda.synchronize()
        rows = {"kernel": [], "call": [], "host": []}
        for _ in range(args.reps):
            ts = []
            for _ in range(args.n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                kernel()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            rows["kernel"].append(med(ts))
            for name, fn, n in (("call", call, args.n), ("host", host, max(3, args.n // 10))):
                ts = []
                for _ in range(n):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    ts.append((time.perf_counter() - t0) * 1e6)
                rows[name].append(med(ts))
        print("%d map%s, %2d layers, results equal: %s" % (maps, " " if maps == 1 else "s", layers, same))
        for name, what in (("kernel", "device events around MapRender.render, 3 launches (launch latency)"),
                           ("call", "MapRender.__call__, warm legend cache, wall"),
                           ("host", "numpy restatement + upload, wall (median of %d)" % max(3, args.n // 10))):
            v = rows[name]
            print("    %-68s %s   spread %4.1f %%" % (what, "  ".join("%10.1f" % x for x in v), 100 * (max(v) - min(v)) / med(v)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
