"""Box input: what a dd_box_views launch costs, beside the host work it replaces.

    python tools/box_input_timing.py [--n 50] [--reps 3]          # -> stdout; profiles/box_input.txt keeps a run
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o bi -- python tools/box_input_timing.py --trace
    python tools/box_input_timing.py --summarise DIR              # the kernel's own duration per case, from the trace

Cases: 1 and 4 scenes x 6 views x 200 boxes, `all-xyz`, both filters (positive z; canvas 224 x 400), seeded boxes and ring
cameras of tests/box_input_reference.py.  After a warm-up, per case and repetition:
  * launch: the whole `ops.box_views` call on resident inputs between a pair of device events, median of N.  The bracket
            holds the host side of the call too — argument checks, ctypes marshalling, the gap between the 4-byte clear of
            max_len and the kernel launch — so for a kernel this short it measures LAUNCH LATENCY, not device time;
  * host:   wall clock of the numpy float64 restatement (transform, filter, selection, padding to the batch maximum) plus
            the three host-to-device copies (bboxes, classes, masks) that the launch replaces, ending in a device
            synchronise, median of N runs, one CPU thread for torch (numpy's BLAS keeps its own setting);
  * call:   wall clock of the whole `BoxPreProcess.__call__` with sync=True (pack, one upload, launch, 4-byte readback).
Each figure is printed per repetition, with the spread (max - min) / median over the repetitions.
--trace: per case WARM + N launches and nothing else, for a kernel trace; --summarise splits the trace's
dd_box_views_kernel rows, in time order, into the cases and prints the median and minimum of the kernel's own duration.
Timing is reported, not gated.  Exits non-zero when there is no GPU."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VIEWS, BOXES = 6, 200
CASES = [(1, True), (1, False), (4, True), (4, False)]           # (scenes, use_3d_filter)
KERNEL = "dd_box_views_kernel"
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
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            if KERNEL in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort()
    if len(rows) != len(CASES) * (WARM + n):
        raise SystemExit("expected %d launches of %s in the trace, found %d" % (len(CASES) * (WARM + n), KERNEL, len(rows)))
    print("# %s, kernel duration from the trace, %d views x %d boxes a scene, all-xyz; median / min of %d launches; us"
          % (KERNEL, VIEWS, BOXES, n))
    for i, (scenes, f3d) in enumerate(CASES):
        d = [(e - s) / 1e3 for s, e in rows[i * (WARM + n) + WARM:(i + 1) * (WARM + n)]]
        print("%d scene%s, filter %-10s  median %6.2f  min %6.2f" % (scenes, " " if scenes == 1 else "s",
                                                                   "positive_z" if f3d else "canvas", statistics.median(d), min(d)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50, help="launches / runs per measurement")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarise", metavar="DIR_OR_KERNEL_TRACE_CSV")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.n)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("box_input_timing: no GPU", file=sys.stderr)
        return 2
    from dualdiff_amd import ops
    from dualdiff_amd.networks.layers import box_capacity
    from dualdiff_amd.pipeline.box_input import BoxPreProcess
    from tests import box_input_reference as RB
    torch.set_num_threads(1)
    med = statistics.median
    if not args.trace:
        print("# dd_box_views, %d views x %d boxes a scene, all-xyz; median of %d, %d repetitions; us" % (VIEWS, BOXES, args.n, args.reps))
    for scenes, f3d in CASES:
        data = RB.batch(50 + scenes, (BOXES,) * scenes, VIEWS)
        trans = RB.transforms_of(data, f3d)
        filt = "positive_z" if f3d else "canvas"
        pre = BoxPreProcess("all-xyz", use_3d_filter=f3d, canvas_size=RB.CANVAS)
        cap = box_capacity(BOXES)
        dev = lambda parts: torch.from_numpy(np.concatenate(parts)).cuda()   # noqa: E731
        corners, fcorners, labels = dev(data["corners"]), dev(data["filter_corners"]), dev(data["labels"])
        offsets = torch.arange(0, BOXES * scenes + 1, BOXES, dtype=torch.int32).cuda()
        tdev = torch.from_numpy(trans).cuda()

        def kernel(out=None):
            return ops.box_views(corners, labels, offsets, tdev, VIEWS, cap, "all-xyz", filt, RB.CANVAS, fcorners, out=out)

        def host():
            d = RB.preprocess(data, "all-xyz", False, f3d)
            d = {k: v.cuda() for k, v in d.items()}
            torch.cuda.synchronize()
            return d

        def call():
            return pre(data["corners"], data["labels"], trans, filter_corners=data["filter_corners"])

        if args.trace:
            out = None
            for _ in range(WARM + args.n):
                out = kernel(out)
            torch.cuda.synchronize()
            continue
        out = kernel()
        want, got = host(), call()
        same = all(torch.equal(got[k], want[k]) for k in want)
        for _ in range(5):
            kernel(out), host(), call()
        torch.cuda.synchronize()
        rows = {"kernel": [], "host": [], "call": []}
        for _ in range(args.reps):
            ts = []
            for _ in range(args.n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                kernel(out)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            rows["kernel"].append(med(ts))
            for name, fn in (("host", host), ("call", call)):
                ts = []
                for _ in range(args.n):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    ts.append((time.perf_counter() - t0) * 1e6)
                rows[name].append(med(ts))
        ml = want["masks"].shape[2]
        print("%d scene%s, filter %-10s max_len %3d, cap %d, results equal: %s" % (scenes, " " if scenes == 1 else "s", filt, ml, cap, same))
        for name, what in (("kernel", "device events around the ops.box_views call (launch latency)"),
                           ("host", "numpy restatement + 3 host-to-device copies, wall"),
                           ("call", "BoxPreProcess.__call__, sync=True, wall")):
            v = rows[name]
            print("    %-58s %s   spread %4.1f %%" % (what, "  ".join("%9.1f" % x for x in v), 100 * (max(v) - min(v)) / med(v)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
