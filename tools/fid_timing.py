"""FID feature extractor: the HIP InceptionV3 (dualdiff_amd.networks.inception, fp16, eager launches) timed per forward
and per layer class, against the fp32 restatement (tests/inception_reference.py — the network the reference's
tools/fid_score.py runs, here with seeded weights) on 16 host threads.

    python tools/fid_timing.py                  # -> stdout; profiles/fid.txt holds one such run

Per batch size (50: get_activations' batch; 6: one sample's views), 224 x 400 fp32 images in [0, 1] resized to 299 x 299
by the network's own input kernel:
  * device-event time of features(x, 2048), median of N forwards per repetition, spread over the repetitions;
  * one forward under ops.KernelTimer (one event pair per launch, overhead calibrated and subtracted), launches grouped by
    layer class — stem convs, the 35 x 35 / 17 x 17 / 8 x 8 levels, pools, input, global average — with algorithmic FLOPs
    and achieved TFLOP/s beside the 2500 TFLOP/s MFMA figure of DESIGN.md section 5;
  * the same forward of the fp32 restatement on the host (torch.set_num_threads(16)), wall clock, best of 2.
Exits non-zero when there is no GPU."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 2500.0
BATCHES = (50, 6)
SRC = (224, 400)


def layer_class(name, m):
    """Class of one timed launch from its booked name (ops.conv2d / pool3x3 under KernelTimer(shapes=True))."""
    if name.startswith("dd_inception_input"):
        return "input"
    if name.startswith("dd_global_avgpool"):
        return "global avg"
    rows = int(name.rsplit(" ", 1)[1].split("x")[0])
    kind = "pool" if name.startswith("dd_pool3x3") else "conv"
    level = {35 * 35: "35x35", 17 * 17: "17x17", 8 * 8: "8x8"}.get(rows // m, "stem")
    return "%s %s" % (kind, level)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10, help="forwards per repetition")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the fp32 host comparison")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("fid_timing: no GPU", file=sys.stderr)
        return 2
    from dualdiff_amd import ops
    from dualdiff_amd.networks.inception import InceptionV3
    from tests import inception_reference as R

    sd = R.seeded_state_dict(R.WEIGHT_SEED)
    hip = InceptionV3(dtype=torch.float16)
    hip.load_state_dict(sd)
    hip = hip.to("cuda")
    host = R.InceptionV3().eval()
    host.load_state_dict(sd)
    torch.set_num_threads(16)
    print("# %s, fp16 activations, eager launches; images %d x %d -> 299 x 299" % (torch.cuda.get_device_name(0), *SRC))
    for m in BATCHES:
        x = R.seeded_images((m, 3) + SRC, 40 + m)
        xd = x.cuda()
        for _ in range(3):
            hip.features(xd)
        torch.cuda.synchronize()
        meds = []
        for _ in range(args.reps):
            t = []
            for _ in range(args.n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                hip.features(xd)
                e1.record()
                e1.synchronize()
                t.append(e0.elapsed_time(e1))
            meds.append(statistics.median(t))
        fwd = statistics.median(meds)
        timer = ops.KernelTimer(shapes=True)
        timer.calibrate()
        ops.set_timer(timer)
        try:
            hip.features(xd)
            summ = timer.summary()
        finally:
            ops.set_timer(None)
        classes = {}
        for name, d in summ.items():
            c = classes.setdefault(layer_class(name, m), {"n": 0, "ms": 0.0, "flops": 0.0, "bytes": 0.0})
            c["n"] += d["count"]
            c["ms"] += d["ms"]
            c["flops"] += d["flops"]
            c["bytes"] += d["bytes"]
        flops = sum(c["flops"] for c in classes.values())
        print("batch %2d: forward %8.3f ms (spread %.3f over %d repetitions of %d)  %7.1f images/s  %.2f GFLOP/image  "
              "%6.1f TFLOP/s = %.3f of %g" % (m, fwd, max(meds) - min(meds), args.reps, args.n, m / fwd * 1e3,
                                            flops / m / 1e9, flops / fwd / 1e9, flops / fwd / 1e9 / PEAK_TFLOPS, PEAK_TFLOPS))
        print("  %-14s %4s %10s %10s %9s %8s" % ("class", "n", "kernel ms", "GFLOP", "TFLOP/s", "GB/s"))
        for k in sorted(classes, key=lambda k: -classes[k]["ms"]):
            c = classes[k]
            ms = max(c["ms"], 1e-6)
            print("  %-14s %4d %10.3f %10.2f %9.1f %8.0f" % (k, c["n"], c["ms"], c["flops"] / 1e9, c["flops"] / ms / 1e9,
                                                             c["bytes"] / ms / 1e6))
        print("  %-14s %4d %10.3f   (sum of bracketed kernel times; overhead %.1f us per bracket subtracted)"
              % ("all", sum(c["n"] for c in classes.values()), sum(c["ms"] for c in classes.values()), timer.overhead_ms * 1e3))
        if not args.no_host:
            best = None
            with torch.no_grad():
                for _ in range(2):
                    t0 = time.perf_counter()
                    ref = host.features(x)
                    dt = (time.perf_counter() - t0) * 1e3
                    best = dt if best is None else min(best, dt)
            y = hip.features(xd).cpu()
            print("  fp32 restatement on 16 host threads: %9.1f ms (best of 2) = %.0f x the HIP forward; rel-L2 between them %.2e"
                  % (best, best / fwd, ((y - ref).norm() / ref.norm()).item()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
