"""CLIP text encoder: the HIP model (dualdiff_amd.networks.text_encoder.CLIPTextModel, eager launches) against the same
network in eager PyTorch-ROCm (tests/clip_text_reference.py moved to the GPU in fp16 — the torch ops a user's
`transformers` encoder issues today), both in ONE process, alternating forward by forward.

    python tools/text_encoder_timing.py                       # device-event medians -> stdout
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o te -- python tools/text_encoder_timing.py --trace
    python tools/text_encoder_timing.py --summarise DIR/te_kernel_trace.csv

Timing: per shape (b, l) in (2, 77), (7, 77), (28, 77), after a warm-up of every shape on both paths (which also tunes the
GEMM shapes that are not in the tracked table), REPS repetitions of N >= 25 forwards per path, each forward bracketed by
its own pair of device events; the median of a repetition is one sample, and the spread over the repetitions (max - min of
the medians) is reported for both paths.  Exits non-zero when there is no GPU.

--trace: for every shape and path, a few warm-up forwards, then N forwards between two launches of the one-wave
dd_probe_spin kernel; --summarise splits the kernel trace at those sentinels and prints launches per forward, and for the
HIP path the causal attention kernel's share of the kernel time and its time per call."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(2, 77), (7, 77), (28, 77)]
SENTINEL = "dd_probe_spin_kernel"
TRACE_N = 10


def summarise(path):
    import collections
    import csv
    csv.field_size_limit(1 << 30)
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    marks = [i for i, r in enumerate(rows) if SENTINEL in r[2]]
    want = 2 * 2 * len(SHAPES)
    if len(marks) != want:
        raise SystemExit("expected %d sentinel launches in the trace, found %d" % (want, len(marks)))
    seg = 0
    for b, l in SHAPES:
        for path_name in ("hip", "torch"):
            win = rows[marks[2 * seg] + 1:marks[2 * seg + 1]]
            seg += 1
            busy, cnt = collections.Counter(), collections.Counter()
            for s, e, n in win:
                key = "dd_causal_attn_kernel" if "dd_causal_attn_kernel" in n else \
                    "dd_* other" if "dd_" in n else "torch / rocBLAS"
                busy[key] += e - s
                cnt[key] += 1
            total = sum(busy.values())
            print("(%d, %d) %-5s %6.1f launches/forward  kernel time %8.1f us/forward  wall %8.1f us/forward"
                  % (b, l, path_name, len(win) / TRACE_N, total / TRACE_N / 1e3,
                     (max(r[1] for r in win) - win[0][0]) / TRACE_N / 1e3))
            for k, v in busy.most_common():
                print("      %-24s %6.1f launches/forward  %8.1f us/forward (%4.1f%% of kernel time)  %6.2f us/call"
                      % (k, cnt[k] / TRACE_N, v / TRACE_N / 1e3, 100.0 * v / total, v / cnt[k] / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30, help="forwards per path and repetition (>= 25)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarise", metavar="KERNEL_TRACE_CSV")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    import torch
    if not torch.cuda.is_available():
        print("text_encoder_timing: no GPU", file=sys.stderr)
        return 2
    if args.n < 25:
        ap.error("--n must be at least 25")
    from dualdiff_amd import _native, ops
    from dualdiff_amd.networks.text_encoder import CLIPTextModel
    from oracle.init_utils import seeded_state_dict
    from tests import clip_text_reference as RT

    dtype = torch.float16
    base = RT.CLIPTextModel().eval()
    sd = {k: v.to(dtype).float() for k, v in seeded_state_dict(base, RT.GOLDEN_SEED).items()}
    base.load_state_dict(sd)
    hip = CLIPTextModel()
    hip.load_state_dict(sd)
    hip = hip.to("cuda", dtype).eval()
    base = base.to("cuda", dtype)
    ids = {s: RT.seeded_ids(s[0], s[1], 900 + s[0]).cuda() for s in SHAPES}

    def run_hip(x):
        return hip(x)[0]

    def run_base(x):
        with torch.no_grad():
            return base(x)[0]

    paths = (("hip", run_hip), ("torch", run_base))
    for s in SHAPES:                                   # warm-up of every shape on both paths (tunes unknown GEMM shapes)
        for _ in range(3):
            for _, fn in paths:
                fn(ids[s])
    torch.cuda.synchronize()
    for s in SHAPES:
        a, b_ = run_hip(ids[s]).float(), run_base(ids[s]).float()
        print("# (%d, %d) rel-L2 between the two paths: %.2e" % (s[0], s[1], ((a - b_).norm() / b_.norm()).item()))

    if args.trace:
        lib = _native.load()
        stamps = torch.zeros(2, dtype=torch.int64, device="cuda")

        def sentinel():
            torch.cuda.synchronize()
            _native.check(lib.dd_probe_spin(stamps.data_ptr(), 100, ops._stream()), "probe_spin")
            torch.cuda.synchronize()

        for s in SHAPES:
            for _, fn in paths:
                fn(ids[s])
                sentinel()
                for _ in range(TRACE_N):
                    fn(ids[s])
                sentinel()
        return 0

    print("# fp16, eager launches, device-event time per forward in us: median of %d forwards, %d repetitions" % (args.n, args.reps))
    worst = 0.0
    for s in SHAPES:
        med = {"hip": [], "torch": []}
        for _ in range(args.reps):
            t = {"hip": [], "torch": []}
            for _ in range(args.n):
                for name, fn in paths:                 # alternating, forward by forward
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn(ids[s])
                    e1.record()
                    e1.synchronize()
                    t[name].append(e0.elapsed_time(e1) * 1e3)
            for name in t:
                med[name].append(statistics.median(t[name]))
        h, b_ = statistics.median(med["hip"]), statistics.median(med["torch"])
        sh, sb = max(med["hip"]) - min(med["hip"]), max(med["torch"]) - min(med["torch"])
        print("(%2d, %d)  hip %8.1f us (spread %5.1f)   torch eager %8.1f us (spread %5.1f)   torch / hip = %.2f"
              % (s[0], s[1], h, sh, b_, sb, b_ / h))
        worst = max(worst, h - (b_ + sb))
    print("# hip slower than torch eager beyond its spread at some shape: %s" % ("YES" if worst > 0 else "no"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
