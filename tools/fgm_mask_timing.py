"""FGM loss mask and loss (`FgmMask`: dd_fgm_box_records + dd_fgm_mask; `fgm_loss`: dd_fgm_loss): what they cost on the GPU.

    python tools/fgm_mask_timing.py                        # device-event / wall-clock medians -> stdout
    rocprofv3 --kernel-trace --output-format csv -d DIR -o fgm -- python tools/fgm_mask_timing.py --trace
    python tools/fgm_mask_timing.py --summarise DIR        # the kernels' own durations out of that run

One scene of 6 views x 40 boxes, every box with a corner on the grid (tests/fgm_reference.py: scenes, seeded — the scene
tests/golden/mint_fgm_mask.py times the reference's own lines on), at the grids (50, 28) and (96, 54).  Per grid, after a
comparison with the numpy restatement:
  * `ops.fgm_mask` (both launches) from device tensors, the workspace allocated once, between a pair of device events,
    median of N, three rounds;
  * the whole `FgmMask.__call__` from device tensors followed by a device synchronise, and with check=True (the 4-byte
    readback instead), wall clock, median of N;
  * the numpy restatement on one host thread, wall clock (the reference's own lines need scipy and matplotlib: the mint
    script times them where they are installed).
Then `ops.fgm_loss` with the gradient at (1, 6, 4, 28, 50) and (2, 6, 4, 54, 96), fp16, the same way.
--trace: N calls of each per grid and nothing else, for a profiler run of its own."""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import fgm_reference as R  # noqa: E402

GRIDS = ((50, 28), (96, 54))
LOSS_SHAPES = ((1, 6, 4, 28, 50), (2, 6, 4, 54, 96))
KERNELS = ("dd_fgm_box_records_kernel", "dd_fgm_mask_kernel", "dd_fgm_loss_partials_kernel", "dd_fgm_loss_final_kernel")


def median_ms(fn, n):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


def summarise(folder):
    rows = []
    for path in glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += [r for r in csv.DictReader(f) if "dd_fgm_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for name in KERNELS:
        mine = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        half = len(mine) // 2
        for label, part in (("first shape", mine[:half]), ("second shape", mine[half:])):
            part = part[len(part) // 4:]                                   # the warm launches
            if part:
                print("%s, %s: last %d launches median %.2f us, min %.2f, max %.2f"
                      % (name, label, len(part), statistics.median(part), min(part), max(part)))


def device_events(torch, launch, n):
    rounds = []
    for _ in range(3):
        ts = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b) * 1e3)
        rounds.append(ts)
    return " / ".join("%.1f" % statistics.median(t) for t in rounds), min(min(t) for t in rounds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarise")
    ap.add_argument("-n", type=int, default=30)
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    import torch
    from dualdiff_amd import ops
    from dualdiff_amd.pipeline.fgm_mask import FgmMask
    if not torch.cuda.is_available():
        sys.exit("no GPU")
    if not args.trace:
        print("# %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    host = R.scenes(22277, ((40,) * 6,), 40, visible=(50, 28))
    bboxes, masks, l2i = (torch.from_numpy(a).cuda() for a in host)
    ws = torch.empty((ops.fgm_workspace_bytes(240),), dtype=torch.uint8, device="cuda")
    for grid in GRIDS:
        def launch():
            return ops.fgm_mask(bboxes, masks, l2i, grid, workspace=ws)
        for _ in range(args.n // 3 + 1):
            heat, flags = launch()
        torch.cuda.synchronize()
        if args.trace:
            for _ in range(args.n):
                launch()
            torch.cuda.synchronize()
            continue
        ref = R.heatmap(*host, grid)
        print("%s, 6 views x 40 boxes: equal to the numpy restatement: %s; %.0f %% of the pixels painted; flags %d"
              % (grid, torch.equal(heat.cpu(), torch.from_numpy(ref["heat"])), 100 * (ref["heat"] != 0).mean(), int(flags.item())))
        meds, low = device_events(torch, launch, args.n)
        print("     both launches, device events, median of %d (3 rounds)  %s us   (min %.1f)" % (args.n, meds, low))
        fm = FgmMask(grid)

        def whole(check):
            out = fm(bboxes, masks, l2i, check=check)
            if not check:
                torch.cuda.synchronize()
            return out
        for check in (False, True):
            whole(check)
            med, low = median_ms(lambda: whole(check), args.n)
            print("     FgmMask.__call__ from device tensors, check=%s, wall clock, median of %d   %.3f ms (min %.3f)"
                  % (check, args.n, med, low))
        med, low = median_ms(lambda: R.heatmap(*host, grid), 3)
        print("     the numpy restatement, one host thread, median of 3   %.1f ms (min %.1f)" % (med, low))
    for shape in LOSS_SHAPES:
        g = torch.Generator().manual_seed(1)
        pred, target = (torch.randn(shape, generator=g).half().cuda() for _ in range(2))
        heat = torch.rand(shape[:2] + shape[3:], generator=g).cuda()

        def launch():
            return ops.fgm_loss(pred, target, heat, want_grad=True)
        for _ in range(args.n // 3 + 1):
            launch()
        torch.cuda.synchronize()
        if args.trace:
            for _ in range(args.n):
                launch()
            torch.cuda.synchronize()
            continue
        meds, low = device_events(torch, launch, args.n)
        print("fgm_loss with gradient, fp16 %s: both launches, device events, median of %d (3 rounds)  %s us   (min %.1f)"
              % (shape, args.n, meds, low))

        def eager():
            p = pred.clone().requires_grad_(True)
            loss = torch.nn.functional.mse_loss(p.float(), target.float(), reduction="none")
            loss = loss.mean() + (loss * heat.unsqueeze(2)).mean()
            loss.backward()
            return p.grad
        for _ in range(3):
            eager()
        meds, low = device_events(torch, eager, args.n)
        print("     the reference's two lines and their backward in eager torch: device events  %s us   (min %.1f)" % (meds, low))


if __name__ == "__main__":
    main()
