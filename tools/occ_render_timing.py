"""The ORS panorama (`OccRender`, dd_ors_first_hit): what it costs on the GPU, against the composition it replaces.

    python tools/occ_render_timing.py                      # device-event / wall-clock medians -> stdout
    python tools/occ_render_timing.py --host               # the host path only (no GPU needed): see below
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o occ -- python tools/occ_render_timing.py --trace

The fixture volume and rig (tests/golden/cases.py: ors_inputs) at the two sizes a user runs: 6 x 224 x 400 rays
(`OccRender.for_image_size([224, 400])`) and 6 x 432 x 768 (`[432, 768]`), 320 samples of 0.2 m, modes all / bg / fg.
Per size and mode, after a warm-up and a comparison of the results:
  * the one launch from a volume and ray tables already on the device, between a pair of device events, median of N;
  * the whole `OccRender.__call__` from a host volume with a warm ray cache (the 640 KB upload, the rig index, the
    launch), wall clock around a device synchronise, median of N;
  * (a) the composition this replaces: `OccupancyRay.project_volume` (every sample's label, uint8, then int64) and the
    reference's first-hit and palette lines as torch on the GPU, between device events, alternating with ours;
  * the bytes each path writes, and the share of the n x hw x samples lookups the launch makes with each of its two early
    exits on and off (`exits`: bit 0 stop at the hit, bit 1 stop once out of the volume for good).
--host: (b) the CPU restatement of the reference's path (oracle labels + first hit + palette, tests/occ_render_reference.py)
with 16 threads, wall clock; it needs no GPU and says nothing about one.
--trace: N launches per size in mode bg and nothing else, for a profiler run of its own.  Exits non-zero without a GPU."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ([224, 400], [432, 768])
MODES = ("all", "bg", "fg")


def composition(proj, occ, Ks, Rts, mode, palette):
    """(a): every label, then occ3d_proj.py:156-197 as torch on the device"""
    import torch
    lab = proj.project_volume(occ, Ks, Rts)                                   # (n, h, w, S) int64
    if mode == "bg":
        lab = torch.where(lab <= 10, 17, lab)
    elif mode == "fg":
        lab = torch.where(11 <= lab, 17, lab)
    flat = lab.view(-1, lab.shape[-1])
    idx = (flat != 17).float().argmax(dim=1)
    val = flat[torch.arange(flat.size(0), device=flat.device), idx].view(lab.shape[:3])
    img = palette[val]                                                        # (n, h, w, 3)
    return torch.cat([img[i] for i in range(img.shape[0])], dim=-2), val


def host(args):
    import torch
    from tests import occ_render_reference as R
    from tests.golden import cases as C
    torch.set_num_threads(16)
    occ, Ks, Rts = C.ors_inputs()
    for size in SIZES:
        h, w = size
        ratio = w / 1600
        for mode in MODES if size == SIZES[0] else ("bg",):                   # the large size once: minutes of host time
            ts = []
            for _ in range(args.host_runs if size == SIZES[0] else 1):
                t0 = time.perf_counter()
                R.render(occ, Ks, Rts, h, w, ratio, 320, 0.2, mode)
                ts.append(time.perf_counter() - t0)
            print("host    %d x %d, %-3s: oracle labels + first hit + palette, %d threads, median of %d   %9.1f ms"
                  % (h, w, mode, torch.get_num_threads(), len(ts), statistics.median(ts) * 1e3), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30, help="calls per measurement (>= 25)")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--host-runs", type=int, default=3)
    args = ap.parse_args()
    if args.host:
        return host(args)
    import torch
    if not torch.cuda.is_available():
        print("occ_render_timing: no GPU", file=sys.stderr)
        return 2
    if args.n < 25:
        ap.error("--n must be at least 25")
    from dualdiff_amd import ops as O
    from dualdiff_amd.pipeline.occ_render import OCC_COLORS, OccRender
    from tests.golden import cases as C
    occ, Ks, Rts = C.ors_inputs()
    occ_host = occ.to(torch.uint8)
    print("# %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))

    def events(fn):
        ts = []
        for _ in range(args.n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return statistics.median(ts), min(ts)

    palette = torch.tensor(OCC_COLORS, dtype=torch.uint8, device="cuda")
    for size in SIZES:
        render = {m: OccRender.for_image_size(size, mode=m) for m in MODES}
        proj = render["bg"].projector
        h, w = proj.image_shape_compress
        s, step = proj.sample_point, proj.sample_step
        origin, direction = proj.rays(Ks, Rts)
        for m in MODES:
            render[m].projector._ray_cache = proj._ray_cache                  # one table for the three modes
        vol = proj._volumes([occ_host])
        rays = 6 * h * w
        launch = lambda m, **kw: O.ors_first_hit(vol, origin[None], direction[None], [0], (h, w), s, step, mode=m,   # noqa: E731
                                                 palette=OCC_COLORS, **kw)
        for m in MODES:                                                       # warm-up
            launch(m, want_classes=True)
            render[m]([occ_host], (Ks, Rts))
        torch.cuda.synchronize()
        if args.trace:
            for _ in range(args.n):
                launch("bg")
            torch.cuda.synchronize()
            continue
        print("# %d x %d per view: %d rays x %d samples = %.1f M lookups at most; the launch writes %d B per ray (%.2f MB: frames; "
              "+1 B per ray with the classes); (a) writes %d B per ray of uint8 labels (%.0f MB) and %d B per ray of int64 labels "
              "(%.0f MB) before its first-hit passes" % (h, w, rays, s, rays * s / 1e6, 3, rays * 3 / 1e6, s, rays * s / 1e6, 8 * s,
                                                          rays * s * 8 / 1e6))
        for m in MODES:
            frames, cls = launch(m, want_classes=True)
            want_f, want_c = composition(proj, occ_host, Ks, Rts, m, palette)
            assert torch.equal(frames[0], want_f) and torch.equal(cls[0].long(), want_c), m
            del want_f, want_c
            shares = []
            for exits in (0, 1, 2, 3):
                f2, _, visited = launch(m, want_visited=True, exits=exits)
                assert torch.equal(f2, frames)
                shares.append(float(visited.sum()) / (rays * s))
            ours, theirs = [], []
            for _ in range(3):                                                # alternating
                ours.append(events(lambda: launch(m)))
                theirs.append(events(lambda: composition(proj, occ_host, Ks, Rts, m, palette)))
            wall = []
            for _ in range(args.n):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                render[m]([occ_host], (Ks, Rts))
                torch.cuda.synchronize()
                wall.append(time.perf_counter() - t0)
            print("%-3s  hit share %.3f; lookups made: no exit %.3f, hit only %.3f, leaving only %.3f, both %.3f of n x hw x S"
                  % (m, float((cls != 17).float().mean()), *shares))
            print("     one launch, device events, median of %d (3 rounds)  %s us   (min %.1f)"
                  % (args.n, " / ".join("%.1f" % o[0] for o in ours), min(o[1] for o in ours)))
            print("     (a) project_volume + torch first hit, device events   %s us   (min %.1f)"
                  % (" / ".join("%.1f" % t[0] for t in theirs), min(t[1] for t in theirs)))
            print("     OccRender.__call__ from a host volume, warm ray cache, wall clock, median of %d   %.3f ms"
                  % (args.n, statistics.median(wall) * 1e3), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
