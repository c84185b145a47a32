"""Image output: what the last step of the sampling path costs on the GPU, against the host path it replaces.

    python tools/image_output_timing.py                       # device-event / wall-clock medians -> stdout
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o io -- python tools/image_output_timing.py --trace
    python tools/image_output_timing.py --summarise DIR       # kernel time per configuration and its share of the bound

Production sizes only, 6 views, fp16 decoder output in [-1, 1] (the `m11` form decode_images launches).

Default run, after a warm-up of every shape:
  * per reference configuration (dataset.back_resize / back_pad), `ops.image_resample_u8` between a pair of device events,
    median of N >= 25 launches;
  * end to end at the default configuration (224 x 400 -> 896 x 1600, pad (0, 4, 0, 0)), alternating run by run:
      gpu   decode_images(vae, latents, post) and the device-to-host copy of the uint8 frames
      host  decode_latents(vae, latents).cpu(), numpy's (x * 255).round().astype("uint8"), PIL resize + pad per view
    wall clock around work that ends in a synchronising copy, median of N; the PIL leg runs only where PIL is installed,
    and is reported as "not measured" otherwise.

--trace: per configuration N launches between two launches of the one-wave dd_probe_spin kernel; --summarise splits the
kernel trace at those sentinels and prints the median kernel time of dd_image_resample_kernel, the bytes it has to move
(read: 6 x 3 x h x w fp16; written: 6 x H x W x 3 bytes) and the time those take at the HBM peak (8 TB/s) and at the
achievable streaming rate (6.3 TB/s).  Exits non-zero when there is no GPU."""
import argparse
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VIEWS = 6
# (h, w) -> (oh, ow), pad (left, top, right, bottom): configs/dataset/Nuscenes*.yaml back_resize / back_pad
CONFIGS = [((224, 400), (896, 1600), (0, 4, 0, 0)), ((256, 704), (533, 1466), (67, 367, 67, 0)),
           ((432, 768), (900, 1600), (0, 0, 0, 0)), ((192, 384), (800, 1600), (0, 100, 0, 0))]
SENTINEL = "dd_probe_spin_kernel"
KERNEL = "dd_image_resample_kernel"
HBM_PEAK, HBM_STREAM = 8.0e12, 6.3e12


def cfg_name(c):
    return "%dx%d->%dx%d pad %s" % (c[0] + c[1] + (list(c[2]),))


def bytes_moved(c, elem=2):
    (h, w), (oh, ow), (pl, pt, pr, pb) = c
    return VIEWS * 3 * h * w * elem, VIEWS * (pt + oh + pb) * (pl + ow + pr) * 3


def summarise(path):
    import csv
    if os.path.isdir(path):
        found = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
        if not found:
            raise SystemExit("no *kernel_trace.csv under %s" % path)
        path = found[0]
    csv.field_size_limit(1 << 30)
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    marks = [i for i, r in enumerate(rows) if SENTINEL in r[2]]
    if len(marks) != 2 * len(CONFIGS):
        raise SystemExit("expected %d sentinel launches in the trace, found %d" % (2 * len(CONFIGS), len(marks)))
    print("# %s, 6 views, fp16 input: kernel time from the trace (median of the launches between the sentinels)" % KERNEL)
    for i, c in enumerate(CONFIGS):
        win = [e - s for s, e, n in rows[marks[2 * i] + 1:marks[2 * i + 1]] if KERNEL in n]
        other = [n for s, e, n in rows[marks[2 * i] + 1:marks[2 * i + 1]] if KERNEL not in n]
        rd, wr = bytes_moved(c)
        med = statistics.median(win) / 1e3
        print("%-40s %3d launches (%d other kernels)  median %7.2f us  min %7.2f us   read %5.2f MB + written %5.2f MB"
              "   bound %5.2f us at 8 TB/s (%4.1f %% of it), %5.2f us at 6.3 TB/s (%4.1f %%)"
              % (cfg_name(c), len(win), len(other), med, min(win) / 1e3, rd / 1e6, wr / 1e6, (rd + wr) / HBM_PEAK * 1e6,
                 100 * (rd + wr) / HBM_PEAK * 1e6 / med, (rd + wr) / HBM_STREAM * 1e6, 100 * (rd + wr) / HBM_STREAM * 1e6 / med))


def host_path(vae, lat, size, padding, have_pil):
    """Today's path, leg by leg -> (frames or None, seconds per leg)."""
    import torch
    from dualdiff_amd.networks.vae_decoder import decode_latents
    t0 = time.perf_counter()
    img = decode_latents(vae, lat).cpu()                                 # pipeline_bev_controlnet.py:112
    t1 = time.perf_counter()
    arr = (img.flatten(0, 1).permute(0, 2, 3, 1).float().numpy() * 255).round().astype("uint8")
    t2 = time.perf_counter()
    if not have_pil:
        return None, (t1 - t0, t2 - t1, None)
    from PIL import Image
    out = []
    pl, pt, pr, pb = padding
    for a in arr:                                                         # Resize(BICUBIC) then Pad, per view
        r = Image.fromarray(a).resize((size[1], size[0]), Image.BICUBIC)
        p = Image.new("RGB", (pl + size[1] + pr, pt + size[0] + pb), 0)
        p.paste(r, (pl, pt))
        out.append(p)
    t3 = time.perf_counter()
    return out, (t1 - t0, t2 - t1, t3 - t2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30, help="launches / runs per measurement (>= 25)")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarise", metavar="DIR_OR_KERNEL_TRACE_CSV")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    import torch
    if not torch.cuda.is_available():
        print("image_output_timing: no GPU", file=sys.stderr)
        return 2
    if args.n < 25:
        ap.error("--n must be at least 25")
    import numpy as np
    from dualdiff_amd import _native, ops
    dtype = torch.float16
    g = torch.Generator().manual_seed(1)
    xs = {c: (torch.rand((VIEWS, 3) + c[0], generator=g) * 2.2 - 1.1).to(dtype).cuda() for c in CONFIGS}
    outs = {}
    for c in CONFIGS:                                                    # warm-up: builds the device tables, loads the code
        for _ in range(3):
            outs[c] = ops.image_resample_u8(xs[c], c[1], c[2], m11=True)
    torch.cuda.synchronize()

    if args.trace:
        lib = _native.load()
        stamps = torch.zeros(2, dtype=torch.int64, device="cuda")

        def sentinel():
            torch.cuda.synchronize()
            _native.check(lib.dd_probe_spin(stamps.data_ptr(), 100, ops._stream()), "probe_spin")
            torch.cuda.synchronize()
        for c in CONFIGS:
            sentinel()
            for _ in range(args.n):
                ops.image_resample_u8(xs[c], c[1], c[2], m11=True, out=outs[c])
            sentinel()
        return 0

    print("# ops.image_resample_u8, %d views, fp16 input, device events around one launch, median of %d" % (VIEWS, args.n))
    for c in CONFIGS:
        ts = []
        for _ in range(args.n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.image_resample_u8(xs[c], c[1], c[2], m11=True, out=outs[c])
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        rd, wr = bytes_moved(c)
        print("%-40s median %7.1f us  min %7.1f us  (read %5.2f MB, written %5.2f MB; %5.2f us at 8 TB/s)"
              % (cfg_name(c), statistics.median(ts), min(ts), rd / 1e6, wr / 1e6, (rd + wr) / HBM_PEAK * 1e6))

    from dualdiff_amd.networks.layers import device_init_
    from dualdiff_amd.networks.vae_decoder import AutoencoderKLDecoder
    from dualdiff_amd.pipeline.image_output import ImagePostProcess, decode_images
    try:
        import PIL
        have_pil = True
    except ImportError:
        have_pil = False
    (h, w), size, padding = CONFIGS[0]
    with torch.device("cuda"):
        vae = AutoencoderKLDecoder().to(dtype).eval()
    device_init_(vae, 3)
    lat = (torch.randn((1, VIEWS, 4, h // 8, w // 8), generator=g) * 0.5).cuda()
    post = ImagePostProcess(resize=size, padding=padding)
    for _ in range(3):
        frames = decode_images(vae, lat, post).cpu()
        ref, _ = host_path(vae, lat, size, padding, have_pil)
    if ref is not None:
        diff = sum(int((np.asarray(p) != f.numpy()).sum()) for p, f in zip(ref, frames[0]))
        print("# bytes that differ between the two paths' frames: %d of %d" % (diff, frames.numel()))
    gpu_t, legs = [], []
    for _ in range(args.n):                                              # alternating, run by run
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        decode_images(vae, lat, post).cpu()
        gpu_t.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        legs.append(host_path(vae, lat, size, padding, have_pil)[1])
    med = lambda v: statistics.median(v) * 1e3                           # noqa: E731
    print("# end to end, %s, %d views, wall clock in ms, median of %d runs (PIL uses one CPU thread)"
          % (cfg_name(CONFIGS[0]), VIEWS, args.n))
    print("gpu   decode_images + copy of the uint8 frames to the host      %8.2f ms" % med(gpu_t))
    print("host  decode_latents(...).cpu()                                  %8.2f ms" % med([l[0] for l in legs]))
    print("host  (x * 255).round().astype(uint8) in numpy                   %8.2f ms" % med([l[1] for l in legs]))
    if have_pil:
        print("host  PIL %s resize(BICUBIC) + pad, %d views                  %8.2f ms" % (PIL.__version__, VIEWS, med([l[2] for l in legs])))
        print("host  total                                                      %8.2f ms" % med([sum(l) for l in legs]))
    else:
        print("host  PIL resize + pad: not measured (PIL is not installed here)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
