"""PNG output: what encoding the frames on the GPU costs, against the host path it replaces.

    python tools/png_output_timing.py                         # device-event / wall-clock medians -> stdout
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o png -- python tools/png_output_timing.py --trace
    python tools/png_output_timing.py --summarise DIR

Two workloads: one scene of 6 frames of 900 x 1600, and one 448 x 1200 grid (`concat_views` of six 224 x 400 views).  The
content is `smooth`, a low-frequency field with a little noise, what decoded views look like to a lossless coder; for the
scene also `noise` (uniform bytes, every chunk stored) as the other end.

Default run, after a warm-up:
  * `ops.png_encode_u8` between a pair of device events, median of N >= 25 calls (four launches each);
  * end to end, alternating run by run, wall clock around work that ends in a synchronising copy, median of N:
      device  encode_png(frames): the four launches, the readback of the lengths, the copy of the files' bytes
      host    frames.cpu() and `Image.fromarray(a).save(BytesIO(), "PNG")` per frame in one thread
    The host leg runs only where PIL is installed; where it is, the device files are first decoded with PIL and compared
    with the frames, and the two paths' sizes are printed.

--trace: the smooth scene alone, 3 warm-up calls and N more, for the profiler.  --summarise: the four kernels' rows of the profiler's
kernel statistics.  Exits non-zero when there is no GPU."""
import argparse
import csv
import glob
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = (("scene 6 x 900 x 1600", (6, 900, 1600), ("smooth", "noise")), ("grid 1 x 448 x 1200", (1, 448, 1200), ("smooth",)))
KERNELS = ("dd_png_filter_kernel", "dd_png_deflate_kernel", "dd_png_scan_kernel", "dd_png_assemble_kernel")


def make_frames(kind, shape):
    import torch
    m, h, w = shape
    g = torch.Generator().manual_seed(5 if kind == "smooth" else 6)
    if kind == "noise":
        return torch.randint(0, 256, (m, h, w, 3), generator=g, dtype=torch.uint8).cuda()
    low = torch.rand((m, 3, 15, 25), generator=g).cuda()
    x = torch.nn.functional.interpolate(low, size=(h, w), mode="bicubic", align_corners=False)
    x = x + (torch.rand((m, 3, h, w), generator=g).cuda() - 0.5) * 0.03
    return (x.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def summarise(path):
    found = sorted(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True))
    if not found:
        raise SystemExit("no *kernel_stats.csv under %s" % path)
    with open(found[0], newline="") as f:
        rows = [r for r in csv.DictReader(f) if any(k in r["Name"] for k in KERNELS)]
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    for r in rows:
        name = next(k for k in KERNELS if k in r["Name"])
        print("%-24s %4s calls  average %9.2f us  min %9.2f us  max %9.2f us  %5.1f %% of the four"
              % (name, r["Calls"], float(r["AverageNs"]) / 1e3, float(r["MinNs"]) / 1e3, float(r["MaxNs"]) / 1e3,
                 100 * float(r["TotalDurationNs"]) / total))


def host_path(frames, have_pil, **kw):
    """Today's path -> (files or None, seconds of the copy, seconds of the encoder)."""
    t0 = time.perf_counter()
    arr = frames.cpu().numpy()
    t1 = time.perf_counter()
    if not have_pil:
        return None, t1 - t0, None
    from PIL import Image
    files = []
    for a in arr:
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, "PNG", **kw)
        files.append(buf.getvalue())
    return files, t1 - t0, time.perf_counter() - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30, help="calls / runs per measurement (>= 25)")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarise", metavar="DIR")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    import torch
    if not torch.cuda.is_available():
        print("png_output_timing: no GPU", file=sys.stderr)
        return 2
    if args.n < 25:
        ap.error("--n must be at least 25")
    import numpy as np
    from dualdiff_amd import ops
    from dualdiff_amd.pipeline.image_output import encode_png
    try:
        import PIL
        from PIL import Image
        have_pil = True
    except ImportError:
        have_pil = False
    med = lambda v: statistics.median(v) * 1e3                           # noqa: E731
    for title, shape, contents in WORKLOADS:
        for k in contents:
            if args.trace and not (title.startswith("scene") and k == "smooth"):
                continue
            frames = make_frames(k, shape)
            for _ in range(3):                                           # warm-up: workspace, code
                out, lengths = ops.png_encode_u8(frames)
            sizes = lengths.cpu().tolist()
            torch.cuda.synchronize()
            if args.trace:
                for _ in range(args.n):
                    ops.png_encode_u8(frames, out=out)
                torch.cuda.synchronize()
                continue
            ts = []
            for _ in range(args.n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ops.png_encode_u8(frames, out=out)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            print("# %s, %s: ops.png_encode_u8, device events around one call (four launches), median of %d" % (title, k, args.n))
            print("median %8.1f us  min %8.1f us   files %s bytes (%.2f MB of %.2f MB of frames)"
                  % (statistics.median(ts), min(ts), sizes, sum(sizes) / 1e6, frames.numel() / 1e6))
            for _ in range(2):
                dev = encode_png(frames)
                ref, _, _ = host_path(frames, have_pil)
            if ref is not None:
                host = frames.cpu().numpy()
                same = sum(np.array_equal(np.array(Image.open(io.BytesIO(d))), a) for d, a in zip(dev, host))
                level0 = host_path(frames, True, compress_level=0)[0]
                print("# device files that PIL decodes to the frame: %d of %d; sizes device %d, PIL default %d (ratio %.3f), "
                      "PIL compress_level=0 %d" % (same, len(dev), sum(map(len, dev)), sum(map(len, ref)),
                                                  sum(map(len, dev)) / sum(map(len, ref)), sum(map(len, level0))))
            dev_t, legs = [], []
            for _ in range(args.n):                                      # alternating, run by run
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                encode_png(frames)
                dev_t.append(time.perf_counter() - t0)
                legs.append(host_path(frames, have_pil)[1:])
            print("# end to end, wall clock in ms, median of %d runs" % args.n)
            print("device  encode_png: four launches, lengths read back, files copied     %8.2f ms" % med(dev_t))
            print("host    frames.cpu()                                                   %8.2f ms" % med([l[0] for l in legs]))
            if have_pil:
                print("host    PIL %s Image.save(BytesIO, \"PNG\"), %d frames, one thread      %8.2f ms"
                      % (PIL.__version__, shape[0], med([l[1] for l in legs])))
                print("host    total                                                          %8.2f ms" % med([sum(l) for l in legs]))
            else:
                print("host    PIL Image.save: not measured (PIL is not installed here)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
