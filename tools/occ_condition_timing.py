"""The resized ORS condition (image_size [192, 384], `crop_drivewm`): what it costs on the GPU, against the host path it
replaces.

    python tools/occ_condition_timing.py                      # device-event / wall-clock medians -> stdout
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o occ -- python tools/occ_condition_timing.py --trace

b = 1 and b = 4 panoramas of the reference's size, 224 x 2400 RGBA (six views of 224 x 400), flat patches of class colours
as the condition's files are, written here with zlib.  Per batch size, after a warm-up and a comparison of the two results:
  * `ResizedOccCondition.drivewm()` from uint8 frames on the device — one launch of dd_png_condition_resize_kernel —
    between a pair of device events, median of N calls, beside the bytes it moves and what they take at the HBM rates;
  * the same from `bytes` between device events: the chunk walk and the pinned upload on the host, `ops.png_decode_u8`'s
    launches, the status read-back, then the condition's launch;
  * end to end, alternating run by run, wall clock around work that ends in a device synchronise, median of N:
      device  frames on the device -> condition;   files -> condition
      host    the reference's collate step with torch on the CPU — per sample and view pad_top, F.interpolate(bilinear,
              align_corners=False), the crop, cat; stack — from ToTensor() panoramas already in memory, plus the upload of
              the result.  With torch's default thread count and with one thread.
--trace: N calls from frames per batch size and nothing else, for a profiler run of its own.  Exits non-zero without a GPU."""
import argparse
import os
import statistics
import struct
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VIEWS, H, W = 6, 224, 400
PAD, RESIZE, OUT = 1, (216, 384), (192, 384)
HBM_PEAK, HBM_STREAM = 8.0e12, 6.3e12


def panorama(seed):
    """(H, VIEWS * W, 4) uint8: flat patches of a few class colours, alpha 255 but for a band of 0"""
    import numpy as np
    rs = np.random.RandomState(seed)
    img = np.zeros((H, VIEWS * W, 4), dtype=np.uint8)
    img[..., 3] = 255
    colours = rs.randint(0, 256, (18, 3)).astype(np.uint8)
    for _ in range(60 * VIEWS):
        y, x = rs.randint(0, H), rs.randint(0, VIEWS * W)
        img[y:y + rs.randint(4, H // 2), x:x + rs.randint(4, W // 2), :3] = colours[rs.randint(18)]
    img[:H // 8, :, 3] = 0
    return img


def png_rgba(img):
    """an RGBA file with every row's filter type 0"""
    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))
    h, w = img.shape[:2]
    rows = b"".join(b"\x00" + img[y].tobytes() for y in range(h))
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(rows))
            + chunk(b"IEND", b""))


def host_path(x):
    """x: float32 (b, 3, H, VIEWS * W) on the host, the ToTensor() panoramas -> the condition on the device"""
    import torch
    import torch.nn.functional as F
    t0 = time.perf_counter()
    samples = []
    for s in x:
        parts = []
        for v in range(VIEWS):
            padded = torch.zeros((3, H + PAD, W))
            padded[:, PAD:] = s[:, :, v * W:(v + 1) * W]
            r = F.interpolate(padded[None], size=RESIZE, mode="bilinear", align_corners=False)[0]
            parts.append(r[:, RESIZE[0] - OUT[0]:, (RESIZE[1] - OUT[1]) // 2:RESIZE[1] - (RESIZE[1] - OUT[1]) // 2])
        samples.append(torch.cat(parts, dim=-1))
    out = torch.stack(samples)
    t1 = time.perf_counter()
    dev = out.cuda()
    torch.cuda.synchronize()
    return dev, t1 - t0, time.perf_counter() - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30, help="calls / runs per measurement (>= 25)")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("occ_condition_timing: no GPU", file=sys.stderr)
        return 2
    if args.n < 25:
        ap.error("--n must be at least 25")
    import numpy as np
    from dualdiff_amd.pipeline.png_input import ResizedOccCondition, decode_png
    occ = ResizedOccCondition.drivewm()
    threads = torch.get_num_threads()
    print("# %s, torch %s, %d CPU threads by default" % (torch.cuda.get_device_name(0), torch.__version__, threads))
    med = lambda v: statistics.median(v) * 1e3                               # noqa: E731

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

    for b in (1, 4):
        imgs = [panorama(10 * b + i) for i in range(b)]
        files = [png_rgba(a) for a in imgs]
        frames = decode_png(files)
        assert torch.equal(frames.cpu(), torch.from_numpy(np.stack([a[..., :3] for a in imgs])))
        for _ in range(3):                                                   # warm-up: the tables, the code, the workspace
            got = occ(frames)
            occ(files)
        torch.cuda.synchronize()
        if args.trace:
            for _ in range(args.n):
                occ(frames)
            torch.cuda.synchronize()
            continue
        x = torch.from_numpy(np.stack([a[..., :3] for a in imgs])).permute(0, 3, 1, 2).float().div(255).contiguous()
        want = host_path(x)[0]
        torch.set_num_threads(1)
        want1 = host_path(x)[0]
        torch.set_num_threads(threads)
        rd, wr = frames.numel(), got.numel() * 4
        print("# b = %d: %d files, %.3f MB -> frames %.2f MB -> condition %s, %.2f MB; elements that differ from torch's CPU result: "
              "%d (default threads, max %.3g), %d (one thread, max %.3g) of %d"
              % (b, b, sum(map(len, files)) / 1e6, rd / 1e6, tuple(got.shape), wr / 1e6, int((got != want).sum()),
                 float((got - want).abs().max()), int((got != want1).sum()), float((got - want1).abs().max()), got.numel()))
        m, lo = events(lambda: occ(frames))
        print("device  from frames, device events around the one launch, median of %d   %9.1f us  (min %.1f; %.2f MB read + %.2f MB "
              "written: %.2f us at 8 TB/s, %.2f us at 6.3 TB/s)"
              % (args.n, m, lo, rd / 1e6, wr / 1e6, (rd + wr) / HBM_PEAK * 1e6, (rd + wr) / HBM_STREAM * 1e6))
        m, lo = events(lambda: occ(files))
        print("device  from bytes, device events around the whole call, median of %d    %9.1f us  (min %.1f)" % (args.n, m, lo))
        fr_t, by_t, legs, legs1 = [], [], [], []
        for _ in range(args.n):                                              # alternating, run by run
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            occ(frames)
            torch.cuda.synchronize()
            fr_t.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            occ(files)
            torch.cuda.synchronize()
            by_t.append(time.perf_counter() - t0)
            legs.append(host_path(x)[1:])
            torch.set_num_threads(1)
            legs1.append(host_path(x)[1:])
            torch.set_num_threads(threads)
        print("device  frames -> condition, wall clock                                  %9.3f ms" % med(fr_t))
        print("device  files -> condition, wall clock                                   %9.3f ms" % med(by_t))
        for name, l in (("%d threads" % threads, legs), ("one thread", legs1)):
            print("host    torch pad / interpolate / crop / cat per view, %-12s %9.3f ms + upload %7.3f ms = %9.3f ms"
                  % (name + ":", med([t[0] for t in l]), med([t[1] for t in l]), med([sum(t) for t in l])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
