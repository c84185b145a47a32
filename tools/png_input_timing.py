"""PNG input: what decoding .png files on the GPU costs, against the host path it replaces.

    python tools/png_input_timing.py                          # device-event / wall-clock medians -> stdout
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o png -- python tools/png_input_timing.py --only 2

Four workloads, each against `Image.open(f).convert("RGB")` per file in one thread plus the upload of the frames:
  * one 224 x 2400 RGBA flat-colour panorama of six views, written by PIL (the image-mode ORS condition of one sample);
  * one 432 x 4608 one;
  * a scene of 6 x 900 x 1600 written by `encode_png` (our own format), chunk-parallel and with chunked=False;
  * the same scene written by PIL.
The scene's content is `smooth`, a low-frequency field with a little noise, what decoded views look like to a lossless
coder.  For the panoramas `OccCondition` is timed on top (one more launch).

Per workload, after a warm-up and a check that the frames equal PIL's:
  * `ops.png_decode_u8` between a pair of device events (one memset and its launches), median of N calls;
  * end to end, alternating run by run, wall clock around work that ends in a synchronising copy, median of N:
      device  decode_png(files): the chunk walk with its CRCs, one pinned upload, the launches, the status read back
      host    PIL per file in one thread, np.stack, the upload of the frames
N is --n (25) where a call takes under 50 ms, else 7.  Exits non-zero when there is no GPU or no PIL."""
import argparse
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def panorama(h, w, seed):
    """(h, w, 4) uint8: flat patches of a few class colours per view, alpha 255 but for a band of 0"""
    import numpy as np
    rs = np.random.RandomState(seed)
    img = np.zeros((h, w, 4), dtype=np.uint8)
    img[..., 3] = 255
    colours = rs.randint(0, 256, (18, 3)).astype(np.uint8)
    for _ in range(60 * 6):
        y, x = rs.randint(0, h), rs.randint(0, w)
        img[y:y + rs.randint(4, h // 2), x:x + rs.randint(4, w // 12), :3] = colours[rs.randint(18)]
    img[:h // 8, :, 3] = 0
    return img


def smooth_frames(m, h, w):
    import torch
    g = torch.Generator().manual_seed(5)
    low = torch.rand((m, 3, 15, 25), generator=g).cuda()
    x = torch.nn.functional.interpolate(low, size=(h, w), mode="bicubic", align_corners=False)
    x = x + (torch.rand((m, 3, h, w), generator=g).cuda() - 0.5) * 0.03
    return (x.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def pil_save(a):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, "PNG")
    return buf.getvalue()


def host_path(files):
    import numpy as np
    import torch
    from PIL import Image
    t0 = time.perf_counter()
    arr = np.stack([np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files])
    t1 = time.perf_counter()
    dev = torch.from_numpy(arr).cuda()
    torch.cuda.synchronize()
    return dev, t1 - t0, time.perf_counter() - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=25, help="calls / runs per measurement")
    ap.add_argument("--only", type=int, choices=range(5), help="one workload, by its place in the list above (for the profiler)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("png_input_timing: no GPU", file=sys.stderr)
        return 2
    try:
        import PIL
    except ImportError:
        print("png_input_timing: no PIL to compare with", file=sys.stderr)
        return 2
    from dualdiff_amd import ops
    from dualdiff_amd.pipeline.image_output import encode_png
    from dualdiff_amd.pipeline.png_input import OccCondition, decode_png, upload_png
    print("# %s, PIL %s, torch %s" % (torch.cuda.get_device_name(0), PIL.__version__, torch.__version__))
    scene = smooth_frames(6, 900, 1600)
    own = encode_png(scene)
    by_pil = [pil_save(a) for a in scene.cpu().numpy()]
    work = [("panorama 224 x 2400 RGBA, PIL's file", [pil_save(panorama(224, 2400, 1))], None, True),
            ("panorama 432 x 4608 RGBA, PIL's file", [pil_save(panorama(432, 4608, 2))], None, True),
            ("scene 6 x 900 x 1600, our own files, chunk-parallel", own, None, False),
            ("scene 6 x 900 x 1600, our own files, chunked=False", own, False, False),
            ("scene 6 x 900 x 1600, PIL's files", by_pil, None, False)]
    med = lambda v: statistics.median(v) * 1e3                               # noqa: E731
    for title, files, chunked, condition in (work if args.only is None else [work[args.only]]):
        streams, table, tab, types, h, w = upload_png(files, "cuda")
        for _ in range(2):                                                   # warm-up: workspace, code
            frames, status, paths = ops.png_decode_u8(streams, table, tab, types, h, w, chunked=chunked)
        want = host_path(files)[0]
        same = bool(torch.equal(frames, want)) and status.abs().sum().item() == 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.png_decode_u8(streams, table, tab, types, h, w, chunked=chunked, out=frames)
        torch.cuda.synchronize()
        n = args.n if time.perf_counter() - t0 < 0.05 else 7
        ts = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.png_decode_u8(streams, table, tab, types, h, w, chunked=chunked, out=frames)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        print("# %s: %d files, %.2f MB -> %.2f MB of frames; equal to PIL's: %s; chunk-parallel result used for %d of %d"
              % (title, len(files), sum(map(len, files)) / 1e6, frames.numel() / 1e6, same, int(paths.sum().item()), len(files)))
        print("ops.png_decode_u8, device events around one call, median of %d     %9.3f ms  (min %.3f)" % (n, statistics.median(ts), min(ts)))
        dev_t, legs, cond_t = [], [], []
        for _ in range(n):                                                   # alternating, run by run
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            decode_png(files, chunked=chunked)
            dev_t.append(time.perf_counter() - t0)
            legs.append(host_path(files)[1:])
            if condition:
                t0 = time.perf_counter()
                OccCondition()(files)
                torch.cuda.synchronize()
                cond_t.append(time.perf_counter() - t0)
        print("device  decode_png: chunk walk, upload, launches, status read back    %9.3f ms" % med(dev_t))
        if condition:
            print("device  OccCondition()(files): the same and the condition's launch    %9.3f ms" % med(cond_t))
        print("host    PIL Image.open().convert(\"RGB\"), one thread                    %9.3f ms" % med([l[0] for l in legs]))
        print("host    upload of the frames                                          %9.3f ms" % med([l[1] for l in legs]))
        print("host    total                                                         %9.3f ms" % med([sum(l) for l in legs]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
