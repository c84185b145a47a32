"""JPEG output: what encoding the frames on the GPU costs, against the host path it replaces.

    python tools/jpeg_output_timing.py                        # device-event / wall-clock medians -> stdout
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o jpeg -- python tools/jpeg_output_timing.py --trace --sizes DIR/sizes.json
    python tools/jpeg_output_timing.py --summarise DIR --sizes DIR/sizes.json

One scene, 6 frames of 900 x 1600, two contents as the two ends: `smooth` (a low-frequency field with a little noise, what
decoded views look like to the entropy coder) and `noise` (uniform bytes).

Default run, after a warm-up:
  * `ops.jpeg_encode_u8` between a pair of device events, median of N >= 25 calls (six launches each);
  * end to end, alternating run by run, wall clock around work that ends in a synchronising copy, median of N:
      device  encode_jpeg(frames): the six launches, the readback of the lengths, the copy of the files' bytes
      host    frames.cpu() and `Image.fromarray(a).save(BytesIO(), "JPEG")` per view in one thread
    The host leg runs only where PIL is installed; where it is, the two paths' files are compared first.

--trace: per content N calls between two launches of the one-wave dd_probe_spin kernel, and the files' sizes to --sizes.
--summarise: splits the kernel trace at those sentinels and prints, per launch of the call, the median kernel time, the
bytes the launch has to move and the time those take at the 6.3 TB/s a streaming kernel reaches.  Exits non-zero when there
is no GPU."""
import argparse
import glob
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VIEWS, H, W = 6, 900, 1600
CONTENTS = ("smooth", "noise")
SENTINEL = "dd_probe_spin_kernel"
KERNELS = ("dd_jpeg_blocks_kernel", "dd_jpeg_count_kernel", "dd_jpeg_scan_kernel", "dd_jpeg_emit_kernel",
           "dd_jpeg_ffcount_kernel", "dd_jpeg_assemble_kernel")
HBM_STREAM = 6.3e12
HEADER = 623


def make_frames(kind):
    import torch
    g = torch.Generator().manual_seed(5 if kind == "smooth" else 6)
    if kind == "noise":
        return torch.randint(0, 256, (VIEWS, H, W, 3), generator=g, dtype=torch.uint8).cuda()
    low = torch.rand((VIEWS, 3, 15, 25), generator=g).cuda()
    x = torch.nn.functional.interpolate(low, size=(H, W), mode="bicubic", align_corners=False)
    x = x + (torch.rand((VIEWS, 3, H, W), generator=g).cuda() - 0.5) * 0.03
    return (x.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def traffic(sizes):
    """Bytes each launch reads + writes: the frames, the int16 coefficient workspace (768 bytes per MCU), the per-MCU
    counters, the unstuffed bit stream (the files without header and end marker, less the stuffed zeros: taken as equal)."""
    mcus = VIEWS * ((H + 15) // 16) * ((W + 15) // 16)
    frames, coef, ctr = VIEWS * H * W * 3, mcus * 768, mcus * 4
    stream = sum(sizes) - VIEWS * (HEADER + 2)
    return {"dd_jpeg_blocks_kernel": frames + coef, "dd_jpeg_count_kernel": coef + ctr, "dd_jpeg_scan_kernel": 3 * ctr,
            "dd_jpeg_emit_kernel": coef + ctr + stream, "dd_jpeg_ffcount_kernel": stream,
            "dd_jpeg_assemble_kernel": 2 * stream + VIEWS * HEADER}


def summarise(path, sizes_path):
    import csv
    if os.path.isdir(path):
        found = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
        if not found:
            raise SystemExit("no *kernel_trace.csv under %s" % path)
        path = found[0]
    sizes = json.load(open(sizes_path))
    csv.field_size_limit(1 << 30)
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    marks = [i for i, r in enumerate(rows) if SENTINEL in r[2]]
    if len(marks) != 2 * len(CONTENTS):
        raise SystemExit("expected %d sentinel launches in the trace, found %d" % (2 * len(CONTENTS), len(marks)))
    for i, kind in enumerate(CONTENTS):
        win = rows[marks[2 * i] + 1:marks[2 * i + 1]]
        other = [n for s, e, n in win if not any(k in n for k in KERNELS)]
        print("# %s: %d frames of %d x %d, files %s bytes; kernel time from the trace, median over the calls (%d other kernels)"
              % (kind, VIEWS, H, W, sizes[kind], len(other)))
        moved, total, bound = traffic(sizes[kind]), 0.0, 0.0
        for k in KERNELS:
            t = [e - s for s, e, n in win if k in n]
            med = statistics.median(t) / 1e3
            total += med
            bound += moved[k] / HBM_STREAM * 1e6
            print("%-26s %3d launches  median %8.2f us  min %8.2f us   moves %6.2f MB   %6.2f us at 6.3 TB/s (%4.1f %% of it)"
                  % (k, len(t), med, min(t) / 1e3, moved[k] / 1e6, moved[k] / HBM_STREAM * 1e6,
                     100 * moved[k] / HBM_STREAM * 1e6 / med))
        print("%-26s               sum    %8.2f us                       %6.2f MB   %6.2f us at 6.3 TB/s"
              % ("the six launches", total, sum(moved.values()) / 1e6, bound))


def host_path(frames, have_pil):
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
        Image.fromarray(a).save(buf, "JPEG")
        files.append(buf.getvalue())
    return files, t1 - t0, time.perf_counter() - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30, help="calls / runs per measurement (>= 25)")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarise", metavar="DIR_OR_KERNEL_TRACE_CSV")
    ap.add_argument("--sizes", metavar="JSON", help="--trace writes the files' sizes here, --summarise reads them")
    args = ap.parse_args()
    if args.summarise:
        if not args.sizes:
            ap.error("--summarise needs --sizes")
        return summarise(args.summarise, args.sizes)
    import torch
    if not torch.cuda.is_available():
        print("jpeg_output_timing: no GPU", file=sys.stderr)
        return 2
    if args.n < 25:
        ap.error("--n must be at least 25")
    from dualdiff_amd import _native, ops
    from dualdiff_amd.pipeline.image_output import encode_jpeg
    frames = {k: make_frames(k) for k in CONTENTS}
    outs, sizes = {}, {}
    for k in CONTENTS:                                                   # warm-up: tables, workspace, code
        for _ in range(3):
            outs[k] = ops.jpeg_encode_u8(frames[k])
        sizes[k] = outs[k][1].cpu().tolist()
    torch.cuda.synchronize()

    if args.trace:
        if not args.sizes:
            ap.error("--trace needs --sizes")
        lib = _native.load()
        stamps = torch.zeros(2, dtype=torch.int64, device="cuda")

        def sentinel():
            torch.cuda.synchronize()
            _native.check(lib.dd_probe_spin(stamps.data_ptr(), 100, ops._stream()), "probe_spin")
            torch.cuda.synchronize()
        for k in CONTENTS:
            sentinel()
            for _ in range(args.n):
                ops.jpeg_encode_u8(frames[k], out=outs[k][0])
            sentinel()
        with open(args.sizes, "w") as f:
            json.dump(sizes, f)
        return 0

    print("# ops.jpeg_encode_u8, %d frames of %d x %d, device events around one call (six launches), median of %d"
          % (VIEWS, H, W, args.n))
    for k in CONTENTS:
        ts = []
        for _ in range(args.n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.jpeg_encode_u8(frames[k], out=outs[k][0])
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        print("%-8s median %8.1f us  min %8.1f us   files %s bytes (%.2f MB of %.2f MB of frames)"
              % (k, statistics.median(ts), min(ts), sizes[k], sum(sizes[k]) / 1e6, frames[k].numel() / 1e6))

    try:
        import PIL
        have_pil = True
    except ImportError:
        have_pil = False
    med = lambda v: statistics.median(v) * 1e3                           # noqa: E731
    for k in CONTENTS:
        for _ in range(2):
            dev = encode_jpeg(frames[k])
            ref, _, _ = host_path(frames[k], have_pil)
        if ref is not None:
            print("# %s: files that differ between the two paths: %d of %d" % (k, sum(a != b for a, b in zip(dev, ref)), VIEWS))
        dev_t, legs = [], []
        for _ in range(args.n):                                          # alternating, run by run
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            encode_jpeg(frames[k])
            dev_t.append(time.perf_counter() - t0)
            legs.append(host_path(frames[k], have_pil)[1:])
        print("# end to end, %s, %d frames of %d x %d, wall clock in ms, median of %d runs" % (k, VIEWS, H, W, args.n))
        print("device  encode_jpeg: six launches, lengths read back, files copied     %8.2f ms" % med(dev_t))
        print("host    frames.cpu()                                                   %8.2f ms" % med([l[0] for l in legs]))
        if have_pil:
            print("host    PIL %s Image.save(BytesIO, \"JPEG\"), %d views, one thread      %8.2f ms"
                  % (PIL.__version__, VIEWS, med([l[1] for l in legs])))
            print("host    total                                                          %8.2f ms" % med([sum(l) for l in legs]))
        else:
            print("host    PIL Image.save: not measured (PIL is not installed here)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
