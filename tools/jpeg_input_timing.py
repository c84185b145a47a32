"""JPEG input: what decoding camera files on the GPU costs, against the host path it replaces.

    python tools/jpeg_input_timing.py --build-variants        # (no GPU needed) csrc/jpeg_decode.hip alone at other S
    python tools/jpeg_input_timing.py                         # device-event / wall-clock medians, the sweeps -> stdout
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o jpegd -- python tools/jpeg_input_timing.py --trace
    python tools/jpeg_input_timing.py --summarise DIR

One scene, 6 files of 900 x 1600 at quality 75 and at quality 95: a low-frequency field with sensor-like noise, encoded by
the package's own encoder (the bytes PIL writes, tests/test_jpeg_output_gpu.py).

Default run, after a warm-up:
  * `ops.jpeg_decode_u8` on uploaded bytes between a pair of device events, median of N >= 25 calls, at rounds 0..12;
  * the same call through every variant library `--build-variants` left under build/jpeg_input/ (S = 256 .. 4096 bits per
    subsequence; the library proper is S = DD_JPEG_SUB_BITS), at rounds 1..8;
  * how many subsequences the repair pass decodes again at each (S, rounds): tools/jpeg_decode_host_check.cpp, compiled here
    without sanitizers at that S, runs the same core over the same files and counts them;
  * end to end, alternating run by run, wall clock from `bytes` on the host to frames on the device, median of N:
      device  decode_jpeg(files): header walk, one pinned upload, one call, the status read back
      host    `Image.open(BytesIO(f)).convert("RGB")` per file in one thread, np.stack, one upload of the frames
    The host leg runs only where PIL is installed; where it is, the two paths' frames are compared first.

--trace: per quality N calls between two launches of the one-wave dd_probe_spin kernel.
--summarise: splits the kernel trace at those sentinels and prints the median kernel time per launch of the call.
Exits non-zero when there is no GPU."""
import argparse
import ctypes
import glob
import io
import os
import re
import shutil
import statistics
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VIEWS, H, W = 6, 900, 1600
QUALITIES = (75, 95)
VARIANTS = (256, 512, 2048, 4096)
VARIANT_ROUNDS = (1, 2, 3, 4, 5, 6, 8)
VARIANT_DIR = os.path.join(ROOT, "build", "jpeg_input")
SENTINEL = "dd_probe_spin_kernel"
KERNELS = ("dd_jpegd_ffcount_kernel", "dd_jpegd_unstuff_kernel", "dd_jpegd_spec_kernel", "dd_jpegd_repair_kernel",
           "dd_jpegd_blocks_kernel", "dd_jpegd_emit_kernel", "dd_jpegd_dc_kernel", "dd_jpegd_idct_kernel",
           "dd_jpegd_colour_kernel")


def header_define(name):
    src = open(os.path.join(ROOT, "include", "dualdiff_hip.h")).read()
    return int(re.search(r"#define %s (\d+)" % name, src).group(1))


SUB_BITS, ROUNDS = header_define("DD_JPEG_SUB_BITS"), header_define("DD_JPEG_DECODE_ROUNDS")


def build_variants():
    from dualdiff_amd import _build
    os.makedirs(VARIANT_DIR, exist_ok=True)
    for s in VARIANTS:
        out = os.path.join(VARIANT_DIR, "libjpeg_decode_S%d.so" % s)
        cmd = [_build._hipcc(), "--offload-arch=" + _build.ARCH, "-O2", "-std=c++17", "-fPIC", "-DNDEBUG", "-shared",
               "-DDD_JD_SUB_BITS=%d" % s, os.path.join(_build.CSRC, "jpeg_decode.hip"), "-o", out]
        subprocess.run(cmd, check=True)
        print("built", out)


def make_files(quality):
    """-> (files, frames on the device): 6 frames of a bicubic low-frequency field with +-4 % noise, encoded on the GPU."""
    import torch
    from dualdiff_amd.pipeline.image_output import encode_jpeg
    g = torch.Generator().manual_seed(11)
    low = torch.rand((VIEWS, 3, 15, 25), generator=g).cuda()
    x = torch.nn.functional.interpolate(low, size=(H, W), mode="bicubic", align_corners=False)
    x = x + (torch.rand((VIEWS, 3, H, W), generator=g).cuda() - 0.5) * 0.08
    frames = (x.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return encode_jpeg(frames, quality), frames


def repaired(files, sub_bits, rounds):
    """Subsequences the repair pass decodes again, summed over the files, by the host program at S = sub_bits; None where
    no compiler is at hand."""
    from dualdiff_amd.pipeline import jpeg_input as JI
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        return None
    tmp = tempfile.mkdtemp(prefix="jpeg_input_timing_")
    try:
        exe = os.path.join(tmp, "host_check_S%d" % sub_bits)
        subprocess.run([cxx, "-std=c++17", "-O2", "-DDD_JD_SUB_BITS=%d" % sub_bits, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tools", "jpeg_decode_host_check.cpp"), "-o", exe], check=True)
        out = {}
        for r in rounds:
            cases = []
            for f in files:
                info = JI.parse_jpeg(f)
                scan = f[info.scan[0]:info.scan[1]]
                cases.append(struct.pack("<8i", info.h, info.w, info.sampling, r, len(scan), 0, 0, 0) + JI.table_block(info) + scan)
            path = os.path.join(tmp, "cases.bin")
            with open(path, "wb") as fh:
                fh.write(struct.pack("<2i", 0x43484444, len(cases)) + b"".join(cases))
            text = subprocess.run([exe, path], capture_output=True, text=True, check=True).stdout
            found = re.findall(r"(\d+) of (\d+) subsequences repaired", text)
            out[r] = (sum(int(a) for a, _ in found), sum(int(b) for _, b in found))
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


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
    if len(marks) != 2 * len(QUALITIES):
        raise SystemExit("expected %d sentinel launches in the trace, found %d" % (2 * len(QUALITIES), len(marks)))
    for i, q in enumerate(QUALITIES):
        win = rows[marks[2 * i] + 1:marks[2 * i + 1]]
        other = sorted({n for s, e, n in win if not any(k in n for k in KERNELS)})
        calls = sum(1 for s, e, n in win if KERNELS[0] in n)
        print("# quality %d: %d files of %d x %d; kernel time from the trace per launch, median over %d calls; other kernels: %s"
              % (q, VIEWS, H, W, calls, other or "none"))
        total = 0.0
        for k in KERNELS:
            t = [e - s for s, e, n in win if k in n]
            per_call = sum(t) / max(calls, 1) / 1e3
            total += per_call
            print("%-26s %4d launches (%g per call)  median %8.2f us  min %8.2f us  max %8.2f us  per call %8.2f us"
                  % (k, len(t), len(t) / max(calls, 1), statistics.median(t) / 1e3, min(t) / 1e3, max(t) / 1e3, per_call))
        print("%-26s kernel time per call (mean over the calls) %8.2f us" % ("the call's kernels", total))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=30, help="calls / runs per measurement (>= 25)")
    ap.add_argument("--build-variants", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarise", metavar="DIR_OR_KERNEL_TRACE_CSV")
    args = ap.parse_args()
    if args.build_variants:
        return build_variants()
    if args.summarise:
        return summarise(args.summarise)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("jpeg_input_timing: no GPU", file=sys.stderr)
        return 2
    if args.n < 25:
        ap.error("--n must be at least 25")
    from dualdiff_amd import _native, ops
    from dualdiff_amd.pipeline import jpeg_input as JI
    lib = _native.load()
    files = {q: make_files(q)[0] for q in QUALITIES}
    up = {q: JI.upload_jpeg(files[q], "cuda") for q in QUALITIES}
    for q in QUALITIES:                                                  # warm-up: workspace, code
        for _ in range(3):
            frames, status = ops.jpeg_decode_u8(*up[q])
        assert status.tolist() == [0] * VIEWS
    torch.cuda.synchronize()

    if args.trace:
        stamps = torch.zeros(2, dtype=torch.int64, device="cuda")

        def sentinel():
            torch.cuda.synchronize()
            _native.check(lib.dd_probe_spin(stamps.data_ptr(), 100, ops._stream()), "probe_spin")
            torch.cuda.synchronize()
        for q in QUALITIES:
            sentinel()
            for _ in range(args.n):
                ops.jpeg_decode_u8(*up[q], out=frames)
            sentinel()
        return 0

    def events(call):
        ts = []
        for _ in range(args.n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return statistics.median(ts), min(ts)

    sizes = {q: [len(f) for f in files[q]] for q in QUALITIES}
    print("# ops.jpeg_decode_u8, %d files of %d x %d, device events around one call on uploaded bytes, median (min) of %d in us;"
          % (VIEWS, H, W, args.n))
    print("# S = %d bits per subsequence, default rounds = %d; repaired: subsequences the repair pass decodes again, of all"
          % (SUB_BITS, ROUNDS))
    sweep = (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12)
    for q in QUALITIES:
        print("quality %d: files %s bytes (%.2f MB for %.2f MB of frames)" % (q, sizes[q], sum(sizes[q]) / 1e6, VIEWS * H * W * 3 / 1e6))
        rep = repaired(files[q], SUB_BITS, sweep)
        for r in sweep:
            med, lo = events(lambda: ops.jpeg_decode_u8(*up[q], rounds=r, out=frames))
            print("  S %5d rounds %d   %9.1f (%9.1f) us   repaired %s"
                  % (SUB_BITS, r, med, lo, "not counted (no compiler)" if rep is None else "%d of %d" % rep[r]))

    # the same call through the variant libraries
    for s in VARIANTS:
        path = os.path.join(VARIANT_DIR, "libjpeg_decode_S%d.so" % s)
        if not os.path.exists(path):
            print("S %d: %s is not built (--build-variants)" % (s, os.path.relpath(path, ROOT)))
            continue
        var = ctypes.CDLL(path)
        for name in ("dd_jpeg_decode_workspace_bytes", "dd_jpeg_decode_u8"):
            getattr(var, name).restype, getattr(var, name).argtypes = _native.SIGNATURES[name]
        for q in QUALITIES:
            scan, offsets, lengths, tables, h, w, sampling, longest = up[q]
            need = var.dd_jpeg_decode_workspace_bytes(VIEWS, h, w, sampling, longest)
            ws = torch.zeros((need + 3) // 4, dtype=torch.float32, device="cuda")
            status = torch.empty(VIEWS, dtype=torch.int32, device="cuda")
            out = torch.empty_like(frames)
            rep = repaired(files[q], s, VARIANT_ROUNDS)
            for r in VARIANT_ROUNDS:
                def call():
                    rc = var.dd_jpeg_decode_u8(scan.data_ptr(), scan.numel(), offsets.data_ptr(), lengths.data_ptr(), longest,
                                               tables.data_ptr(), VIEWS, h, w, sampling, out.data_ptr(), status.data_ptr(),
                                               ws.data_ptr(), ws.numel() * 4, r, ops._stream())
                    assert rc == 0, rc
                call()
                torch.cuda.synchronize()
                good = status.tolist() == [0] * VIEWS and torch.equal(out, ops.jpeg_decode_u8(*up[q])[0])
                med, lo = events(call)
                print("  quality %d S %5d rounds %d   %9.1f (%9.1f) us   repaired %s   frames %s"
                      % (q, s, r, med, lo, "not counted" if rep is None else "%d of %d" % rep[r],
                         "equal" if good else "DIFFER"))

    try:
        import PIL
        from PIL import Image
    except ImportError:
        PIL = None

    def host_path(fs):
        t0 = time.perf_counter()
        arr = np.stack([np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in fs])
        t1 = time.perf_counter()
        dev = torch.from_numpy(arr).cuda()
        torch.cuda.synchronize()
        return dev, t1 - t0, time.perf_counter() - t1

    med = lambda v: statistics.median(v) * 1e3                           # noqa: E731
    for q in QUALITIES:
        for _ in range(2):
            dev = JI.decode_jpeg(files[q])
            ref = host_path(files[q])[0] if PIL else None
        if ref is not None:
            print("# quality %d: frames that differ between the two paths: %d of %d"
                  % (q, sum(not torch.equal(a, b) for a, b in zip(dev, ref)), VIEWS))
        dev_t, walk_t, legs = [], [], []
        for _ in range(args.n):                                          # alternating, run by run
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            JI.decode_jpeg(files[q])
            dev_t.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            for i, f in enumerate(files[q]):
                JI.table_block(JI.parse_jpeg(f, frame=i))
            walk_t.append(time.perf_counter() - t0)
            if PIL:
                legs.append(host_path(files[q])[1:])
        print("# end to end, quality %d, %d files of %d x %d, wall clock in ms, median of %d runs" % (q, VIEWS, H, W, args.n))
        print("device  decode_jpeg: header walk, one pinned upload, one call, status read back   %8.2f ms" % med(dev_t))
        print("          of which the header walk and the table blocks, on the host              %8.2f ms" % med(walk_t))
        if PIL:
            print("host    PIL %s Image.open().convert(\"RGB\"), %d files, one thread               %8.2f ms"
                  % (PIL.__version__, VIEWS, med([l[0] for l in legs])))
            print("host    np.stack'ed frames .cuda()                                              %8.2f ms" % med([l[1] for l in legs]))
            print("host    total                                                                   %8.2f ms" % med([sum(l) for l in legs]))
        else:
            print("host    PIL Image.open: not measured (PIL is not installed here)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
