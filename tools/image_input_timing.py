"""Image input: what the first step of the given-view path costs on the GPU, against the host transform it replaces.

    python tools/image_input_timing.py                        # device-event / wall-clock medians -> stdout
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ii -- python tools/image_input_timing.py --trace
    python tools/image_input_timing.py --summarise DIR        # kernel time per configuration and its share of the bound

Production sizes only: 6 camera frames of 900 x 1600 x 3 bytes, the reference's four configurations (dataset.image_size,
dataset.augment2d.resize), fp32 NCHW `pixel_values` out — and the bf16 channels-last form encode_images launches.

Default run, after a warm-up of every shape:
  * per configuration `ops.image_load_u8` between a pair of device events, median of N >= 25 launches;
  * end to end per configuration, host frames -> `pixel_values` on the device, alternating run by run:
      host  PIL resize + crop, ToTensor, Normalize per view (one CPU thread), stack, one copy to the device
      gpu   one copy of the uint8 frames to the device, then the kernel
    wall clock around work that ends in a device synchronise, median of N, and the number of elements in which the two
    results differ; the host leg runs only where PIL is installed, and is reported as "not measured" otherwise.

--trace: per configuration N launches between two launches of the one-wave dd_probe_spin kernel; --summarise splits the
kernel trace at those sentinels and prints the median kernel time of dd_image_load_kernel, the bytes it has to move (read:
6 x 900 x 1600 x 3; written: 6 x 3 x fH x fW x 4, or 6 x fH x fW x 8 x 2) and the time those take at the HBM peak
(8 TB/s) and at the achievable streaming rate (6.3 TB/s).  Exits non-zero when there is no GPU."""
import argparse
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VIEWS = 6
ORI = (900, 1600)
# dataset.image_size, dataset.augment2d.resize[0]: configs/dataset/Nuscenes*.yaml
CONFIGS = [((224, 400), (0.25, 0.25)), ((256, 704), (0.48, 0.48)), ((432, 768), (0.48, 0.48)), ((192, 384), (0.24, 0.24))]
FORMS = [("fp32 nchw", "float32", "nchw"), ("bf16 nhwc8", "bfloat16", "nhwc8")]
SENTINEL = "dd_probe_spin_kernel"
KERNEL = "dd_image_load_kernel"
HBM_PEAK, HBM_STREAM = 8.0e12, 6.3e12


def pre_of(c):
    from dualdiff_amd.pipeline.image_input import ImagePreProcess
    return ImagePreProcess.from_config({"dataset": {"image_size": c[0], "augment2d": {"resize": [c[1]]}}}, ORI)


def cfg_name(c, pre):
    return "900x1600 -> %dx%d box %s -> %dx%d" % (pre.resize + (list(pre.box),) + tuple(c[0]))


def bytes_moved(c, form):
    fh, fw = c[0]
    return VIEWS * ORI[0] * ORI[1] * 3, (VIEWS * 3 * fh * fw * 4 if form[2] == "nchw" else VIEWS * fh * fw * 8 * 2)


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
    n = len(CONFIGS) * len(FORMS)
    if len(marks) != 2 * n:
        raise SystemExit("expected %d sentinel launches in the trace, found %d" % (2 * n, len(marks)))
    print("# %s, %d frames of 900 x 1600: kernel time from the trace (median of the launches between the sentinels)" % (KERNEL, VIEWS))
    i = 0
    for c in CONFIGS:
        pre = pre_of(c)
        for form in FORMS:
            win = [e - s for s, e, k in rows[marks[2 * i] + 1:marks[2 * i + 1]] if KERNEL in k]
            other = [k for s, e, k in rows[marks[2 * i] + 1:marks[2 * i + 1]] if KERNEL not in k]
            i += 1
            rd, wr = bytes_moved(c, form)
            med = statistics.median(win) / 1e3
            print("%-52s %-10s %3d launches (%d other kernels)  median %7.2f us  min %7.2f us   read %5.2f MB + written %5.2f MB"
                  "   bound %5.2f us at 8 TB/s (%4.1f %% of it), %5.2f us at 6.3 TB/s (%4.1f %%)"
                  % (cfg_name(c, pre), form[0], len(win), len(other), med, min(win) / 1e3, rd / 1e6, wr / 1e6,
                     (rd + wr) / HBM_PEAK * 1e6, 100 * (rd + wr) / HBM_PEAK * 1e6 / med, (rd + wr) / HBM_STREAM * 1e6,
                     100 * (rd + wr) / HBM_STREAM * 1e6 / med))


def host_path(frames, pre, Image):
    """Today's path: the dataset transform per view on the host, then one copy -> pixel_values on the device."""
    import numpy as np
    import torch
    mean = torch.as_tensor(pre.mean, dtype=torch.float32).view(-1, 1, 1)
    std = torch.as_tensor(pre.std, dtype=torch.float32).view(-1, 1, 1)
    views = []
    for a in frames:
        img = Image.fromarray(a).resize((pre.resize[1], pre.resize[0])).crop(pre.box)            # ImageAug3D
        x = torch.from_numpy(np.array(img, copy=True)).permute((2, 0, 1)).contiguous().to(dtype=torch.float32).div(255)
        views.append(x.sub_(mean).div_(std))                                                      # ToTensor, Normalize
    out = torch.stack(views).float().cuda()                                                       # collate_fn, the copy
    torch.cuda.synchronize()
    return out


def gpu_path(frames, pre):
    import torch
    out = pre(torch.from_numpy(frames).cuda())
    torch.cuda.synchronize()
    return out


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
        print("image_input_timing: no GPU", file=sys.stderr)
        return 2
    if args.n < 25:
        ap.error("--n must be at least 25")
    import numpy as np
    from dualdiff_amd import _native, ops
    torch.set_num_threads(1)
    rng = np.random.RandomState(1)
    host = rng.randint(0, 256, size=(VIEWS,) + ORI + (3,)).astype(np.uint8)
    frames = torch.from_numpy(host).cuda()
    pres = {c: pre_of(c) for c in CONFIGS}
    outs = {}

    def launch(c, form, out=None):
        p = pres[c]
        return ops.image_load_u8(frames, p.resize, p.box, p.mean, p.std, getattr(torch, form[1]), form[2], out=out)
    for c in CONFIGS:                                                    # warm-up: builds the device tables, loads the code
        for form in FORMS:
            for _ in range(3):
                outs[c, form] = launch(c, form)
    torch.cuda.synchronize()

    if args.trace:
        lib = _native.load()
        stamps = torch.zeros(2, dtype=torch.int64, device="cuda")

        def sentinel():
            torch.cuda.synchronize()
            _native.check(lib.dd_probe_spin(stamps.data_ptr(), 100, ops._stream()), "probe_spin")
            torch.cuda.synchronize()
        for c in CONFIGS:
            for form in FORMS:
                sentinel()
                for _ in range(args.n):
                    launch(c, form, outs[c, form])
                sentinel()
        return 0

    print("# ops.image_load_u8, %d frames of 900 x 1600, device events around one launch, median of %d" % (VIEWS, args.n))
    for c in CONFIGS:
        for form in FORMS:
            ts = []
            for _ in range(args.n):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch(c, form, outs[c, form])
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            rd, wr = bytes_moved(c, form)
            print("%-52s %-10s median %7.1f us  min %7.1f us  (read %5.2f MB, written %5.2f MB; %5.2f us at 8 TB/s)"
                  % (cfg_name(c, pres[c]), form[0], statistics.median(ts), min(ts), rd / 1e6, wr / 1e6,
                     (rd + wr) / HBM_PEAK * 1e6))

    try:
        import PIL
        from PIL import Image
    except ImportError:
        PIL = Image = None
    med = lambda v: statistics.median(v) * 1e3                           # noqa: E731
    print("# end to end, host frames -> fp32 pixel_values on the device, %d views, wall clock in ms, median of %d runs%s"
          % (VIEWS, args.n, "" if PIL is None else " (PIL %s, one CPU thread)" % PIL.__version__))
    for c in CONFIGS:
        pre = pres[c]
        diff = None
        for _ in range(2):
            got = gpu_path(host, pre)
            if Image is not None:
                diff = int((host_path(host, pre, Image) != got).sum())
        gpu_t, host_t = [], []
        for _ in range(args.n):                                          # alternating, run by run
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gpu_path(host, pre)
            gpu_t.append(time.perf_counter() - t0)
            if Image is not None:
                t0 = time.perf_counter()
                host_path(host, pre, Image)
                host_t.append(time.perf_counter() - t0)
        print("%-52s gpu  copy of the uint8 frames + kernel %8.2f ms   host  PIL resize + crop + ToTensor + Normalize + copy %s"
              "   differing elements: %s" % (cfg_name(c, pre), med(gpu_t),
                                             "%8.2f ms" % med(host_t) if host_t else "not measured (PIL is not installed here)",
                                             "not measured" if diff is None else "%d of %d" % (diff, got.numel())))
    return 0


if __name__ == "__main__":
    sys.exit(main())
