"""Attention-map pictures: what `AttnMapRender` costs, beside the host work it replaces.

    python tools/attn_output_timing.py [--n 20] [--reps 3]        # GPU -> stdout; profiles/attn_output.txt keeps a run
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ao -- python tools/attn_output_timing.py --trace
    python tools/attn_output_timing.py --summarise DIR            # the kernels' own durations, from the trace
    python tools/attn_output_timing.py --host [--loop-tiles 8]    # the host restatement, no GPU needed

Workload: one scene — 6 views, hw (28, 50), 106 context columns of softmax data, 79 text tiles (4 rows) and 28 box tiles
(1 row) per view at 224 x 400: 474 + 168 tiles, twelve sheets of 6 x (1087 x 8095) and 6 x (224 x 11308) pixels.
After a warm-up, per repetition:
  * events: `text_sheets` + `box_sheets` (six launches: dd_attn_heat, dd_image_resample_u8, dd_attn_sheet_u8, twice)
            between a pair of device events, median of N: device time plus the gaps the host leaves between launches;
  * call:   wall clock of `render(maps, n_text)` + `render.save(...)` into a temporary directory, i.e. with the PNG
            encode on the GPU, the copy of the files and the writes.
--trace: WARM + N calls of the six launches and nothing else, for a kernel trace; --summarise prints the median and the
minimum of each kernel's own duration, the text and the box launch apart.
--host: tests/attn_output_reference.py on this machine's CPU, one thread.  The per-pixel `cmap(...)` loop — the
reference's own cost — is timed on --loop-tiles tiles and scaled to the scene's 642; the rest (normalise, resize, strip,
view_images, PIL's PNG save) is timed on the whole scene with one `cmap` call per tile.
Timing is reported, not gated.  Exits non-zero when a GPU mode finds no GPU."""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VIEWS, HW, SIZE, N, N_TEXT, FIRST = 6, (28, 50), (224, 400), 106, 79, 78
KERNELS = ("dd_attn_heat_kernel", "dd_image_resample_kernel", "dd_attn_sheet_kernel")
WARM = 3


def scene():
    import numpy as np
    rng = np.random.RandomState(0)
    logits = rng.randn(VIEWS, HW[0] * HW[1], N) * 4
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def summarise(path, n):
    import csv
    import glob
    if os.path.isdir(path):
        found = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
        if not found:
            raise SystemExit("no *kernel_trace.csv under %s" % path)
        path = found[0]
    csv.field_size_limit(1 << 30)
    rows = {k: [] for k in KERNELS}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            for k in KERNELS:
                if k in r["Kernel_Name"]:
                    rows[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    print("# kernel durations from the trace, one scene (%d views, %d text + %d box tiles each); median / min of %d; us"
          % (VIEWS, N_TEXT, N - FIRST, n))
    total = 0.0
    for k in KERNELS:
        rows[k].sort()
        if len(rows[k]) != 2 * (WARM + n):
            raise SystemExit("expected %d launches of %s in the trace, found %d" % (2 * (WARM + n), k, len(rows[k])))
        timed = rows[k][2 * WARM:]
        for which, name in enumerate(("text", "box")):
            d = [(e - s) / 1e3 for s, e in timed[which::2]]
            total += statistics.median(d)
            print("%-4s %-26s median %8.2f  min %8.2f" % (name, k, statistics.median(d), min(d)))
    print("     %-26s        %8.2f" % ("sum of the six medians", total))


def host(loop_tiles):
    import numpy as np
    from PIL import Image
    from tests import attn_output_reference as R
    maps = scene()
    tiles = VIEWS * (N_TEXT + N - FIRST)
    R.colormap()
    t0 = time.perf_counter()
    for i in range(loop_tiles):
        R.colour_loop(R.normalise(maps[0, :, 1 + i], HW))
    loop = (time.perf_counter() - t0) / loop_tiles
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        for v in range(VIEWS):
            text = R.view_images(np.stack([R.with_strip(R.resized(R.colour(R.normalise(maps[v, :, i], HW)), SIZE))
                                           for i in range(1, N_TEXT + 1)]), num_rows=4)
            box = R.view_images(np.stack([R.resized(R.colour(R.normalise(maps[v, :, i], HW)), SIZE)
                                          for i in range(FIRST, N)]), num_rows=1)
            t1 = time.perf_counter()
            Image.fromarray(text).save(os.path.join(tmp, "view_images_%d.png" % v))
            Image.fromarray(box).save(os.path.join(tmp, "view_images_%dbox.png" % v))
            if v == 0:
                save = time.perf_counter() - t1
        rest = time.perf_counter() - t0
    print("# host restatement, one scene (%d tiles), one CPU thread; s" % tiles)
    print("per-pixel cmap loop: %.4f a tile over %d tiles timed -> %.1f for the scene's %d" % (loop, loop_tiles, loop * tiles, tiles))
    print("everything else (normalise, one cmap call a tile, resize, strip, view_images, PIL PNG save): %.2f, of which "
          "the PNG save %.2f (6 x the first view's %.3f)" % (rest, 6 * save, save))
    print("the reference's loop + the rest: %.1f" % (loop * tiles + rest))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20, help="calls per measurement")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarise", metavar="DIR_OR_KERNEL_TRACE_CSV")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--loop-tiles", type=int, default=8)
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.n)
    if args.host:
        return host(args.loop_tiles)
    import torch
    if not torch.cuda.is_available():
        print("attn_output_timing: no GPU", file=sys.stderr)
        return 2
    from dualdiff_amd.pipeline.attn_output import AttnMapRender
    med = statistics.median
    render = AttnMapRender(hw=HW, size=SIZE)
    maps = torch.from_numpy(scene()).cuda()

    def launches():
        return render.text_sheets(maps, N_TEXT), render.box_sheets(maps, first=FIRST)

    if args.trace:
        for _ in range(WARM + args.n):
            launches()
        torch.cuda.synchronize()
        return 0
    def row(what, v):
        print("    %-76s %s   spread %4.1f %%" % (what, "  ".join("%12.1f" % x for x in v), 100 * (max(v) - min(v)) / med(v)),
              flush=True)

    for _ in range(WARM):
        text, box = launches()
    torch.cuda.synchronize()
    print("# AttnMapRender, one scene: %d views, %d text + %d box tiles each; sheets %s and %s; %d repetitions; us"
          % (VIEWS, N_TEXT, N - FIRST, tuple(text.shape[1:3]), tuple(box.shape[1:3]), args.reps), flush=True)
    events = []
    for _ in range(args.reps):
        ts = []
        for _ in range(args.n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launches()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        events.append(med(ts))
    row("device events around text_sheets + box_sheets, 6 launches (median of %d)" % args.n, events)
    del text, box
    with tempfile.TemporaryDirectory() as tmp:
        def call():
            text, box = render(maps, N_TEXT)
            return render.save(tmp, text, box)

        paths = call()
        sizes = sum(os.path.getsize(p) for p in paths)
        calls, k = [], max(3, args.n // 5)
        for _ in range(args.reps):
            ts = []
            for _ in range(k):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                ts.append((time.perf_counter() - t0) * 1e6)
            calls.append(med(ts))
    row("render(maps, n_text) + render.save(...): %d files, %.1f MB, wall (median of %d)" % (len(paths), sizes / 1e6, k), calls)
    return 0


if __name__ == "__main__":
    sys.exit(main())
