"""Map input (`BevMapInput`, dd_bev_box_records + dd_bev_map_layers): what it costs on the GPU, against the host path.

    python tools/map_input_timing.py                       # device-event / wall-clock medians -> stdout
    python tools/map_input_timing.py --host                # the host path only (no GPU needed)
    rocprofv3 --kernel-trace --output-format csv -d DIR -o map -- python tools/map_input_timing.py --trace
    python tools/map_input_timing.py --summarise DIR       # the kernels' own durations out of that run

One scene of 40 boxes and one of 300 at the reference's 200 x 200 canvas, 8 static + 10 object layers and all eight aux
channels (tests/map_input_reference.py: random_scene, seeded).  Per scene, after a comparison with the restatement:
  * `ops.bev_map_layers` (both launches) from device tensors, workspace and outputs allocated once, between a pair of
    device events, median of N, three rounds;
  * the whole `BevMapInput.__call__` from host lists (pack, one upload, two launches, the 4-byte flags readback of
    check=True; and with check=False followed by a device synchronise), wall clock, median of N;
  * the host path: the reference's lines restated with numpy + PIL itself (`ImageDraw.polygon` per box and class, a fresh
    image and the aux writes per box, the meshgrid per box as the reference builds it), one thread, plus the upload of its
    two results, wall clock, median of N (--host runs this alone).
--trace: N calls of `ops.bev_map_layers` per scene and nothing else, for a profiler run of its own."""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import map_input_reference as R  # noqa: E402

BOUND = (-50.0, 50.0, 0.5)
AUX = ("visibility", "center_offset", "center_ohw", "height")
COUNTS = (40, 300)


def scene(n):
    rng = np.random.default_rng(500 + n)
    sc = R.random_scene(rng, n, 10, BOUND, BOUND, spread=1.0)
    static = rng.integers(0, 2, (8, 200, 200)).astype(np.uint8)
    return static, sc


def host_path(static, sc, l2c, size=200):
    """pipeline.py:88-217 with numpy + PIL, as the reference runs it"""
    from PIL import Image, ImageDraw
    dyn = np.zeros((10, size, size), np.uint8)
    for c in range(10):
        idx = np.nonzero(sc["labels"] == c)[0]
        if len(idx) < 1:
            continue
        quads = R.to_canvas(sc["corners"][idx][:, list(R.BOTTOM), :2], l2c)
        render = Image.fromarray(dyn[c])
        draw = ImageDraw.Draw(render)
        for q in quads:
            draw.polygon(q.round().astype(np.int32).flatten().tolist(), fill=1)
        dyn[c, :] = np.array(render)[:]
    masks = np.concatenate([static, dyn.transpose(0, 2, 1)], axis=0)
    aux = np.zeros((size, size, 8), np.float32)
    for i in range(len(sc["labels"])):
        vis, cen, hh, ww, v, bh = R.box_aux_values(sc["corners"][i], sc["bottom_center"][i], sc["height"][i],
                                                   sc["visibility"][i], l2c)
        render = Image.fromarray(np.zeros((size, size), np.uint8))
        ImageDraw.Draw(render).polygon(R.quad_of(sc["corners"][i], l2c).flatten().tolist(), fill=1)
        mask = np.array(render) > 0
        coords = np.stack(np.meshgrid(np.arange(size), np.arange(size)), -1).astype(np.float32)
        aux[mask, 0:1] = vis
        aux[mask, 1:3] = coords[mask] - cen[None]
        aux[mask, 3:7] = np.array([hh, ww, v[0], v[1]])[None]
        aux[mask, 7:8] = np.array([float(bh)])[None]
    return masks, aux.transpose(2, 1, 0)


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
            rows += [r for r in csv.DictReader(f) if "dd_bev_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for name in ("dd_bev_box_records_kernel", "dd_bev_map_layers_kernel"):
        mine = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
        half = len(mine) // 2
        for label, part in (("40 boxes", mine[:half]), ("300 boxes", mine[half:])):
            part = part[len(part) // 4:]                                   # the warm launches
            print("%s, %s: last %d launches median %.2f us, min %.2f, max %.2f"
                  % (name, label, len(part), statistics.median(part), min(part), max(part)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarise")
    ap.add_argument("-n", type=int, default=30)
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    (_, _), l2c = R.canvas_of(BOUND, BOUND)
    if args.host:
        for n in COUNTS:
            static, sc = scene(n)
            med, low = median_ms(lambda: host_path(static, sc, l2c), max(3, args.n // 3))
            print("host    %3d boxes: numpy + PIL, one thread, median %.2f ms (min %.2f)" % (n, med, low))
        return
    import torch
    from dualdiff_amd import ops
    from dualdiff_amd.pipeline.map_input import BevMapInput
    if not torch.cuda.is_available():
        sys.exit("no GPU")
    if not args.trace:
        print("# %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    mi = BevMapInput(BOUND, BOUND, 8, 10, AUX)
    for n in COUNTS:
        static, sc = scene(n)
        st = torch.from_numpy(static)[None].cuda()
        dev = {k: torch.from_numpy(v).cuda() for k, v in sc.items()}
        dev["visibility"] = dev["visibility"].float()
        off = torch.tensor([0, n], dtype=torch.int32, device="cuda")
        ws = torch.empty((ops.bev_map_workspace_bytes(n),), dtype=torch.uint8, device="cuda")
        out = (torch.empty((1, 18, 200, 200), dtype=torch.uint8, device="cuda"),
               torch.empty((1, 8, 200, 200), dtype=torch.float32, device="cuda"), torch.empty((1,), dtype=torch.int32, device="cuda"))

        def launch():
            return ops.bev_map_layers(st, dev["corners"], dev["bottom_center"], dev["height"], dev["visibility"],
                                      dev["labels"], off, 200, 8, 10, 15, mi.l2c, workspace=ws, out=out)
        for _ in range(args.n // 3 + 1):
            launch()
        torch.cuda.synchronize()
        if args.trace:
            for _ in range(args.n):
                launch()
            torch.cuda.synchronize()
            continue
        ref_m, ref_a = host_path(static, sc, l2c)
        same = torch.equal(out[0][0].cpu(), torch.from_numpy(ref_m)) and torch.equal(out[1][0].cpu(), torch.from_numpy(ref_a.copy()))
        covered = int((ref_a[0] != 0).sum())
        print("%3d boxes: equal to the numpy + PIL host path: %s; %d of 40000 pixels under a box; flags %d"
              % (n, same, covered, int(out[2].item())))
        rounds = []
        for _ in range(3):
            ts = []
            for _ in range(args.n):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                launch()
                b.record()
                b.synchronize()
                ts.append(a.elapsed_time(b) * 1e3)
            rounds.append(ts)
        print("     both launches, device events, median of %d (3 rounds)  %s us   (min %.1f)"
              % (args.n, " / ".join("%.1f" % statistics.median(t) for t in rounds), min(min(t) for t in rounds)))
        host = {k: [torch.from_numpy(v)] for k, v in sc.items()}

        def whole(check):
            o = mi(st, host["corners"], host["labels"], bottom_center=host["bottom_center"], height=host["height"],
                   visibility=host["visibility"], check=check)
            if not check:
                torch.cuda.synchronize()
            return o
        for check in (True, False):
            whole(check)
            med, low = median_ms(lambda: whole(check), args.n)
            print("     BevMapInput.__call__ from host lists, check=%s, wall clock, median of %d   %.3f ms (min %.3f)"
                  % (check, args.n, med, low))

        def host_whole():
            m, a = host_path(static, sc, l2c)
            torch.from_numpy(m).cuda(), torch.from_numpy(np.ascontiguousarray(a)).cuda()
            torch.cuda.synchronize()
        med, low = median_ms(host_whole, max(3, args.n // 3))
        print("     host path: numpy + PIL, one thread, + upload, wall clock, median of %d   %.2f ms (min %.2f)"
              % (max(3, args.n // 3), med, low))


if __name__ == "__main__":
    main()
