"""Mints tests/golden/map_output.npz from the reference's own `visualize_map` (runner/map_visualizer.py), so that the map
output tests pin the reference's pictures where neither the reference nor matplotlib is installed.  Needs the reference's
file, matplotlib and Pillow:

    python -m tests.golden.mint_map_output <path to magicdrive/runner/map_visualizer.py>

The module is loaded by path with matplotlib on the Agg backend; a namespace stands in for `cfg`; `show_legend` is wrapped
so that every legend it draws is kept with the class set it was given.

Stored per case `<n>` of CASES: `in_<n>` (np.packbits of the (C, S, S) 0 / 1 map), `out_<n>` (the whole picture),
`legend_<n>` (the legend the reference drew) and `used_<n>` (the names handed to `show_legend`, sorted, joined by commas).
Once: `color_names` / `color_values` (the reference's COLORS in its order), `static_priority`, `pil_version`,
`matplotlib_version`.  The class lists, sizes and inputs are code here (CASES, `inputs`), shared with the tests."""
import os
import sys

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "map_output.npz")

# configs/dataset/Nuscenes.yaml:63-85
OBJECT_CLASSES = ("car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
                  "traffic_cone")
MAP_CLASSES = ("drivable_area", "ped_crossing", "walkway", "stop_line", "carpark_area", "road_divider", "lane_divider",
               "road_block")
# MAP_CLASSES by rising priority (their indices in the reference's STATIC_PRIORITY: 0, 2, 3, 4, 5, 6, 8, 9)
BY_PRIORITY = ("drivable_area", "road_block", "walkway", "stop_line", "carpark_area", "ped_crossing", "road_divider",
               "lane_divider")

# name -> (S, target_size, C, map_classes, object_classes)
CASES = {
    "pairs": (12, 40, 8, MAP_CLASSES, OBJECT_CLASSES),          # what collate_fn produces today: no dynamic part
    "few_dynamic": (12, 40, 12, MAP_CLASSES, OBJECT_CLASSES),
    "mixed": (20, 50, 18, MAP_CLASSES, OBJECT_CLASSES),         # ratio 2.5
    "aux": (12, 40, 26, MAP_CLASSES, OBJECT_CLASSES),           # 7 aux layers + 1 that nothing reads
    "empty": (12, 40, 18, MAP_CLASSES, OBJECT_CLASSES),         # the legend of {'car'}
    "static_only": (12, 40, 8, MAP_CLASSES, None),
    "dynamic_only": (12, 40, 10, None, OBJECT_CLASSES),
    "full": (200, 400, 18, MAP_CLASSES, OBJECT_CLASSES),
}


def _rect(m, k, y0, y1, x0, x1):
    m[k, y0:y1, x0:x1] = 1


def inputs(name):
    """The (C, S, S) uint8 map of a case, 0 / 1."""
    s, _, c, mc, oc = CASES[name]
    m = np.zeros((c, s, s), dtype=np.uint8)
    ns = 0 if mc is None else len(mc)
    if name in ("pairs", "static_only"):
        # row r < 7: the r-th pair of neighbouring priorities together on columns 2..9, each of the two alone on column
        # 0 / 1 and 10 / 11; rows 7..11: a three-layer overlap, and pixels with nothing
        for r in range(7):
            a, b = mc.index(BY_PRIORITY[r]), mc.index(BY_PRIORITY[r + 1])
            _rect(m, a, r, r + 1, 0, 10)
            _rect(m, b, r, r + 1, 2, 12)
        _rect(m, mc.index("drivable_area"), 8, 11, 1, 9)
        _rect(m, mc.index("lane_divider"), 9, 10, 0, 12)
        _rect(m, mc.index("walkway"), 8, 12, 4, 6)
    elif name == "few_dynamic":
        _rect(m, 0, 0, 12, 0, 9)
        _rect(m, 7, 2, 5, 3, 12)
        _rect(m, ns + 1, 1, 4, 1, 5)                             # truck over both, and over nothing at column 9..
        _rect(m, ns + 3, 3, 7, 4, 11)                            # bus overlaps truck: the first set layer wins
        _rect(m, ns + 2, 9, 11, 8, 12)                           # car (layer ns) is set nowhere: still in the legend
    elif name == "mixed":
        rs = np.random.RandomState(2050)
        for k in range(ns):
            y, x = rs.randint(0, 14, 2)
            _rect(m, k, y, y + rs.randint(2, 9), x, x + rs.randint(2, 9))
        for j in (1, 4, 5, 8, 9):                                # no car; overlapping objects
            y, x = rs.randint(0, 16, 2)
            _rect(m, ns + j, y, y + rs.randint(2, 6), x, x + rs.randint(2, 6))
        _rect(m, ns + 6, 5, 9, 5, 9)
        _rect(m, ns + 2, 7, 12, 7, 12)
    elif name == "aux":
        _rect(m, 1, 0, 6, 0, 6)
        _rect(m, 5, 3, 4, 0, 12)
        _rect(m, ns + 0, 4, 8, 4, 8)                             # car set, everywhere else argmax is car too
        _rect(m, ns + 9, 6, 10, 6, 10)
        m[18:] = np.random.RandomState(26).randint(0, 2, (8, s, s))      # the aux layers: ignored
    elif name == "dynamic_only":
        _rect(m, 3, 1, 6, 2, 8)
        _rect(m, 8, 4, 9, 5, 11)
        _rect(m, 9, 10, 12, 0, 3)
    elif name == "full":
        rs = np.random.RandomState(200400)
        _rect(m, 0, 20, 180, 30, 170)
        for k in range(1, ns):
            for _ in range(3):
                y, x = rs.randint(0, 170, 2)
                _rect(m, k, y, y + rs.randint(3, 40), x, x + rs.randint(3, 40))
        for j in range(1, 10):
            for _ in range(2):
                y, x = rs.randint(0, 185, 2)
                _rect(m, ns + j, y, y + rs.randint(4, 14), x, x + rs.randint(4, 14))
    return m


def load():
    return np.load(PATH)


def colors(z):
    return {str(n): tuple(int(v) for v in rgb) for n, rgb in zip(z["color_names"], z["color_values"])}


def priority(z):
    return [str(n) for n in z["static_priority"]]


def used(z, name):
    s = str(z["used_" + name])
    return set(s.split(",")) if s else set()


def main(path):
    import importlib.util
    import types
    import matplotlib
    matplotlib.use("Agg")
    import PIL
    spec = importlib.util.spec_from_file_location("reference_map_visualizer", path)
    mv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mv)
    drawn = []
    real = mv.show_legend

    def show_legend(semantic_in_use, long_edge_size=200, ncol=4):
        im = real(semantic_in_use, long_edge_size=long_edge_size, ncol=ncol)
        drawn.append((set(str(n) for n in semantic_in_use), im))
        return im
    mv.show_legend = show_legend
    out = {"pil_version": np.array(PIL.__version__), "matplotlib_version": np.array(matplotlib.__version__),
           "color_names": np.array(list(mv.COLORS)), "color_values": np.array(list(mv.COLORS.values()), dtype=np.uint8),
           "static_priority": np.array(mv.STATIC_PRIORITY)}
    for name, (s, target, c, mc, oc) in CASES.items():
        m = inputs(name)
        assert m.shape == (c, s, s) and m.max() <= 1
        cfg = types.SimpleNamespace(dataset=types.SimpleNamespace(map_classes=None if mc is None else list(mc),
                                                                  object_classes=None if oc is None else list(oc)))
        del drawn[:]
        pic = mv.visualize_map(cfg, m.astype(np.float32), target_size=target)
        (names, legend), = drawn
        out["in_" + name] = np.packbits(m)
        out["out_" + name] = pic
        out["legend_" + name] = legend
        out["used_" + name] = np.array(",".join(sorted(names)))
        print("%-13s %s -> %s, legend %s of %s" % (name, m.shape, pic.shape, legend.shape, sorted(names)))
    np.savez_compressed(PATH, **out)
    size = os.path.getsize(PATH)
    assert size < 300 * 1000, size
    print("wrote %s (PIL %s, matplotlib %s, %d bytes)" % (PATH, PIL.__version__, matplotlib.__version__, size))


if __name__ == "__main__":
    main(sys.argv[1])
