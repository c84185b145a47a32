"""numpy restatement of the reference's `visualize_map` (runner/map_visualizer.py:143-211), vectorised: the colouring of
the static and dynamic layers, the classes in use, PIL's bicubic resize (tests/pil_resample_reference.py), the quarter
turn and the legend paste.  Written from the behaviour pinned by tests/golden/map_output.npz, independent of
dualdiff_amd; it reads nothing but its arguments.

`fault` plants one deliberate mistake (FAULTS): tests/test_map_output_cpu.py shows that the fixture catches each."""
import numpy as np

from tests import pil_resample_reference as PR

NOTHING = "nothing"
FAULTS = ("swap_priorities", "last_dynamic", "static_over_dynamic", "turn_other_way", "turn_before_resize",
          "legend_wrong_side", "dynamic_used_from_set_pixels")


def target_side(s, target_size):
    ratio = max(target_size / s, target_size / s)
    return int(s * ratio)


def colour(maps, map_classes, object_classes, colors, priority, fault=None, swap=None):
    """maps (C, S, S) of 0 / 1 -> (rendered (S, S, 3) uint8, used: set of class names).  swap: with fault
    "swap_priorities", the two class names whose priority entries trade places."""
    maps = np.asarray(maps) != 0
    c, s = maps.shape[0], maps.shape[1]
    mc = [] if map_classes is None else list(map_classes)
    oc = [] if object_classes is None else list(object_classes)
    priority = list(priority)
    if fault == "swap_priorities":
        i, j = priority.index(swap[0]), priority.index(swap[1])
        priority[i], priority[j] = priority[j], priority[i]
    static = maps[:len(mc)]
    dynamic = maps[len(mc):len(mc) + len(oc)]
    used = set()
    out = np.empty((s, s, 3), dtype=np.uint8)
    out[:] = np.asarray(colors[NOTHING], dtype=np.uint8)
    any_static = np.zeros((s, s), dtype=bool)
    static_rgb = np.zeros((s, s, 3), dtype=np.uint8)
    if len(mc):
        best = np.full((s, s), -1, dtype=np.int64)
        for k in range(static.shape[0]):
            if static[k].any():
                used.add(mc[k])
            rank = priority.index(mc[k])
            take = static[k] & (rank > best)
            best[take] = rank
            static_rgb[take] = np.asarray(colors[mc[k]], dtype=np.uint8)
        any_static = best >= 0
    any_dynamic = np.zeros((s, s), dtype=bool)
    dynamic_rgb = np.zeros((s, s, 3), dtype=np.uint8)
    if len(oc) and dynamic.shape[0] > 0:
        nd = dynamic.shape[0]
        any_dynamic = dynamic.any(axis=0)
        if fault == "last_dynamic":
            arg = nd - 1 - dynamic[::-1].argmax(axis=0)
            arg[~any_dynamic] = 0
        else:
            arg = dynamic.argmax(axis=0)                              # the first set layer; 0 where none is set
        seen = arg[any_dynamic] if fault == "dynamic_used_from_set_pixels" else arg
        used |= {oc[j] for j in np.unique(seen).tolist()}
        table = np.asarray([colors[n] for n in oc[:nd]], dtype=np.uint8)
        dynamic_rgb = table[arg]
    if fault == "static_over_dynamic":
        out[any_dynamic] = dynamic_rgb[any_dynamic]
        out[any_static] = static_rgb[any_static]
    else:
        out[any_static] = static_rgb[any_static]
        out[any_dynamic] = dynamic_rgb[any_dynamic]
    return out, used


def turn(x, fault=None):
    return np.rot90(x, -1 if fault == "turn_other_way" else 1)


def render(maps, map_classes, object_classes, colors, priority, target_size=400, fault=None, swap=None):
    """-> (frame (T, T, 3) uint8: the picture before the legend, used: set of names)."""
    rendered, used = colour(maps, map_classes, object_classes, colors, priority, fault, swap)
    t = target_side(rendered.shape[0], target_size)
    if fault == "turn_before_resize":
        frame = PR.resize(np.ascontiguousarray(turn(rendered)), (t, t))
    else:
        frame = turn(PR.resize(rendered, (t, t)), fault)
    return np.ascontiguousarray(frame), used


def compose(frame, legend, fault=None):
    """np.pad with zeros and the legend: to the right where it is taller than wide, below otherwise (:200-211)."""
    h, w, _ = frame.shape
    lh, lw, _ = legend.shape
    right = lh > lw
    if fault == "legend_wrong_side":
        right = not right
    if right:
        out = np.zeros((h, w + lw, 3), dtype=np.uint8)
        out[:, :w] = frame
        out[:lh, w:] = legend[:h]
    else:
        out = np.zeros((h + lh, w, 3), dtype=np.uint8)
        out[:h] = frame
        out[h:, :lw] = legend[:, :w]
    return out


def used_word(used, map_classes, object_classes):
    every = ([] if map_classes is None else list(map_classes)) + ([] if object_classes is None else list(object_classes))
    return sum(1 << k for k, n in enumerate(every) if n in used)
