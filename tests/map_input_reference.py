"""CPU restatement of the BEV map input — TEST INFRASTRUCTURE ONLY, independent of the kernels.

Restates, in numpy, `LoadBEVSegmentationM` of magicdrive/dataset/pipeline.py: `_project_dynamic_bbox` (:176-200) and
`_project_dynamic` (:202-217) for the object layers, `_get_dynamic_aux_bbox` (:88-152) and `_get_dynamic_aux`
(:154-174) for the aux channels, `one_hot_decode` / `one_hot_encode` of dataset/pipeline_utils.py and the
`bev_map_with_aux` lines of `collate_fn` (dataset/utils.py:341-345).  PIL is NOT imported here: `polygon_fill` restates
`ImageDraw.polygon(xy, fill=1)` (Pillow's `ImagingDrawPolygon` + `polygon_generic` of Draw.c, 8-bit image, no
outline) in float32 arithmetic, and tests/test_map_input_cpu.py compares it with the installed Pillow pixel for pixel.
PINNED: tests/golden/mint_map_input.py executes the reference's own lines and the CPU test compares this file with them.
"""
import math

import numpy as np

AUX_DATA_CH = (("visibility", 1), ("center_offset", 2), ("center_ohw", 4), ("height", 1))   # pipeline.py:43-48, fixed order
BOTTOM = (0, 3, 7, 4)                                                                    # :100, :187
F32 = np.float32


# ------------------------------------------------------------------------------------------------------- PIL's polygon

def _round_up(f):
    """Draw.c ROUND_UP: half away from zero"""
    f = float(f)
    return int(math.floor(F32(f) + F32(0.5))) if f >= 0 else -int(math.floor(F32(abs(f)) + F32(0.5)))


def _round_down(f):
    """Draw.c ROUND_DOWN: half toward zero"""
    f = float(f)
    return int(math.ceil(F32(f) - F32(0.5))) if f >= 0 else -int(math.ceil(F32(abs(f)) - F32(0.5)))


def _lround(f):
    """C's lroundf: half away from zero"""
    f = float(f)
    return int(math.floor(f + 0.5)) if f >= 0 else -int(math.floor(-f + 0.5))


class _Edge:
    __slots__ = ("x0", "y0", "xmin", "xmax", "ymin", "ymax", "dx")

    def __init__(self, x0, y0, x1, y1):
        self.x0, self.y0 = x0, y0
        self.xmin, self.xmax = min(x0, x1), max(x0, x1)
        self.ymin, self.ymax = min(y0, y1), max(y0, y1)
        self.dx = F32(0) if y0 == y1 else F32(x1 - x0) / F32(y1 - y0)

    def at(self, y):
        """(y - y0) * dx + x0, two float32 roundings (no contraction)"""
        return F32(F32(F32(y - self.y0) * self.dx) + F32(self.x0))


def polygon_edges(pts):
    """ImagingDrawPolygon's edge list for the ring `pts` ((x, y) ints): consecutive points, a horizontal edge that
    continues the previous horizontal edge in the same direction widens that one, and the closing edge only where the
    last point is not the first."""
    n = len(pts)
    edges = []
    for i in range(n - 1):
        (x0, y0), (x1, y1) = pts[i], pts[i + 1]
        if y0 == y1 and i != 0 and y0 == pts[i - 1][1]:
            if x1 > x0 > pts[i - 1][0]:
                edges[-1].xmax = x1
                continue
            if x1 < x0 < pts[i - 1][0]:
                edges[-1].xmin = x1
                continue
        edges.append(_Edge(x0, y0, x1, y1))
    if tuple(pts[-1]) != tuple(pts[0]):
        edges.append(_Edge(pts[-1][0], pts[-1][1], pts[0][0], pts[0][1]))
    return edges


def polygon_spans(pts, size):
    """The hline calls of polygon_generic, in order and unclipped in x: a list of (y, x_start, x_end).  `size` is the
    image's height (the scan range is clipped to [0, size], as Draw.c does)."""
    edges = polygon_edges([(int(x), int(y)) for x, y in pts])
    spans = []
    ymin, ymax = size - 1, 0
    table = []
    for e in edges:
        ymin, ymax = min(ymin, e.ymin), max(ymax, e.ymax)
        if e.ymin == e.ymax:
            spans.append((e.ymin, e.xmin, e.xmax))
            continue
        table.append(e)
    ymin, ymax = max(ymin, 0), min(ymax, size)
    for y in range(ymin, ymax + 1):
        xx = []
        for i, cur in enumerate(table):
            if not cur.ymin <= y <= cur.ymax:
                continue
            xx.append(cur.at(y))
            if y == cur.ymax and y < ymax:
                xx.append(xx[-1])
            elif cur.dx != 0 and F32(np.round(xx[-1])) == xx[-1]:
                # "connect discontiguous corners": an earlier edge of the same strict slope sign that STARTS with this
                # one on this row, or ENDS with it, at the same x.  The span then reaches to the pixel next to the one
                # that the adjacent row rounds to (half away from zero), never short of the corner itself.
                x = xx[-1]
                for k in range(i):
                    oth = table[k]
                    if (cur.dx > 0 and oth.dx <= 0) or (cur.dx < 0 and oth.dx >= 0):
                        continue
                    if not ((y == cur.ymin and y == oth.ymin) or (y == cur.ymax and y == oth.ymax)):
                        continue
                    if x == oth.at(y):
                        off = -1 if y == ymax else 1
                        a, b = cur.at(y + off), oth.at(y + off)
                        if y == cur.ymax:
                            v = min(_lround(max(a, b)) + 1, x) if cur.dx > 0 else max(_lround(min(a, b)) - 1, x)
                        else:
                            v = max(_lround(min(a, b)) - 1, x) if cur.dx > 0 else min(_lround(max(a, b)) + 1, x)
                        if k < len(xx):          # slot k of the LIST, as Draw.c's xx[k]
                            xx[k] = F32(v)
                        break
        xx.sort()
        if not xx:
            continue
        x_pos = int(xx[0])                       # C's float -> int: toward zero
        for i in range(1, len(xx), 2):
            x_end = _round_down(xx[i])
            if x_end < x_pos:
                continue
            x_start = _round_up(xx[i - 1])
            if x_pos > x_start:
                x_start = x_pos
                if x_end < x_start:
                    continue
            spans.append((y, x_start, x_end))
            x_pos = x_end + 1
    return spans


def polygon_fill(img, pts, value=1):
    """ImageDraw.Draw(img).polygon(pts, fill=value) on a 2-D uint8 array (rows = y), in place: hline8's clipping."""
    h, w = img.shape
    for y, x0, x1 in polygon_spans(pts, h):
        if not 0 <= y < h or x0 >= w or x1 < 0:
            continue
        x0, x1 = max(x0, 0), min(x1, w - 1)
        if x0 <= x1:
            img[y, x0:x1 + 1] = value
    return img


# ------------------------------------------------------------------------------------------------------- the pipeline

def canvas_of(xbound, ybound):
    """pipeline.py:61-74 -> ((canvas_h, canvas_w), lidar2canvas float64 (3, 3))"""
    patch_h = ybound[1] - ybound[0]
    patch_w = xbound[1] - xbound[0]
    canvas_h = int(patch_h / ybound[2])
    canvas_w = int(patch_w / xbound[2])
    l2c = np.array([[canvas_h / patch_h, 0, canvas_h / 2], [0, canvas_w / patch_w, canvas_w / 2], [0, 0, 1]])
    return (canvas_h, canvas_w), l2c


def to_canvas(xy, l2c):
    """np.dot(np.pad(xy, 1.0), lidar2canvas.T)[..., :2] of :106-108 / :188-191: float32 points, float64 product"""
    xy = np.asarray(xy)
    padded = np.pad(xy, [(0, 0)] * (xy.ndim - 1) + [(0, 1)], constant_values=1.0)
    return np.dot(padded, l2c.T)[..., :2]


def quad_of(corners, l2c):
    """corners (8, 3) float32 -> the rounded bottom rectangle, int32 (4, 2) (:118, :197)"""
    return to_canvas(np.asarray(corners, np.float32)[list(BOTTOM), :2], l2c).round().astype(np.int32)


def vertex_margin(corners, l2c):
    """Distance of the float64 canvas coordinates of the bottom rectangles from the nearest half-integer (the rounded
    vertex is defined only where this is not within rounding of 0)."""
    c = to_canvas(np.asarray(corners, np.float32).reshape(-1, 8, 3)[:, list(BOTTOM), :2], l2c)
    return np.abs(c - np.floor(c) - 0.5).min() if c.size else np.inf


def quad_unsupported(q):
    """The one family that the map input does not draw (and counts in `flags`): two OPPOSITE vertices equal, the other two
    distinct from them and from each other, one of those two more than one pixel (Chebyshev) from the repeated vertex.
    No rectangle rounds to such a quad.  `polygon_fill` does not equal Pillow on this family."""
    q = [tuple(int(v) for v in p) for p in q]
    for rep, b, c in (((q[0], q[1], q[3]),) if q[0] == q[2] else ()) + (((q[1], q[0], q[2]),) if q[1] == q[3] else ()):
        if b == rep or c == rep or b == c:
            continue
        if max(abs(b[0] - rep[0]), abs(b[1] - rep[1])) > 1 or max(abs(c[0] - rep[0]), abs(c[1] - rep[1])) > 1:
            return True
    return False


def flagged(corners, l2c):
    """the number of boxes whose quad is of the family that is not drawn"""
    return sum(bool(quad_unsupported(quad_of(c, l2c))) for c in corners)


def object_layers(corners, labels, n_object, size, l2c):
    """_project_dynamic_bbox + the transpose of :215 -> (n_object, S, S) uint8, [c, x, y]"""
    dyn = np.zeros((n_object, size, size), np.uint8)
    labels = np.asarray(labels)
    for c in range(n_object):
        for i in np.nonzero(labels == c)[0]:
            q = quad_of(corners[i], l2c)
            if not quad_unsupported(q):
                polygon_fill(dyn[c], q)
    return dyn.transpose(0, 2, 1)


def aux_channels_of(aux_data):
    """channel count and the (name, first channel) of the names present, in the reference's fixed order"""
    names = [n for n, _ in AUX_DATA_CH]
    unknown = [a for a in aux_data if a not in names]
    if unknown:
        raise ValueError("unknown aux_data: %s" % unknown)
    ch, first = 0, {}
    for n, w in AUX_DATA_CH:
        if n in aux_data:
            first[n] = ch
            ch += w
    return ch, first


def box_aux_values(corners, bottom_center, height, visibility, l2c):
    """The eight values of one box in the order of AUX_DATA_CH, apart from the pixel's own coordinate: (visibility,
    centre x, centre y (float64), h, w, v0, v1 (float64), height)."""
    corners = np.asarray(corners, np.float32)
    front = corners[[4, 7], :2].mean(axis=0, dtype=np.float32)
    left = corners[[0, 4], :2].mean(axis=0, dtype=np.float32)
    cen, fr, le = (to_canvas(np.asarray(p, np.float32)[:2], l2c) for p in (bottom_center, front, left))
    d = fr - cen
    hh = np.sqrt(d[0] * d[0] + d[1] * d[1])
    e = le - cen
    ww = np.sqrt(e[0] * e[0] + e[1] * e[1])
    v = d / (hh + 1e-6)
    return visibility, cen, hh, ww, v, height


def aux_layers(corners, bottom_center, height, visibility, aux_data, size, l2c):
    """_get_dynamic_aux_bbox + the transpose of :173 -> (aux_ch, S, S) float32 [ch, x, y], or None"""
    if aux_data is None:
        return None
    ch, first = aux_channels_of(aux_data)
    if ch == 0:
        return None
    aux = np.zeros((size, size, ch), np.float32)
    coords = np.stack(np.meshgrid(np.arange(size), np.arange(size)), -1).astype(np.float32)
    for i in range(len(corners)):
        q = quad_of(corners[i], l2c)
        if quad_unsupported(q):
            continue
        mask = polygon_fill(np.zeros((size, size), np.uint8), q) > 0
        vis, cen, hh, ww, v, bh = box_aux_values(corners[i], bottom_center[i], height[i], visibility[i], l2c)
        if "visibility" in first:
            aux[mask, first["visibility"]] = vis
        if "center_offset" in first:
            k = first["center_offset"]
            aux[mask, k:k + 2] = coords[mask] - cen[None]
        if "center_ohw" in first:
            k = first["center_ohw"]
            aux[mask, k:k + 4] = np.array([hh, ww, v[0], v[1]])[None]
        if "height" in first:
            aux[mask, first["height"]] = np.array([float(height[i])])[None]
    return aux.transpose(2, 1, 0)


def one_hot_decode(data, n):
    """pipeline_utils.py:34-49 without numba -> (n, h, w) {0, 1}"""
    data = np.asarray(data)
    return ((data[..., None] >> np.arange(n, dtype=np.int32)) & 1).transpose(2, 0, 1)


def one_hot_encode(layers):
    """pipeline_utils.py:11-30 -> (h, w) int32"""
    layers = np.asarray(layers)
    assert layers.shape[0] <= 30
    shift = np.arange(layers.shape[0], dtype=np.int64)
    return ((layers.transpose(1, 2, 0) > 0).astype(np.int64) << shift).sum(-1).astype(np.int32)


def scene(static, corners, labels, bottom_center, height, visibility, n_object, aux_data, xbound, ybound):
    """One sample -> (gt_masks_bev (ns + nd, S, S) uint8, gt_aux_bev (aux_ch, S, S) float32 or None).  `static` is
    (ns, S, S) of 0 / 1."""
    (size, w), l2c = canvas_of(xbound, ybound)
    assert size == w
    dyn = object_layers(corners, labels, n_object, size, l2c)
    masks = np.concatenate([np.asarray(static).astype(np.uint8), dyn], axis=0)
    return masks, aux_layers(corners, bottom_center, height, visibility, aux_data, size, l2c)


def collate(masks, channels=8):
    """dataset/utils.py:341-345 (keys = ["gt_masks_bev"], [:8], .float()) -> float32 (b, channels, S, S)"""
    return np.stack([np.asarray(m)[:channels] for m in masks]).astype(np.float32)


# ------------------------------------------------------------------------------------------------------- test data

def box_corners(cx, cy, length, width, yaw, z=0.0, h=1.5):
    """Eight corners (8, 3) float32 of a box in the order that makes [0, 3, 7, 4] the bottom ring and [4, 7] the front
    edge: indices 0-3 at x_min side ... as mmdet3d 0.x's LiDARInstance3DBoxes numbers them (x front, y left, z up):
    0 (-,-,-) 1 (-,-,+) 2 (-,+,+) 3 (-,+,-) 4 (+,-,-) 5 (+,-,+) 6 (+,+,+) 7 (+,+,-)."""
    sx = np.array([-1, -1, -1, -1, 1, 1, 1, 1], np.float64) * length / 2
    sy = np.array([-1, -1, 1, 1, -1, -1, 1, 1], np.float64) * width / 2
    sz = np.array([0, 1, 1, 0, 0, 1, 1, 0], np.float64) * h
    c, s = math.cos(yaw), math.sin(yaw)
    out = np.stack([cx + c * sx - s * sy, cy + s * sx + c * sy, z + sz], axis=1)
    return out.astype(np.float32)


def corners_of_quad(quad, l2c, z=0.0, h=1.5):
    """Corners (8, 3) float32 whose bottom ring lands EXACTLY on the canvas quad `quad` ((4, 2) ints), for bounds whose
    scale is a power of two (the reference's: scale 2, offset 100): lidar = (canvas - offset) / scale is exact."""
    q = (np.asarray(quad, np.float64) - l2c[:2, 2]) / np.array([l2c[0, 0], l2c[1, 1]])
    out = np.zeros((8, 3), np.float32)
    for j, k in enumerate(BOTTOM):
        out[k, :2] = q[j]
        out[k, 2] = z
    for lo, hi in ((0, 1), (3, 2), (7, 6), (4, 5)):
        out[hi] = out[lo]
        out[hi, 2] = z + h
    return out


def random_scene(rng, n, n_object, xbound=(-50.0, 50.0, 0.5), ybound=(-50.0, 50.0, 0.5), spread=1.1, snap=True):
    """n boxes as a nuScenes scene has them (cars, trucks, pedestrians, cones) around the ego, some beyond the canvas.
    With `snap`, centres and sizes are multiples of 1/64 m and yaws give cos / sin that keep the canvas coordinates far
    from half-integers... which cannot be guaranteed in general: callers assert `vertex_margin`."""
    half = (xbound[1] - xbound[0]) / 2 * spread
    kinds = np.array([[4.6, 1.9, 1.7], [10.0, 2.8, 3.4], [0.7, 0.7, 1.8], [0.4, 0.4, 1.0], [2.0, 0.8, 1.5]])
    kind = rng.integers(0, len(kinds), n)
    size = kinds[kind] * rng.uniform(0.8, 1.2, (n, 3))
    cx, cy = rng.uniform(-half, half, n), rng.uniform(-half, half, n)
    yaw = rng.uniform(-math.pi, math.pi, n)
    quarter = rng.random(n) < 0.3
    yaw[quarter] = np.round(yaw[quarter] / (math.pi / 4)) * (math.pi / 4)
    z = rng.uniform(-2.0, 0.5, n)
    corners = np.stack([box_corners(cx[i], cy[i], size[i, 0], size[i, 1], yaw[i], z[i], size[i, 2]) for i in range(n)]) \
        if n else np.zeros((0, 8, 3), np.float32)
    bottom_center = np.stack([cx, cy, z], axis=1).astype(np.float32)
    height = size[:, 2].astype(np.float32)
    visibility = rng.integers(1, 5, n).astype(np.int64)
    labels = rng.integers(-1, n_object + 1, n).astype(np.int64)
    return {"corners": corners, "bottom_center": bottom_center, "height": height, "visibility": visibility, "labels": labels}
