"""The FGM loss mask and the masked loss, restated in numpy / plain Python: what `create_heatmap_gt(..., resolution)`
(magicdrive/networks/utils.py:26-39, 100-163) makes of `for_mask` and `lidar2image`, `hd_crop` (dataset/utils.py:348-353), and
the two loss lines of runner/multiview_runner.py:506-507 in float64.  scipy and matplotlib are NOT imported here: the hull
is a strict monotone chain and the point-in-polygon rule is matplotlib's crossing rule in integers, both established against
the libraries by tests/test_fgm_mask_cpu.py and against the reference's own run by tests/golden/fgm_mask.npz.

Per (scene, view, box) with mask true:
  * corners fp32 -> float64, `[x, y, z, 1] @ T.T` with T the float32 lidar2image in float64, every product and sum a single
    IEEE operation, summed k = 0, 1, 2, 3 (`project` spells the operations out; the reference's `@` goes through BLAS);
  * points with z <= 0 are dropped; z is clipped to [1e-5, 1e5]; x / z * (W / source_w), y / z * (H / source_h); truncation
    toward zero;
  * the polygon is the counter-clockwise strict convex hull where that has three vertices or more (what qhull returns),
    else the surviving points in corner order (`ConvexHull` raised, `except: pass`); no point, no paint;
  * a pixel (tx, ty) of the W x H grid is painted where `inside` says so; area = the painted pixels of the UNCROPPED grid;
    the box's weight is float32(1.0 - area / (W * H)).
A box is UNSUPPORTED (not painted, counted) where a projected x, y or z of any of its points is not finite, or a surviving
point's scaled coordinate is not finite or truncates beyond 2^25 in magnitude: there the reference's own float64 products of
the crossing test stop being exact and its integer cast is undefined.
The view's map is the maximum over its boxes, 0 where none paints.
"""
import math

import numpy as np

BOUND = 1 << 25
SOURCE = (1600, 900)


def project(corners, trans, resolution, source=SOURCE):
    """corners (P, 3) float32, trans (4, 4) float32 -> (the surviving points as (x, y) Python ints in corner order,
    unsupported?)"""
    sx, sy = resolution[0] / source[0], resolution[1] / source[1]
    c = np.asarray(corners, np.float32).reshape(-1, 3)
    t = np.asarray(trans, np.float32).reshape(4, 4)
    pts, bad = [], False
    for p in c:
        v = (float(p[0]), float(p[1]), float(p[2]), 1.0)
        r = []
        for row in range(3):
            acc = v[0] * float(t[row, 0])
            for k in (1, 2, 3):
                acc = acc + v[k] * float(t[row, k])
            r.append(acc)
        x, y, z = r
        if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
            bad = True
            continue
        if not z > 0.0:
            continue
        z = min(max(z, 1e-5), 1e5)
        x = (x / z) * sx
        y = (y / z) * sy
        if not (math.isfinite(x) and math.isfinite(y)) or abs(int(x)) > BOUND or abs(int(y)) > BOUND:
            bad = True
            continue
        pts.append((int(x), int(y)))                       # int() truncates toward zero, as astype(int) does
    return pts, bad


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def hull(pts):
    """The strict convex hull (collinear and repeated points dropped) of integer points, counter-clockwise in (x, y)
    starting from the lexicographically smallest; fewer than three vertices for a degenerate set."""
    p = sorted(pts)
    if len(p) < 2:
        return []
    h = []
    for q in p:
        while len(h) >= 2 and _cross(h[-2], h[-1], q) <= 0:
            h.pop()
        h.append(q)
    t = len(h) + 1
    for q in reversed(p[:-1]):
        while len(h) >= t and _cross(h[-2], h[-1], q) <= 0:
            h.pop()
        h.append(q)
    return h[:-1]


def ring(pts):
    h = hull(pts)
    return h if len(h) >= 3 else list(pts)


def inside(rng, tx, ty):
    """matplotlib's `Polygon(ring, closed=True).contains_point((tx, ty), radius=0)` for integer vertices and an integer
    point: the even-odd crossing rule over the edges v0 -> v1 of the closed ring."""
    n, res = len(rng), False
    for i in range(n):
        (x0, y0), (x1, y1) = rng[i], rng[(i + 1) % n]
        f0, f1 = y0 >= ty, y1 >= ty
        if f0 != f1 and (((y1 - ty) * (x0 - x1) >= (x1 - tx) * (y0 - y1)) == f1):
            res = not res
    return res


def paint(rng, width, height):
    """-> bool (height, width): `inside` at every pixel of the grid, vectorised (int64; exact within BOUND)"""
    res = np.zeros((height, width), bool)
    n = len(rng)
    if n == 0:
        return res
    tx = np.arange(width, dtype=np.int64)[None, :]
    ty = np.arange(height, dtype=np.int64)[:, None]
    for i in range(n):
        (x0, y0), (x1, y1) = rng[i], rng[(i + 1) % n]
        f0, f1 = y0 >= ty, y1 >= ty
        side = ((y1 - ty) * (x0 - x1) >= (x1 - tx) * (y0 - y1)) == f1
        res ^= (f0 != f1) & side
    return res


def crop_of(x, out_shape):
    """hd_crop: drop the top rows and the same number of columns on each side, (H, W) -> out_shape = (H_out, W_out)"""
    if out_shape is None:
        return x
    h, w = x.shape[-2:]
    hc, wc = h - out_shape[0], (w - out_shape[1]) // 2
    y = x[..., hc:, wc:w - wc]
    assert y.shape[-2:] == tuple(out_shape)
    return y


def heatmap(bboxes, masks, lidar2image, resolution, crop=None, source=SOURCE):
    """bboxes (b, n, m, P, 3) float32, masks (b, n, m) bool, lidar2image (b, n, 4, 4) float32, resolution = (W, H), crop =
    (H_out, W_out) or None -> dict: heat (b, n, H_out, W_out) float32, flagged (int), area / weight / unsupported (b, n, m),
    rings (a list per box)."""
    bboxes, masks = np.asarray(bboxes, np.float32), np.asarray(masks).astype(bool)
    b, n, m = masks.shape
    width, height = resolution
    heat = np.zeros((b, n, height, width), np.float32)
    area = np.zeros((b, n, m), np.int64)
    weight = np.zeros((b, n, m), np.float32)
    unsupported = np.zeros((b, n, m), bool)
    rings = {}
    for i in range(b):
        for j in range(n):
            for k in range(m):
                if not masks[i, j, k]:
                    continue
                pts, bad = project(bboxes[i, j, k], lidar2image[i, j], resolution, source)
                if bad:
                    unsupported[i, j, k] = True
                    continue
                rg = ring(pts)
                rings[(i, j, k)] = rg
                px = paint(rg, width, height)
                area[i, j, k] = int(px.sum())
                weight[i, j, k] = np.float32(1.0 - int(px.sum()) / (width * height))
                heat[i, j] = np.maximum(heat[i, j], px.astype(np.float32) * weight[i, j, k])
    return {"heat": np.ascontiguousarray(crop_of(heat, crop)), "flagged": int(unsupported.sum()), "area": area,
            "weight": weight, "unsupported": unsupported, "rings": rings}


# ---- seeded inputs (the fixture's, the timing tool's) -----------------------------------------------------------------------

def scenes(seed, counts, cap, visible=None):
    """random boxes (re-centred corners) and ring cameras, counts[scene][view] boxes with mask true, padded to cap.
    visible = a grid: only boxes with a corner on that grid, as the canvas filter of `for_mask` leaves them"""
    from tests import box_input_reference as RB
    b, n = len(counts), len(counts[0])
    bboxes, masks = np.zeros((b, n, cap, 8, 3), np.float32), np.zeros((b, n, cap), bool)
    l2i = np.zeros((b, n, 4, 4), np.float32)
    for i in range(b):
        l2i[i] = RB.ring_cameras(seed + i, n)[1]
        for j in range(n):
            k = counts[i][j]
            c = RB.corners_of(RB.boxes(seed + 10 * i + j, 40 * k if visible else k, extent=30.0), RB.CENTRE)
            if visible:
                seen = [any(0 <= x < visible[0] and 0 <= y < visible[1] for x, y in project(q, l2i[i, j], visible)[0])
                        for q in c]
                c = c[np.array(seen, bool)]
            bboxes[i, j, :k] = c[:k]
            masks[i, j, :k] = True
    return bboxes, masks, l2i


# ---- the loss -----------------------------------------------------------------------------------------------------------

def loss(pred, target, heat=None):
    """pred, target (b, n, c, h, w), heat (b, n, h, w) or None, any float arrays -> (value, grad_pred) in float64:
    mean((p - t)^2) + mean((p - t)^2 * heat[:, :, None]) and its derivative 2 (p - t) (1 + heat) / N."""
    p, t = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    w = np.ones(p.shape[:2] + (1,) + p.shape[3:]) if heat is None else 1.0 + np.asarray(heat, np.float64)[:, :, None]
    d = p - t
    return float((d * d * w).sum() / d.size), 2.0 * d * w / d.size


# The reduction tree of dd_fgm_loss (include/dualdiff_hip.h), for the tests' bound.
LOSS_THREADS, LOSS_PER_GROUP, LOSS_MAX_GROUPS = 256, 1024, 1024


def loss_groups(count):
    return max(1, min((count + LOSS_PER_GROUP - 1) // LOSS_PER_GROUP, LOSS_MAX_GROUPS))


def loss_roundings(count):
    """The number of fp32 roundings on the longest path from an input element to the value: 5 for the term (p - t carries
    one, its square that one twice and its own, 1 + heat one, the product one), the serial adds of a lane, 6 levels across
    the wave and 3 adds across the four waves, the same again over the partials, the conversion of N and the division."""
    groups = loss_groups(count)
    serial = (count + groups * LOSS_THREADS - 1) // (groups * LOSS_THREADS)
    final = (groups + LOSS_THREADS - 1) // LOSS_THREADS
    return 5 + serial + 6 + 3 + final + 6 + 3 + 2
