"""The oracle of box output (dualdiff_amd/pipeline/box_output.py) and its case list.

Geometry in numpy float64 — the rules G1-G6 of include/dualdiff_hip.h (dd_box_edges) — then PIL's
`ImageDraw.Draw(im).line((x0, y0, x1, y1), fill=colour, width=1)` per edge in draw order on a PIL image, then G8.  Nothing
here shares code with the package.

Every case satisfies a MARGIN CONDITION, asserted below when the module is imported, so that the byte comparison does
not depend on the order in which the four-term sums of G1 are taken (numpy's matmul here, fused multiply-adds in the
kernel; the two differ by a few ulp of double, ~1e-12 relative at these magnitudes, far inside the margins):
  * every projected u, v of a drawn box is at least 1e-6 * max(1, |value|) from an integer;
  * every corner z is at least 1e-6 from 0;
  * the least z of the boxes drawn in one view differ pairwise by at least 1e-6;
  * no |coordinate| exceeds 2^20, except in the saturation case, where every value is either below 2^20 or above 2^30.
A case that violates it is a bug in the list: nothing is skipped.
"""
import collections
import functools

import numpy as np
from PIL import Image, ImageDraw

EDGES = ((0, 1), (0, 3), (0, 4), (1, 2), (1, 5), (3, 2), (3, 7), (4, 5), (4, 7), (2, 6), (5, 6), (6, 7))
SAT = 1 << 29
FLAG_LABEL, FLAG_SATURATED, FLAG_CAP = 1, 2, 4
FAULTS = ("any_z", "ascending", "round", "swapped_channel", "reversed_edge:1")
OBJECT_CLASSES = ("car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle",
                  "pedestrian", "traffic_cone")
# the nuScenes object colours (runner/map_visualizer.py:32-41), restated: the test compares them with the package's
PALETTE = ((255, 158, 0), (255, 99, 71), (233, 150, 70), (255, 127, 80), (255, 140, 0), (112, 128, 144), (255, 61, 99),
           (220, 20, 60), (0, 0, 230), (47, 79, 79))

Case = collections.namedtuple("Case", "name corners labels transforms h w frames saturating")


# ---- the line ---------------------------------------------------------------------------------------------------------

def line_pixels(x0, y0, x1, y1):
    """PIL's thin line in closed form (Python integers): the pixels of the line FROM (x0, y0) TO (x1, y1), unclipped."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    xs, ys = (1 if x1 >= x0 else -1), (1 if y1 >= y0 else -1)
    if dx >= dy:
        if dx == 0:
            return [(x0, y0)]
        return [(x0 + xs * i, y0 + ys * ((2 * dy * i + dx) // (2 * dx))) for i in range(dx + 1)]
    return [(x0 + xs * ((2 * dx * i + dy) // (2 * dy)), y0 + ys * i) for i in range(dy + 1)]


def on_line(px, py, x0, y0, x1, y1):
    """The same line as a membership test of one pixel, with no loop: what a lane of the kernel asks."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    ix = px - x0 if x1 >= x0 else x0 - px
    iy = py - y0 if y1 >= y0 else y0 - py
    if ix < 0 or ix > dx or iy < 0 or iy > dy:
        return False
    if dx >= dy:
        return dx == 0 or (2 * dy * ix + dx) // (2 * dx) == iy
    return (2 * dx * iy + dy) // (2 * dy) == ix


def pil_line_mask(h, w, x0, y0, x1, y1):
    """(h, w) bool: the pixels PIL's thin line sets."""
    im = Image.new("L", (w, h), 0)
    ImageDraw.Draw(im).line((x0, y0, x1, y1), fill=255, width=1)
    return np.asarray(im) > 0


# ---- geometry ---------------------------------------------------------------------------------------------------------

def project(corners, transform):
    """G1, G4 before the truncation: corners (k, 8, 3) fp32, transform (4, 4) fp32 -> (u, v, z), each (k, 8) float64."""
    c = np.asarray(corners, dtype=np.float32).astype(np.float64).reshape(-1, 8, 3)
    t = np.asarray(transform, dtype=np.float32).astype(np.float64)
    hom = np.concatenate([c, np.ones(c.shape[:2] + (1,))], axis=-1)
    xyz = hom @ t[:3].T
    zc = np.clip(xyz[..., 2], 1e-5, 1e5)
    return xyz[..., 0] / zc, xyz[..., 1] / zc, xyz[..., 2]


def to_int(u, fault=None):
    """G4: truncation toward zero, saturated at +-2^29 -> (int64 array, whether any value saturated)."""
    sat = np.abs(u) > SAT
    i = (np.rint(u) if fault == "round" else np.trunc(u))
    i = np.where(sat, np.sign(u) * SAT, i).astype(np.int64)
    return i, bool(sat.any())


def view_edges(corners, labels, transform, n_classes, cap=None, fault=None):
    """The boxes drawn in one view, in draw order -> (pts (kept', 8, 2) int64, cls (kept',) int64, count, flags): count is
    the number drawn, kept' = min(count, cap) the rows kept (the nearest ones)."""
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    k = labels.shape[0]
    flags = 0
    if k == 0:
        return np.zeros((0, 8, 2), np.int64), np.zeros((0,), np.int64), 0, 0
    u, v, z = project(corners, transform)
    good = (labels >= -n_classes) & (labels < n_classes)                          # G6
    if not good.all():
        flags |= FLAG_LABEL
    front = (z > 0).any(axis=1) if fault == "any_z" else (z > 0).all(axis=1)      # G2
    keep = np.nonzero(good & front)[0]
    min_z = z.min(axis=1)
    key = min_z[keep] if fault == "ascending" else -min_z[keep]
    order = keep[np.argsort(key, kind="stable")]                                  # G3: farthest first, ties to the lower index
    count = len(order)
    if cap is not None and count > cap:
        flags |= FLAG_CAP
        order = order[count - cap:]
    ui, su = to_int(u[order], fault)
    vi, sv = to_int(v[order], fault)
    if su or sv:
        flags |= FLAG_SATURATED
    return np.stack([ui, vi], axis=-1), np.where(labels[order] < 0, labels[order] + n_classes, labels[order]), count, flags


def edge_arrays(case, cap, n_classes=len(OBJECT_CLASSES), fault=None):
    """What dd_box_edges writes for a case at `cap` slots: (pts (s, v, cap, 8, 2) int32, cls (s, v, cap) int32, counts (s,
    v) int32, flags int)."""
    s, v = case.transforms.shape[:2]
    pts = np.zeros((s, v, cap, 8, 2), np.int32)
    cls = np.zeros((s, v, cap), np.int32)
    counts = np.zeros((s, v), np.int32)
    flags = 0
    for i in range(s):
        for j in range(v):
            p, c, n, f = view_edges(case.corners[i], case.labels[i], case.transforms[i, j], n_classes, cap, fault)
            pts[i, j, :len(p)], cls[i, j, :len(c)], counts[i, j] = p, c, n
            flags |= f
    return pts, cls, counts, flags


# ---- drawing ----------------------------------------------------------------------------------------------------------

def draw_view(frame, pts, cls, palette, h, w, transparent, fault=None):
    """G5, G7, G8 with PIL: frame (h, w, 3) uint8 or None; pts (k, 8, 2) integers in draw order; cls (k,) -> (h, w, 3) uint8,
    or (h, w, 4) with transparent."""
    im = Image.new("RGB", (w, h), (0, 0, 0)) if transparent else Image.fromarray(np.ascontiguousarray(frame))
    d = ImageDraw.Draw(im)
    for p, c in zip(np.asarray(pts).tolist(), np.asarray(cls).tolist()):
        colour = tuple(palette[c])
        if fault == "swapped_channel":
            colour = (colour[2], colour[1], colour[0])
        for e, (a, b) in enumerate(EDGES):
            if fault == "reversed_edge:%d" % e:
                a, b = b, a
            d.line((p[a][0], p[a][1], p[b][0], p[b][1]), fill=colour, width=1)
    rgb = np.asarray(im)
    if not transparent:
        return rgb.copy()
    alpha = np.where((rgb > 0).any(axis=-1), 255, 0).astype(np.uint8)
    return np.concatenate([rgb, alpha[..., None]], axis=-1)


def direction_boxes():
    """Twelve hand-made boxes, one per edge: box e has corner a of EDGES[e] at (10, 10), corner b at (12, 11) and every
    other corner straight above b, off the canvas, so that the pixel (11, 11) or (11, 10) tells the direction of edge e
    (tests/test_box_output_cpu.py asserts that it does) -> (12, 8, 2) int32, for a canvas of 16 x 24 each."""
    pts = np.empty((12, 8, 2), np.int32)
    pts[:] = (12, -50)
    for e, (a, b) in enumerate(EDGES):
        pts[e, a], pts[e, b] = (10, 10), (12, 11)
    return pts


def draw_arrays(frames, pts, cls, counts, palette, h, w, transparent):
    """What dd_box_draw_u8 writes from the arrays of dd_box_edges: frames (m, h, w, 3) or None, pts (m, cap, 8, 2), cls (m,
    cap), counts (m,) -> (m, h, w, 3 or 4)."""
    m, cap = cls.shape
    out = []
    for i in range(m):
        n = min(max(int(counts[i]), 0), cap)
        out.append(draw_view(None if frames is None else frames[i], pts[i, :n], cls[i, :n], palette, h, w, transparent))
    return np.stack(out)


def overlay(case, transparent, palette=PALETTE, fault=None):
    """The whole call for a case -> (s, v, h, w, 3 or 4) uint8."""
    s, v = case.transforms.shape[:2]
    out = np.zeros((s, v, case.h, case.w, 4 if transparent else 3), np.uint8)
    for i in range(s):
        for j in range(v):
            p, c, _, _ = view_edges(case.corners[i], case.labels[i], case.transforms[i, j], len(palette), None, fault)
            out[i, j] = draw_view(case.frames[i, j], p, c, palette, case.h, case.w, transparent, fault)
    return out


# ---- the cases --------------------------------------------------------------------------------------------------------

def cuboid(rs, centre, size, yaw):
    """The eight corners of a box, float32 (8, 3): corner k = (x, y, z) choices in the order 000 001 011 010 100 101 111 110,
    so that EDGES are the twelve edges of the cuboid."""
    signs = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 1], [0, 1, 0], [1, 0, 0], [1, 0, 1], [1, 1, 1], [1, 1, 0]], np.float64) - 0.5
    c, s = np.cos(yaw), np.sin(yaw)
    rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    return ((signs * size) @ rot.T + centre).astype(np.float32)


def camera(yaw, h, w, focal, roll=0.0):
    """A 4 x 4 fp32 lidar-to-image matrix: a camera at the origin looking along `yaw` in the lidar's x-y plane, turned by
    `roll` about its axis (so that the boxes' upright edges are no vertical lines)."""
    fwd = np.array([np.cos(yaw), np.sin(yaw), 0.0])
    right0 = np.array([np.sin(yaw), -np.cos(yaw), 0.0])
    down0 = np.array([0.0, 0.0, -1.0])
    right, down = np.cos(roll) * right0 + np.sin(roll) * down0, np.cos(roll) * down0 - np.sin(roll) * right0
    t = np.eye(4)
    t[0, :3] = focal * right + 0.5 * w * fwd
    t[1, :3] = focal * down + 0.5 * h * fwd
    t[2, :3] = fwd
    t[:3, 3] = (0.37 * w * 0.01, 0.41 * h * 0.01, -0.13)
    return t.astype(np.float32)


def random_scene(rs, k, spread):
    """k boxes around the origin (all around it with spread = pi, in front of yaw 0 with a small spread) and their labels,
    some of them negative (Python's indexing)."""
    boxes, labels = [], []
    for _ in range(k):
        r, a = rs.uniform(3.0, 45.0), rs.uniform(-spread, spread)
        centre = np.array([r * np.cos(a), r * np.sin(a), rs.uniform(-2.0, 1.0)])
        boxes.append(cuboid(rs, centre, rs.uniform(0.4, 6.0, size=3), rs.uniform(-np.pi, np.pi)))
        labels.append(int(rs.randint(-len(OBJECT_CLASSES), len(OBJECT_CLASSES))))
    return (np.stack(boxes) if boxes else np.zeros((0, 8, 3), np.float32)), np.asarray(labels, np.int64)


def make_case(name, seed, sizes, views, h, w, spread=np.pi, saturating=False, roll=0.0):
    rs = np.random.RandomState(seed)
    corners, labels = zip(*(random_scene(rs, k, spread) for k in sizes))
    transforms = np.stack([np.stack([camera(2 * np.pi * j / max(views, 3) + 0.1 * i, h, w, 0.9 * w, roll) for j in range(views)])
                           for i in range(len(sizes))])
    frames = rs.randint(0, 256, (len(sizes), views, h, w, 3)).astype(np.uint8)
    return Case(name, list(corners), list(labels), transforms, h, w, frames, saturating)


def saturating_case():
    """One view whose matrix scales x by 1e9: of its two boxes the first projects beyond +-2^30 in u (x = +-12 over z in
    (4, 6)), the second — flat in x = 0 — does not; v stays small."""
    rs = np.random.RandomState(5)
    a = cuboid(rs, np.array([0.31, 0.27, 5.03]), np.array([24.0, 1.1, 1.7]), 0.0)
    b = cuboid(rs, np.array([0.0, -0.61, 7.07]), np.array([0.0, 2.3, 1.9]), 0.0)
    t = np.array([[1e9, 0, 3.3, 0], [0, 40.0, 16.7, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
    frames = rs.randint(0, 256, (1, 1, 24, 40, 3)).astype(np.uint8)
    return Case("saturating", [np.stack([a, b])], [np.array([3, 8], np.int64)], t[None, None], 24, 40, frames, True)


def bad_label_case():
    c = make_case("bad_label", 11, (5,), 2, 37, 53, spread=0.5)
    c.labels[0][:] = (10, -10, -1, 9, -11)                  # 10 and -11 are outside [-10, 10)
    return c


def around_case():
    """Boxes all around the cameras, and in the second scene one that reaches through the camera plane of view 0 (four
    corners in front of it, four behind): G2 drops it there."""
    c = make_case("around", 3, (23, 4), 2, 48, 80, roll=0.4)
    through = cuboid(None, np.array([0.5, 0.2, 0.0]), np.array([3.0, 1.0, 1.0]), 0.0)
    c.corners[1] = np.concatenate([c.corners[1], through[None]])
    c.labels[1] = np.concatenate([c.labels[1], np.array([6], np.int64)])
    z = project(through[None], c.transforms[1, 0])[2]
    assert (z > 0).sum() == 4, "the box must straddle the camera plane"
    return c


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case.  `two_scenes` is also the whole-call case (2 x 3 views of 64 x 96, a scene without boxes and one with
    7); `seventy` ranks 70 boxes (more than one wave) in one view; `saturating` and `bad_label` raise their flag bits."""
    out = [make_case("two_scenes", 1, (0, 7), 3, 64, 96),
           make_case("seventy", 2, (70,), 1, 37, 53, spread=0.45),
           around_case(), bad_label_case(), saturating_case()]
    for c in out:
        check_margins(c)
        for a in (c.transforms, c.frames) + tuple(c.corners) + tuple(c.labels):
            a.setflags(write=False)
    return {c.name: c for c in out}


def check_margins(case, n_classes=len(OBJECT_CLASSES)):
    """The margin condition of the module's docstring; raises AssertionError naming the case."""
    s, v = case.transforms.shape[:2]
    for i in range(s):
        labels = np.asarray(case.labels[i])
        if len(labels) == 0:
            continue
        good = (labels >= -n_classes) & (labels < n_classes)
        for j in range(v):
            u, w_, z = project(case.corners[i], case.transforms[i, j])
            assert np.abs(z).min() >= 1e-6, (case.name, i, j, "a corner z within 1e-6 of 0")
            drawn = good & (z > 0).all(axis=1)
            mz = np.sort(z.min(axis=1)[drawn])
            assert len(mz) < 2 or np.diff(mz).min() >= 1e-6, (case.name, i, j, "two least z within 1e-6")
            for val in (u[drawn], w_[drawn]):
                if case.saturating:
                    assert ((np.abs(val) <= 1 << 20) | (np.abs(val) >= 1 << 30)).all(), (case.name, i, j, "a coordinate between 2^20 and 2^30")
                    val = val[np.abs(val) <= 1 << 20]
                else:
                    assert np.abs(val).max(initial=0.0) <= 1 << 20, (case.name, i, j, "a coordinate beyond 2^20")
                gap = np.abs(val - np.rint(val))
                assert (gap >= 1e-6 * np.maximum(1.0, np.abs(val))).all(), (case.name, i, j, "a coordinate within the margin of an integer")


cases()                                                     # the margin condition is asserted on import
