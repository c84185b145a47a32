"""The reference's box pre-processing restated in numpy float64, and a deterministic test-data generator.

Restated (tests/test_box_input_cpu.py pins it to tests/golden/box_input.npz, which the reference's own functions wrote):
  * the transform of runner/box_visualizer.py:49-86 (`trans_boxes_to_view`): homogeneous corners in float64 times the
    transposed float32 matrix, and with `proj` x, y divided by z clipped to [1e-5, 1e5] and z by |z|;
  * the two filters of dataset/utils.py:60-82 (`ensure_canvas`, `ensure_positive_z`);
  * selection and padding of dataset/utils.py:128-262 (`_preprocess_bbox` at test time), with the `cxyz` pick;
  * the aug-text rule of dataset/utils.py:496-506.

The generator makes boxes (x, y, z, dx, dy, dz, yaw), their eight corners about any origin, and six ring cameras.  It is
data generation only: it does not claim mmdet3d's corner order or yaw convention.
"""
import numpy as np
import torch

CANVAS = (224, 400)
CXYZ = [6, 5, 7, 2]
OBJECT_CLASSES = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle",
                  "pedestrian", "traffic_cone"]
BOTTOM, CENTRE = (0.5, 0.5, 0.0), (0.5, 0.5, 0.5)
MARGIN = 1e-6
# the batches of tests/golden/box_input.npz (tests/golden/mint_box_input.py runs the reference on them)
GOLDEN_COUNTS = (0, 5, 70)
GOLDEN_SEED, GOLDEN_SEED_INVISIBLE = 3, 4
# (bbox_mode, view_shared, use_3d_filter)
GOLDEN_CONFIGS = [("all-xyz", False, True), ("all-xyz", False, False), ("cxyz", False, True), ("cxyz", False, False),
                  ("all-xyz", True, True), ("cxyz", True, True)]


def config_name(mode, shared, f3d):
    return "%s_%s_%s" % (mode.replace("-", ""), "shared" if shared else "views", "z" if f3d else "canvas")


# ---- data ---------------------------------------------------------------------------------------------------------------

def boxes(seed, n, extent=50.0):
    """(n, 7) float32: x, y within +-extent, z in [-3, 1], sizes in [0.5, 6], yaw in [-pi, pi)."""
    g = np.random.default_rng(seed)
    b = np.empty((n, 7))
    b[:, :2] = g.uniform(-extent, extent, (n, 2))
    b[:, 2] = g.uniform(-3.0, 1.0, n)
    b[:, 3:6] = g.uniform(0.5, 6.0, (n, 3))
    b[:, 6] = g.uniform(-np.pi, np.pi, n)
    return b.astype(np.float32)


def labels(seed, n):
    return np.random.default_rng(seed + 7919).integers(0, len(OBJECT_CLASSES), n).astype(np.int64)


def corners_of(b, origin=BOTTOM):
    """(n, 7) -> (n, 8, 3) float32: the unit cube's corners (0,0,0) (0,0,1) (0,1,1) (0,1,0) (1,0,0) (1,0,1) (1,1,1) (1,1,0)
    minus `origin`, times the sizes, turned about z by yaw, moved to (x, y, z).  float32 arithmetic throughout."""
    b = np.asarray(b, dtype=np.float32).reshape(-1, 7)
    unit = np.array([[0, 0, 0], [0, 0, 1], [0, 1, 1], [0, 1, 0], [1, 0, 0], [1, 0, 1], [1, 1, 1], [1, 1, 0]], np.float32)
    c = (unit - np.asarray(origin, np.float32))[None] * b[:, None, 3:6]
    cos, sin = np.cos(b[:, 6])[:, None], np.sin(b[:, 6])[:, None]
    out = np.empty_like(c)
    out[..., 0] = c[..., 0] * cos - c[..., 1] * sin
    out[..., 1] = c[..., 0] * sin + c[..., 1] * cos
    out[..., 2] = c[..., 2]
    return (out + b[:, None, :3]).astype(np.float32)


def ring_cameras(seed, n=6, yaw0=0.0, spread=2 * np.pi):
    """n cameras on a ring (x right, y down, z forward), looking outwards `spread / n` apart with a small seeded pitch and
    offset -> (lidar2camera, lidar2image, img_aug_matrix), each (n, 4, 4) float32.  The intrinsics are those of a 1600 x 900
    image; the augmentation is its resize by 0.25 with one row cut from the top: the 224 x 400 canvas."""
    g = np.random.default_rng(seed + 104729)
    l2c, l2i, aug = (np.zeros((n, 4, 4), np.float32) for _ in range(3))
    for i in range(n):
        yaw = yaw0 + spread * i / n + g.uniform(-0.05, 0.05)
        pitch = g.uniform(-0.03, 0.03)
        pos = np.array([g.uniform(-1, 1), g.uniform(-0.5, 0.5), g.uniform(1.3, 1.7)])
        fwd = np.array([np.cos(yaw) * np.cos(pitch), np.sin(yaw) * np.cos(pitch), np.sin(pitch)])
        right = np.array([np.sin(yaw), -np.cos(yaw), 0.0])
        down = np.cross(fwd, right)
        rot = np.stack([right, down, fwd])
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = rot, -rot @ pos
        k = np.eye(4)
        k[0, 0] = k[1, 1] = 1266.0 + g.uniform(-10, 10)
        k[0, 2], k[1, 2] = 816.0 + g.uniform(-5, 5), 491.0 + g.uniform(-5, 5)
        l2c[i] = m.astype(np.float32)
        l2i[i] = k.astype(np.float32) @ l2c[i]
        aug[i] = np.array([[0.25, 0, 0, 0], [0, 0.25, 0, -1], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
    return l2c, l2i, aug


def batch(seed, counts, views=6, invisible=False):
    """A batch of len(counts) scenes: per-scene boxes, labels, payload and filter corners, and the (b, views, 4, 4)
    matrices.  invisible: every camera looks along +x and every box lies behind them."""
    out = {"boxes": [], "labels": [], "corners": [], "filter_corners": [], "lidar2camera": [], "lidar2image": [],
           "img_aug_matrix": []}
    for s, n in enumerate(counts):
        b = boxes(seed * 100 + s, n)
        if invisible:
            b[:, 0] = -np.abs(b[:, 0]) - 12.0
            cams = ring_cameras(seed * 100 + s, views, spread=0.0)
        else:
            cams = ring_cameras(seed * 100 + s, views)
        out["boxes"].append(b)
        out["labels"].append(labels(seed * 100 + s, n))
        out["corners"].append(corners_of(b, BOTTOM))
        out["filter_corners"].append(corners_of(b, CENTRE))
        for key, m in zip(("lidar2camera", "lidar2image", "img_aug_matrix"), cams):
            out[key].append(m)
    for key in ("lidar2camera", "lidar2image", "img_aug_matrix"):
        out[key] = np.stack(out[key])
    return out


def transforms_of(data, use_3d_filter):
    """aug @ lidar2camera (3D filter) or aug @ lidar2image (canvas filter) per view, float32, as the reference composes."""
    trans = data["lidar2camera" if use_3d_filter else "lidar2image"]
    out = np.empty_like(trans)
    for b in range(trans.shape[0]):
        for n in range(trans.shape[1]):
            out[b, n] = data["img_aug_matrix"][b, n] @ trans[b, n]
    return out


# ---- the restatement ----------------------------------------------------------------------------------------------------

def view_coords(filter_corners, trans, proj):
    """(N, 8, 3) corners, one (4, 4) float32 matrix -> ((N, 8, 3) float64 as the reference returns them, the raw z (N, 8))."""
    pts = np.asarray(filter_corners).reshape(-1, 3)
    hom = np.concatenate([pts.astype(np.float64), np.ones((pts.shape[0], 1))], axis=-1)
    c = hom @ np.asarray(trans).reshape(4, 4).astype(np.float64).T
    raw_z = c[:, 2].copy()
    if proj:
        with np.errstate(divide="ignore", invalid="ignore"):
            z = np.clip(c[:, 2], 1e-5, 1e5)
            c[:, 0] /= z
            c[:, 1] /= z
            c[:, 2] /= np.abs(c[:, 2])
    return c[:, :3].reshape(-1, 8, 3), raw_z.reshape(-1, 8)


def keep_positive_z(coords):
    return (coords[..., 2] > 0).any(1)


def keep_canvas(coords, canvas_size):
    """A box stays if some corner is in front, some corner's x is inside the canvas width and some corner's y inside its
    height — three separate questions, each over the box's eight corners."""
    h, w = canvas_size
    x, y, z = coords[..., 0], coords[..., 1], coords[..., 2]
    in_front = (z > 0).any(1)
    in_width = ((x > 0) & (x < w)).any(1)
    in_height = ((y > 0) & (y < h)).any(1)
    return in_front & in_width & in_height


def visibility(filter_corners, transforms, use_3d_filter, canvas_size=CANVAS):
    """Per scene a (views, N_i) bool array, and the smallest distance of a decisive quantity from its threshold: corner
    z from 0, and for the canvas filter x from 0 and w, y from 0 and h."""
    keeps, margin = [], np.inf
    for s, fc in enumerate(filter_corners):
        rows = []
        for trans in transforms[s]:
            if len(fc) == 0:
                rows.append(np.zeros(0, bool))
                continue
            coords, raw_z = view_coords(fc, trans, proj=not use_3d_filter)
            margin = min(margin, np.abs(raw_z).min())
            if use_3d_filter:
                rows.append(keep_positive_z(coords))
            else:
                h, w = canvas_size
                x, y = coords[..., 0], coords[..., 1]
                margin = min(margin, np.abs(x).min(), np.abs(x - w).min(), np.abs(y).min(), np.abs(y - h).min())
                rows.append(keep_canvas(coords, canvas_size))
        keeps.append(np.stack(rows))
    return keeps, float(margin)


def select(corners, labels_, keeps, bbox_mode, length):
    """Rows of `length` slots: the kept boxes of every (scene, view) in order (those beyond `length` dropped), padded with
    zero points / class -1 / mask False -> (bboxes, classes, masks, counts) as numpy arrays."""
    if bbox_mode not in ("cxyz", "all-xyz"):
        raise NotImplementedError("Wrong mode %s" % bbox_mode)
    b, views = len(corners), keeps[0].shape[0]
    pts = 4 if bbox_mode == "cxyz" else 8
    bboxes = np.zeros((b, views, length, pts, 3), np.float32)
    classes = -np.ones((b, views, length), np.int64)
    masks = np.zeros((b, views, length), bool)
    counts = np.zeros((b, views), np.int32)
    for s in range(b):
        c = np.asarray(corners[s], np.float32).reshape(-1, 8, 3)
        c = c[:, CXYZ] if bbox_mode == "cxyz" else c
        for v in range(views):
            idx = np.nonzero(keeps[s][v])[0]
            counts[s, v] = len(idx)
            idx = idx[:length]
            bboxes[s, v, :len(idx)] = c[idx]
            classes[s, v, :len(idx)] = np.asarray(labels_[s], np.int64)[idx]
            masks[s, v, :len(idx)] = True
    return bboxes, classes, masks, counts


def keeps_of(data, view_shared, use_3d_filter, canvas_size=CANVAS):
    """-> (per-scene (views, N_i) bool, margin); view_shared: one view that keeps everything."""
    if view_shared:
        return [np.ones((1, len(c)), bool) for c in data["corners"]], np.inf
    return visibility(data["filter_corners"], transforms_of(data, use_3d_filter), use_3d_filter, canvas_size)


def preprocess(data, bbox_mode, view_shared, use_3d_filter, canvas_size=CANVAS):
    """`_preprocess_bbox(...)[0]` at test time: {"bboxes", "classes", "masks"} as torch tensors, or None."""
    keeps, _ = keeps_of(data, view_shared, use_3d_filter, canvas_size)
    max_len = max(int(k.sum(axis=1).max()) if k.size else 0 for k in keeps)
    if bbox_mode not in ("cxyz", "all-xyz"):
        raise NotImplementedError("Wrong mode %s" % bbox_mode)
    if max_len == 0:
        return None
    bboxes, classes, masks, _ = select(data["corners"], data["labels"], keeps, bbox_mode, max_len)
    return {"bboxes": torch.from_numpy(bboxes), "classes": torch.from_numpy(classes), "masks": torch.from_numpy(masks)}


def add_uncond(d):
    """The CFG layout of `add_uncond_to_kwargs`: an all-zero half in front."""
    return {k: torch.cat([torch.zeros_like(v), v]) for k, v in d.items()}


def aug_text(classes, names=OBJECT_CLASSES):
    """dataset/utils.py:496-506: per (scene, view) the sorted unique classes without the first, as names."""
    out = []
    for scene in np.asarray(classes):
        for view in scene:
            out.append(", ".join(names[i] for i in np.unique(view)[1:].tolist()))
    return out
