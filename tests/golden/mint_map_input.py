"""Mints tests/golden/map_input.npz by running the REFERENCE'S OWN `LoadBEVSegmentationM._project_dynamic` and
`_get_dynamic_aux` (magicdrive/dataset/pipeline.py, the object built by its own `__init__`), `one_hot_encode` /
`one_hot_decode` (dataset/pipeline_utils.py) and `collate_fn` (dataset/utils.py, for `bev_map_with_aux`) on three seeded
scenes of 0, 5 and 70 boxes at the reference's 200 x 200 canvas, so that tests/map_input_reference.py stays pinned to the
reference where the reference is not installed.  It also pins Pillow's own `ImageDraw.polygon(fill=1)` on a set of quads
(random rotated rectangles and every family of repeated vertices) for machines without PIL, and times the reference's
lines on this machine's CPU (printed; profiles/map_input.txt quotes them).

Runs only where the reference tree is (REF of tests/golden/mint_box_input.py); no test imports this module.  Everything
the reference's files import and this machine lacks is a name-only stand-in IN MEMORY (nothing is written to disk, no
reference code is copied): those of mint_box_input.py, and `nuscenes.map_expansion.map_api` (no locations, so `__init__`
loads no map), `mmdet.datasets.builder.PIPELINES` (a decorator that returns the class), three box class names of
`mmdet3d.core.bbox`, `h5py` and `numba` (`njit` returning the function: the bit fields run as plain numpy).  The stand-in
box class answers `len`, an index, a boolean mask, `.corners`, `.bottom_center` and `.height` from the arrays of
tests/map_input_reference.py's scene generator.

Usage:  python -m tests.golden.mint_map_input
"""
import math
import os
import sys
import time
import types

import numpy as np
import torch

from tests import map_input_reference as R
from tests.golden import mint_box_input as MB

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "map_input.npz")
BOUND = (-50.0, 50.0, 0.5)
COUNTS, SEED = (0, 5, 70), 20261
CLASSES = ["drivable_area", "ped_crossing", "walkway", "stop_line", "carpark_area", "road_divider", "lane_divider",
           "road_block"]
OBJECTS = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
           "traffic_cone"]
AUX = ["visibility", "center_offset", "center_ohw", "height"]
PIL_SIDE = 12


class MapBoxes:
    """Name-only stand-in for LiDARInstance3DBoxes as LoadBEVSegmentationM uses it."""

    def __init__(self, corners, bottom_center, height):
        self._c, self._b, self._h = (torch.as_tensor(np.asarray(v)) for v in (corners, bottom_center, height))

    def __len__(self):
        return self._c.shape[0]

    def __getitem__(self, i):
        if isinstance(i, (int, np.integer)):
            i = slice(int(i), int(i) + 1)
        elif isinstance(i, np.ndarray):
            i = torch.from_numpy(i)
        return MapBoxes(self._c[i], self._b[i], self._h[i])

    corners = property(lambda self: self._c)
    bottom_center = property(lambda self: self._b)
    height = property(lambda self: self._h)


def install_stubs():
    MB.install_stubs()

    class Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls

    class Name:
        def __init__(self, *a, **k):
            pass

    for pkg in ("nuscenes", "nuscenes.map_expansion", "mmdet", "mmdet.datasets"):
        MB._mod(pkg).__path__ = []
    MB._mod("nuscenes.map_expansion.map_api", NuScenesMap=Name, locations=[])
    MB._mod("mmdet.datasets.builder", PIPELINES=Registry())
    bbox = sys.modules["mmdet3d.core.bbox"]
    bbox.CameraInstance3DBoxes = bbox.DepthInstance3DBoxes = Name
    for name in ("h5py", "numba"):
        try:
            __import__(name)
        except ImportError:
            MB._mod(name, njit=lambda f: f)


def static_layers(rng, size):
    """eight layers of rectangles and stripes, as a road map has them"""
    st = np.zeros((len(CLASSES), size, size), np.int64)
    for k in range(len(CLASSES)):
        for _ in range(3):
            x0, y0 = rng.integers(0, size, 2)
            w, h = rng.integers(2, size // 2, 2)
            st[k, x0:x0 + w, y0:y0 + h] = 1
    return st


def pil_quads(rng):
    """the quads whose Pillow pictures are pinned: rotated rectangles (a third at multiples of 45 degrees, a fifth with
    edges of slope 1/2 and 2), partly off the canvas and at negative coordinates, and every quad with a repeated vertex
    on a 3 x 3 grid that straddles the canvas corner"""
    quads = []
    for it in range(1500):
        cx, cy = rng.uniform(-3, PIL_SIDE + 3, 2)
        l, w, yaw = rng.uniform(0.3, 14), rng.uniform(0.3, 6), rng.uniform(-math.pi, math.pi)
        if it % 3 == 0:
            yaw = round(yaw / (math.pi / 4)) * math.pi / 4
        elif it % 5 == 0:
            yaw = math.atan2(*((1, 2), (2, 1), (-1, 2), (1, -2))[it % 4])
            cx, cy, l, w = round(cx), round(cy), round(l) * math.sqrt(5), round(w) * math.sqrt(5)
        c, s = math.cos(yaw), math.sin(yaw)
        quads.append([np.round((cx + c * a * l / 2 - s * b * w / 2, cy + s * a * l / 2 + c * b * w / 2))
                      for a, b in ((-1, -1), (-1, 1), (1, 1), (1, -1))])
    pts = [(x, y) for x in (-1, 0, 2) for y in (-1, 1, 3)]
    for a in pts:
        for b in pts:
            for c in pts:
                for q in ((a, a, b, c), (a, b, b, c), (a, b, c, a), (a, b, a, c)):
                    if not R.quad_unsupported(q):
                        quads.append(q)
    return np.asarray(quads, np.int32)


def main():
    from PIL import Image, ImageDraw
    install_stubs()
    from magicdrive.dataset.pipeline import LoadBEVSegmentationM
    from magicdrive.dataset.pipeline_utils import one_hot_decode, one_hot_encode
    from magicdrive.dataset.utils import collate_fn
    load = LoadBEVSegmentationM("", BOUND, BOUND, CLASSES, object_classes=OBJECTS, aux_data=AUX)
    size = load.canvas_size[0]
    assert load.canvas_size == (200, 200)
    rng = np.random.default_rng(SEED)
    out = {"counts": np.array(COUNTS), "bound": np.array(BOUND), "lidar2canvas": load.lidar2canvas}
    masks, times = [], []
    for s, n in enumerate(COUNTS):
        sc = R.random_scene(rng, n, len(OBJECTS), BOUND, BOUND)
        static = static_layers(rng, size)
        bits = one_hot_encode(static)
        assert bits.dtype == np.int32 and np.array_equal(one_hot_decode(bits, len(CLASSES)), static)
        data = {"gt_bboxes_3d": MapBoxes(sc["corners"], sc["bottom_center"], sc["height"]), "gt_labels_3d": sc["labels"],
                "visibility": sc["visibility"]}
        t0 = time.perf_counter()
        final = load._project_dynamic(static, data)
        aux = load._get_dynamic_aux(data)
        times.append(time.perf_counter() - t0)
        assert final.shape == (18, size, size) and aux.shape == (8, size, size) and aux.dtype == np.float32
        for k, v in sc.items():
            out["%s_%d" % (k, s)] = v
        out["static_bits_%d" % s] = bits
        out["gt_masks_bev_%d" % s] = final.astype(np.uint8)
        out["gt_aux_bev_%d" % s] = aux
        masks.append(final)
    print("reference _project_dynamic + _get_dynamic_aux, seconds per scene of %s boxes: %s" % (COUNTS, times))
    # the 18-channel bit field of the cache, both ways
    out["masks_bits_2"] = one_hot_encode(masks[2])
    assert np.array_equal(one_hot_decode(out["masks_bits_2"], 18), masks[2])
    # bit 29: the highest layer one_hot_encode allows
    top = np.zeros((30, 4, 4), np.int64)
    top[29, 1, 2] = top[0, 3, 3] = top[29, 3, 3] = 1
    out["bits30"] = one_hot_encode(top)
    out["layers30"] = one_hot_decode(out["bits30"], 30).astype(np.uint8)
    # collate_fn's bev_map_with_aux over the three samples
    data = MB.RB.batch(MB.SEED, MB.COUNTS)
    examples = MB.examples_of(data)
    g = torch.Generator().manual_seed(SEED)
    for s, ex in enumerate(examples):
        ex["camera_intrinsics"] = MB.Held(torch.randn((6, 4, 4), generator=g))
        ex["camera2lidar"] = MB.Held(torch.randn((6, 4, 4), generator=g))
        ex["img"] = MB.Held(torch.zeros((6, 3) + MB.RB.CANVAS))
        ex["gt_masks_bev"] = masks[s]
        ex["gt_aux_bev"] = out["gt_aux_bev_%d" % s]
        ex["metas"] = MB.Held({"token": "scene%d" % s})
    cfg = types.SimpleNamespace(use_dual_controlnet=False, use_occ_3d=False, use_occ_3d_fg=False, use_occ_3d_bg=False,
                                use_map_vec=False, use_aug_text=False, use_aug_loss=False,
                                dataset=types.SimpleNamespace(image_size=list(MB.RB.CANVAS), object_classes=MB.RB.OBJECT_CLASSES))
    occ = {"scene%d" % s: torch.zeros((3, 4, 4)) for s in range(len(examples))}
    ret = collate_fn(examples, "", tokenizer=None, is_train=False, bbox_mode="all-xyz", bbox_view_shared=False,
                     occ_proj=occ, map_vec=None, cfg=cfg)
    bev = ret["bev_map_with_aux"]
    assert bev.dtype == torch.float32 and tuple(bev.shape) == (3, 8, size, size)
    out["bev_map_with_aux_bits"] = np.packbits(bev.numpy().astype(np.uint8))
    assert np.array_equal(bev.numpy(), bev.numpy().astype(np.uint8).astype(np.float32))
    # Pillow itself, pinned
    quads = pil_quads(rng)
    pics = np.zeros((len(quads), PIL_SIDE, PIL_SIDE), np.uint8)
    for i, q in enumerate(quads):
        im = Image.fromarray(pics[i])
        ImageDraw.Draw(im).polygon(q.flatten().tolist(), fill=1)
        pics[i] = np.array(im)
    out["pil_quads"] = quads.astype(np.int16)
    out["pil_masks"] = np.packbits(pics)
    import PIL
    out["pil_version"] = np.array(PIL.__version__)
    np.savez_compressed(PATH, **out)
    print("wrote %s (%d arrays, %d bytes)" % (PATH, len(out), os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
