"""Mints tests/golden/box_input.npz by running the REFERENCE'S OWN `_preprocess_bbox` and `collate_fn`
(magicdrive/dataset/utils.py) and `trans_boxes_to_views` (magicdrive/runner/box_visualizer.py) on the seeded batches of
tests/box_input_reference.py, so that the restatement there stays pinned to the reference where the reference is not
installed.  `collate_fn` is run for two of its results: the `use_aug_text` captions (the class sentences it appends, with
its rule of dropping the first unique class) and `camera_param`.

Runs only where the reference tree is (REF below); no test imports this module (the batches' seeds and configurations
are in tests/box_input_reference.py).  Everything those two files import
and this machine lacks is registered as a name-only stand-in IN MEMORY (as tests/golden/mint.py does; nothing is written to
disk, no reference code is copied): torchvision, mmdet3d.core.bbox[.structures], mmdet3d.core.utils, mmcv[.parallel.
data_container], cv2 — and the `magicdrive` packages themselves as empty namespaces over the reference's directories, so
that importing `magicdrive.dataset.utils` does not run the dataset package's __init__ (which needs the whole mmdet3d
dataset stack).  The stand-in box class holds the (N, 7) array the script gives it and answers `.corners` from the
generator of tests/box_input_reference.py for either origin; the reference sees it only through `len`, `.tensor`,
`.corners` and its constructor.

Usage:  python -m tests.golden.mint_box_input
"""
import os
import sys
import types

import numpy as np
import torch

from tests import box_input_reference as RB

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "box_input.npz")
REF = "/root/reference/MD_txt_con_fusion"
COUNTS, SEED, SEED_INVISIBLE = RB.GOLDEN_COUNTS, RB.GOLDEN_SEED, RB.GOLDEN_SEED_INVISIBLE
CONFIGS, config_name = RB.GOLDEN_CONFIGS, RB.config_name


class Boxes:
    """Name-only stand-in for LiDARInstance3DBoxes: the (N, 7) tensor, and corners from the test-data generator."""

    def __init__(self, tensor, box_dim=7, origin=RB.BOTTOM):
        self.tensor = torch.as_tensor(np.asarray(tensor), dtype=torch.float32).reshape(-1, box_dim)
        self.origin = tuple(origin)

    def __len__(self):
        return self.tensor.shape[0]

    @property
    def corners(self):
        return torch.from_numpy(RB.corners_of(self.tensor.numpy(), self.origin))


class Held:
    """mmcv's DataContainer as the collate function sees it: `.data`."""

    def __init__(self, data):
        self.data = data


def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def install_stubs():
    class Name:
        def __init__(self, *a, **k):
            pass

    from transformers import CLIPTokenizer  # noqa: F401  (before the stand-ins: it probes for the real torchvision)
    for pkg in ("magicdrive", "magicdrive.dataset", "magicdrive.runner", "magicdrive.networks"):
        _mod(pkg).__path__ = [os.path.join(REF, *pkg.split("."))]
    tv = _mod("torchvision")
    tv.__path__ = []
    tv.transforms = _mod("torchvision.transforms", Resize=Name)
    _mod("cv2")
    mmcv = _mod("mmcv")
    mmcv.__path__ = []
    par = _mod("mmcv.parallel")
    par.__path__ = []
    par.data_container = _mod("mmcv.parallel.data_container", DataContainer=Held)
    m3 = _mod("mmdet3d")
    m3.__path__ = []
    core = _mod("mmdet3d.core")
    core.__path__ = []
    bbox = _mod("mmdet3d.core.bbox", LiDARInstance3DBoxes=Boxes)
    bbox.__path__ = []
    _mod("mmdet3d.core.bbox.structures", LiDARInstance3DBoxes=Boxes, Box3DMode=Name)
    _mod("mmdet3d.core.utils", visualize_camera=None)
    for name in ("matplotlib", "accelerate.scheduler"):      # installed here; stand-ins only where they are not
        try:
            __import__(name)
        except ImportError:
            if name == "matplotlib":
                mpl = _mod("matplotlib")
                mpl.__path__ = []
                _mod("matplotlib.patches")
                _mod("matplotlib.pyplot")
            else:
                _mod("accelerate").__path__ = []
                _mod("accelerate.scheduler", AcceleratedScheduler=Name)


def examples_of(data):
    return [{"gt_bboxes_3d": Held(Boxes(b)), "gt_labels_3d": Held(torch.from_numpy(l)),
             "lidar2camera": Held(torch.from_numpy(data["lidar2camera"][s])),
             "lidar2image": Held(torch.from_numpy(data["lidar2image"][s])),
             "img_aug_matrix": Held(torch.from_numpy(data["img_aug_matrix"][s]))}
            for s, (b, l) in enumerate(zip(data["boxes"], data["labels"]))]


def collated(data):
    """The reference's whole collate function at test time with `use_aug_text`, an empty caption template and no
    tokenizer, on examples that carry the smallest stand-ins for what it touches besides the boxes: -> its captions (per
    (scene, camera): " " + the class sentence, capitalised, + "."), its camera_param and the inputs of that."""
    from magicdrive.dataset.utils import collate_fn
    g = torch.Generator().manual_seed(SEED)
    examples = examples_of(data)
    for s, ex in enumerate(examples):
        ex["camera_intrinsics"] = Held(torch.randn((6, 4, 4), generator=g))
        ex["camera2lidar"] = Held(torch.randn((6, 4, 4), generator=g))
        ex["img"] = Held(torch.zeros((6, 3) + RB.CANVAS))
        ex["gt_masks_bev"] = np.zeros((8, 4, 4), np.float32)
        ex["metas"] = Held({"token": "scene%d" % s})
    cfg = types.SimpleNamespace(use_dual_controlnet=False, use_occ_3d=False, use_occ_3d_fg=False, use_occ_3d_bg=False,
                                use_map_vec=False, use_aug_text=True, use_aug_loss=False,
                                dataset=types.SimpleNamespace(image_size=list(RB.CANVAS), object_classes=RB.OBJECT_CLASSES))
    occ = {"scene%d" % s: torch.zeros((3, 4, 4)) for s in range(len(examples))}
    ret = collate_fn(examples, "", tokenizer=None, is_train=False, bbox_mode="all-xyz", bbox_view_shared=False,
                     occ_proj=occ, map_vec=None, cfg=cfg)
    ref = _first_config(data)
    for key, v in ret["kwargs"]["bboxes_3d_data"].items():       # the collate function calls _preprocess_bbox as CONFIGS[0]
        assert torch.equal(v, ref[key]), key
    assert len(ret["captions"]) == 6 * len(examples)
    return {"aug_captions": np.array(ret["captions"]), "camera_param": ret["camera_param"].numpy(),
            "camera_intrinsics": torch.stack([ex["camera_intrinsics"].data for ex in examples]).numpy(),
            "camera2lidar": torch.stack([ex["camera2lidar"].data for ex in examples]).numpy()}


def _first_config(data):
    from magicdrive.dataset.utils import _preprocess_bbox
    mode, shared, f3d = CONFIGS[0]
    return _preprocess_bbox(mode, RB.CANVAS, examples_of(data), is_train=False, view_shared=shared, use_3d_filter=f3d)[0]


def main():
    install_stubs()
    from magicdrive.dataset.utils import _preprocess_bbox
    from magicdrive.runner.box_visualizer import trans_boxes_to_views
    out = {"counts": np.array(COUNTS), "seeds": np.array([SEED, SEED_INVISIBLE]), "canvas": np.array(RB.CANVAS)}
    data = RB.batch(SEED, COUNTS)
    for s in range(len(COUNTS)):
        for key in ("boxes", "labels", "corners", "filter_corners"):
            out["%s_%d" % (key, s)] = data[key][s]
    for key in ("lidar2camera", "lidar2image", "img_aug_matrix"):
        out[key] = data[key]
    for mode, shared, f3d in CONFIGS:
        ret, _ = _preprocess_bbox(mode, RB.CANVAS, examples_of(data), is_train=False, view_shared=shared, use_3d_filter=f3d)
        name = config_name(mode, shared, f3d)
        assert ret["bboxes"].dtype == torch.float32 and ret["classes"].dtype == torch.int64 and ret["masks"].dtype == torch.bool
        for key, v in ret.items():
            out["%s_%s" % (name, key)] = v.numpy()
    # the projected coordinates of the 5-box scene, both forms (float64)
    five = Boxes(data["boxes"][1])
    for proj, key in ((False, "lidar2camera"), (True, "lidar2image")):
        coords = trans_boxes_to_views(five, data[key][1], data["img_aug_matrix"][1], proj)
        out["coords_proj%d" % proj] = np.stack(coords)
        assert out["coords_proj%d" % proj].dtype == np.float64
    # nothing visible anywhere: (None, None)
    inv = RB.batch(SEED_INVISIBLE, COUNTS, invisible=True)
    for f3d in (True, False):
        ret = _preprocess_bbox("all-xyz", RB.CANVAS, examples_of(inv), is_train=False, view_shared=False, use_3d_filter=f3d)
        out["invisible_is_none_%s" % ("z" if f3d else "canvas")] = np.array(ret[0] is None and ret[1] is None)
    try:
        _preprocess_bbox("owhr", RB.CANVAS, examples_of(data), is_train=False)
        out["owhr_raises"] = np.array(False)
    except NotImplementedError:
        out["owhr_raises"] = np.array(True)
    out.update(collated(data))
    np.savez_compressed(PATH, **out)
    print("wrote %s (%d arrays, %d bytes)" % (PATH, len(out), os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
