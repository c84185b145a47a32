"""Box input without a GPU: the restatement (tests/box_input_reference.py) against what the reference's own
`_preprocess_bbox` / `trans_boxes_to_views` returned (tests/golden/box_input.npz, written by tests/golden/mint_box_input.py),
the host-side helpers of dualdiff_amd/pipeline/box_input.py, and dd_box_views' validation and ABI entry."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dualdiff_amd import _native
from dualdiff_amd.pipeline import box_input as BI
from tests import box_input_reference as RB

CONFIGS, COUNTS, config_name = RB.GOLDEN_CONFIGS, RB.GOLDEN_COUNTS, RB.config_name
SEED, SEED_INVISIBLE = RB.GOLDEN_SEED, RB.GOLDEN_SEED_INVISIBLE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG = -1
P = 16                                                   # non-null, 16-byte aligned, never dereferenced


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "box_input.npz"))


@pytest.fixture(scope="module")
def data():
    return RB.batch(SEED, COUNTS)


# ---- the restatement against the reference's results -------------------------------------------------------------------

def test_generator_reproduces_the_fixture_inputs(golden, data):
    assert tuple(golden["counts"]) == COUNTS and tuple(golden["canvas"]) == RB.CANVAS
    for s in range(len(COUNTS)):
        for key in ("boxes", "labels", "corners", "filter_corners"):
            assert np.array_equal(golden["%s_%d" % (key, s)], data[key][s]), (key, s)
    for key in ("lidar2camera", "lidar2image", "img_aug_matrix"):
        assert np.array_equal(golden[key], data[key]) and data[key].dtype == np.float32


@pytest.mark.parametrize("mode,shared,f3d", CONFIGS, ids=[config_name(*c) for c in CONFIGS])
def test_restatement_equals_the_reference(golden, data, mode, shared, f3d):
    got = RB.preprocess(data, mode, shared, f3d)
    name = config_name(mode, shared, f3d)
    for key, dtype in (("bboxes", torch.float32), ("classes", torch.int64), ("masks", torch.bool)):
        want = torch.from_numpy(golden["%s_%s" % (name, key)])
        assert got[key].dtype == dtype == want.dtype and torch.equal(got[key], want), (name, key)
    assert got["masks"].any() and not got["masks"][0].any()          # the first scene has no box
    _, margin = RB.keeps_of(data, shared, f3d)
    assert margin >= RB.MARGIN


def test_projected_coordinates_equal_the_reference(golden, data):
    """trans_boxes_to_views on the 5-box scene, float64: the same numpy product on the same operands, bit for bit."""
    for proj, key in ((False, "lidar2camera"), (True, "lidar2image")):
        want = golden["coords_proj%d" % proj]
        trans = RB.transforms_of(data, use_3d_filter=not proj)[1]
        got = np.stack([RB.view_coords(data["filter_corners"][1], t, proj)[0] for t in trans])
        assert got.dtype == np.float64 and got.shape == want.shape == (6, 5, 8, 3)
        assert np.array_equal(got, want)


def test_nothing_visible_is_none(golden):
    assert bool(golden["invisible_is_none_z"]) and bool(golden["invisible_is_none_canvas"])
    inv = RB.batch(SEED_INVISIBLE, COUNTS, invisible=True)
    for f3d in (True, False):
        assert RB.preprocess(inv, "all-xyz", False, f3d) is None
        assert RB.keeps_of(inv, False, f3d)[1] >= RB.MARGIN


def test_wrong_modes_raise_as_the_reference(golden, data):
    assert bool(golden["owhr_raises"])
    for mode in ("owhr", "xyz"):
        with pytest.raises(NotImplementedError):
            RB.preprocess(data, mode, False, True)
        with pytest.raises(NotImplementedError):
            BI.BoxPreProcess(bbox_mode=mode)


# ---- host-side helpers --------------------------------------------------------------------------------------------------

def test_compose_transforms(data):
    for f3d, key in ((True, "lidar2camera"), (False, "lidar2image")):
        want = RB.transforms_of(data, f3d)
        got = BI.compose_transforms(data[key], data["img_aug_matrix"])
        assert got.dtype == np.float32 and got.shape == (3, 6, 4, 4) and np.array_equal(got, want)
        per_scene = BI.compose_transforms([torch.from_numpy(m) for m in data[key]],
                                          [torch.from_numpy(m) for m in data["img_aug_matrix"]])
        assert np.array_equal(per_scene, want)
        assert np.array_equal(BI.compose_transforms(data[key]), data[key])
    with pytest.raises(ValueError):
        BI.compose_transforms(data["lidar2camera"], data["img_aug_matrix"][:, :3])


def test_camera_param():
    g = torch.Generator().manual_seed(1)
    k, c2l = torch.randn(2, 6, 4, 4, generator=g), torch.randn(2, 6, 4, 4, generator=g)
    want = torch.empty(2, 6, 3, 7)
    want[..., :3], want[..., 3:] = k[..., :3, :3], c2l[..., :3, :]
    got = BI.camera_param(k, c2l)
    assert got.shape == (2, 6, 3, 7) and torch.equal(got, want)
    assert torch.equal(BI.camera_param(list(k), list(c2l)), want)
    assert torch.equal(BI.camera_param(k[:, :, :3, :3].numpy(), c2l.numpy()), want)


def test_aug_text_names():
    names = RB.OBJECT_CLASSES
    classes = torch.tensor([[[3, 0, 3, -1, -1], [8, 8, 8, 8, 8]],
                            [[-1, -1, -1, -1, -1], [9, 1, 0, 5, 1]]])
    got = BI.aug_text_names(classes, names)
    assert got == RB.aug_text(classes.numpy(), names)
    assert got[0] == "car, bus"                     # -1 dropped
    assert got[1] == ""                             # no padding, one class: the class itself is dropped
    assert got[2] == ""
    assert got[3] == "truck, barrier, traffic_cone"   # no padding: `car`, the smallest real class, is lost


def test_aug_text_names_equal_the_reference_captions(golden):
    """The captions the reference's collate function made with `use_aug_text`, an empty template and no tokenizer: per
    (scene, camera) " " + the class sentence, capitalised, + ".".  View 1 of the 70-box scene has no padding (43 boxes, the
    batch maximum), so the reference lost `car` there."""
    classes = torch.from_numpy(golden["allxyz_views_z_classes"])
    got = BI.aug_text_names(classes, RB.OBJECT_CLASSES)
    assert got == RB.aug_text(classes.numpy())
    assert [" " + s.capitalize() + "." for s in got] == golden["aug_captions"].tolist()
    assert (classes[2, 1] >= 0).all() and (classes[2, 1] == 0).any() and not got[2 * 6 + 1].startswith("car")
    assert got[2 * 6].startswith("car, truck") and got[:6] == [""] * 6


def test_camera_param_equals_the_reference(golden):
    want = torch.from_numpy(golden["camera_param"])
    got = BI.camera_param(golden["camera_intrinsics"], golden["camera2lidar"])
    assert got.dtype == want.dtype == torch.float32 and got.shape == (3, 6, 3, 7) and torch.equal(got, want)


class StubBoxes:
    def __init__(self, tensor, box_dim=7, origin=RB.BOTTOM):
        self.tensor, self.box_dim, self.origin = torch.as_tensor(tensor), box_dim, tuple(origin)

    @property
    def corners(self):
        return torch.from_numpy(RB.corners_of(self.tensor.numpy(), self.origin))


def test_reference_corners_on_a_stub_class(data):
    b = StubBoxes(data["boxes"][1])
    pay, flt = BI.reference_corners(b)
    assert torch.equal(pay, torch.from_numpy(data["corners"][1]))
    assert torch.equal(flt, torch.from_numpy(data["filter_corners"][1]))
    assert not torch.equal(pay, flt)


def test_from_config():
    cfg = {"model": {"bbox_mode": "cxyz", "bbox_view_shared": False}, "dataset": {"image_size": [224, 400]}}
    pre = BI.BoxPreProcess.from_config(cfg)
    assert (pre.bbox_mode, pre.view_shared, pre.filter_mode, pre.points) == ("cxyz", False, "positive_z", 4)
    pre = BI.BoxPreProcess.from_config(cfg, use_3d_filter=False)
    assert pre.filter_mode == "canvas" and pre.canvas_size == (224, 400)
    cfg["model"]["bbox_view_shared"] = [False, True]
    assert BI.BoxPreProcess.from_config(cfg, branch=1).filter_mode == "all"
    with pytest.raises(ValueError):
        BI.BoxPreProcess.from_config(cfg)
    with pytest.raises(ValueError):
        BI.BoxPreProcess(use_3d_filter=False)
    with pytest.raises(NotImplementedError):
        BI.BoxPreProcess.from_config({"model": {"bbox_mode": "owhr"}})


# ---- the entry point ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    return _native.load(build_if_missing=False)


def _call(lib, **kw):
    a = dict(corners=P, filter_corners=None, labels=P, offsets=P, transforms=P, total=8, scenes=2, views=6, cap=32,
             points_mode=0, filter_mode=1, canvas_h=224, canvas_w=400, bboxes=P, classes=P, masks=P, counts=P, max_len=P)
    a.update(kw)
    return lib.dd_box_views(a["corners"], a["filter_corners"], a["labels"], a["offsets"], a["transforms"], a["total"],
                            a["scenes"], a["views"], a["cap"], a["points_mode"], a["filter_mode"], a["canvas_h"],
                            a["canvas_w"], a["bboxes"], a["classes"], a["masks"], a["counts"], a["max_len"], None)


BAD_CALLS = [{k: None} for k in ("corners", "labels", "offsets", "bboxes", "classes", "masks", "counts", "max_len")] + [
    {"scenes": 0}, {"scenes": -1}, {"views": 0}, {"views": -2}, {"cap": 0}, {"cap": -32}, {"total": -1},
    {"points_mode": 2}, {"points_mode": -1}, {"filter_mode": 3}, {"filter_mode": -1},
    {"filter_mode": 0, "views": 6}, {"filter_mode": 0, "views": 6, "transforms": None},
    {"filter_mode": 1, "transforms": None}, {"filter_mode": 2, "transforms": None},
    {"filter_mode": 2, "canvas_h": 0}, {"filter_mode": 2, "canvas_w": 0}, {"filter_mode": 2, "canvas_h": -224},
    {"corners": 18}, {"filter_corners": 18}, {"labels": 20}, {"classes": 20}, {"bboxes": 18}, {"max_len": 18},
]


@pytest.mark.parametrize("bad", BAD_CALLS, ids=lambda b: ",".join("%s=%s" % kv for kv in b.items()))
def test_launcher_rejects_before_any_runtime_call(lib, bad):
    """Each bad call answers DD_ERR_BAD_ARG on a machine without a GPU: -3 (DD_ERR_LAUNCH) would mean that the HIP runtime was
    called first."""
    assert _call(lib, **bad) == BAD_ARG


def test_entry_point_is_declared_and_bound(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dualdiff_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+dd_box_views\s*\(([^)]*)\)", hdr)
    assert m is not None
    params = [p.split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert not {"dtype", "in_dtype", "out_dtype"} & set(params)      # fp32 / int64 / uint8 only
    res, args = _native.SIGNATURES["dd_box_views"]
    assert res is ctypes.c_int32 and len(args) == len(params) == 19
    assert hasattr(lib, "dd_box_views") and lib.dd_abi_version() == _native.ABI_VERSION == 4
    from dualdiff_amd import _build
    assert "boxes.hip" in _build.SOURCES and "boxes.hip" not in _build.EXTRA_FLAGS      # no fast-math flag on this file


def test_ops_box_views_checks_its_arguments():
    from dualdiff_amd import ops
    c, l = torch.zeros(4, 8, 3), torch.zeros(4, dtype=torch.int64)
    o, t = torch.tensor([0, 4], dtype=torch.int32), torch.zeros(1, 6, 4, 4)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.box_views(c, l, o, t, 6, 32)
    for bad in (dict(points_mode="owhr"), dict(filter_mode="none"), dict(filter_mode="all"), dict(cap=0),
                dict(filter_mode="canvas"), dict(filter_mode="canvas", canvas_size=(0, 400)), dict(transforms=None),
                dict(corners=c.double()), dict(labels=l.int()), dict(offsets=o.long()), dict(filter_corners=c[:2])):
        kw = dict(corners=c, labels=l, offsets=o, transforms=t, views=6, cap=32)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.box_views(**kw)
