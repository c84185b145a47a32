"""The resized ORS condition (`crop_drivewm`, image_size [192, 384]) without a GPU: the numpy restatement that defines the
feature's arithmetic (tests/occ_condition_reference.py) against the reference's torch calls within a derived bound, the
mistakes such a restatement could make planted with torch and shown to pass that bound, the host tables the kernel reads
against the restatement's, and the argument handling of the Python layer and of the built library.

The bound.  torch's own result is not defined to the bit: at the reference's geometry its CPU kernel with one intra-op
thread and with several differ in the last place in a third of the elements.  Both sides use the same weights; every
intermediate is a convex combination of values in [0, 1]; one evaluation rounds at most five times (two products and a
sum per row pair, a product and a sum for the rows), each by at most 2^-25 for a value up to 1, so two evaluations differ
by at most 10 * 2^-25 = 3e-7, and 2^-21 = 4.8e-7 leaves room for an intermediate that rounds to just above 1.  Measured:
1.8e-7 at most; 0 against torch's multi-threaded kernel at the reference's geometry."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import occ_condition_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [R.geometry_id(g) for g in R.GEOMETRIES]


def _args(g):
    return dict(views=g[0], pad_top=g[3], resize=g[4], top=g[5], left=g[6], size=g[7])


_CACHE = {}


def _case(g):
    """(frames, restatement) of a geometry, computed once and not written to afterwards"""
    if g not in _CACHE:
        frames = R.random_frames(g, 1 if g == R.TRUE else 2, seed=192 + R.GEOMETRIES.index(g))
        want = R.restatement(frames, **_args(g))
        frames.setflags(write=False)
        want.setflags(write=False)
        _CACHE[g] = (frames, want)
    return _CACHE[g]


def _with_threads(n, fn):
    before = torch.get_num_threads()
    try:
        if n is not None:
            torch.set_num_threads(n)
        return fn()
    finally:
        torch.set_num_threads(before)


@pytest.mark.parametrize("g", R.GEOMETRIES, ids=IDS)
def test_restatement_equals_torch_within_the_bound(g):
    frames, mine = _case(g)
    assert mine.dtype == np.float32 and mine.shape == (frames.shape[0], 3, g[7][0], g[0] * g[7][1])
    assert R.BOUND == 2.0 ** -21
    for threads in (1, None):                                # torch takes different kernels for the two
        ref = _with_threads(threads, lambda: R.torch_crop_drivewm(frames, **_args(g)))
        d = float(np.abs(mine.astype(np.float64) - ref.astype(np.float64)).max())
        print("%s threads %s: max |restatement - torch| = %.3g, %d of %d elements differ"
              % (R.geometry_id(g), threads or "default", d, int((mine != ref).sum()), mine.size))
        assert d <= R.BOUND
        if g == R.IDENTITY:
            assert np.array_equal(mine, ref)
    if g == R.IDENTITY:                                      # ... and is ToTensor of the cropped bytes
        x = frames[:, 1:4, 1:4].astype(np.float32) / np.float32(255)
        assert np.array_equal(mine, x.transpose(0, 3, 1, 2))


def _downscales(g):
    return g[4][0] < g[1] + g[3] and g[4][1] < g[2]


def _fault_changes_something(g, fault):
    """Whether the planted mistake is a different computation at this geometry at all — from the geometry alone."""
    views, h, w, pad, (rh, rw), top, left, (oh, ow) = g
    identity = (rh, rw) == (h + pad, w)
    return {"whole_panorama": views > 1 and not identity,    # one resize over all the views
            "pad_bottom": pad > 0,
            "align_corners": not identity,
            "antialias": rh < h + pad or rw < w,             # the antialias filter widens only when the size shrinks
            "crop_bottom": top > 0}[fault]                   # the rows kept counted from the wrong end


@pytest.mark.parametrize("fault", R.FAULTS)
@pytest.mark.parametrize("g", R.GEOMETRIES, ids=IDS)
def test_planted_faults_exceed_the_bound(g, fault):
    frames, mine = _case(g)
    bad = R.torch_crop_drivewm(frames, fault=fault, **_args(g))
    over = np.abs(mine.astype(np.float64) - bad.astype(np.float64)) > R.BOUND
    print("%s %s: %.1f %% of the elements beyond the bound" % (R.geometry_id(g), fault, 100 * over.mean()))
    if not _fault_changes_something(g, fault):
        assert not over.any()                                # the same computation: within the bound
        return
    assert over.any()
    # the whole-panorama resize at 3 x 9 x 16 moves the coordinates of few columns: held to "somewhere" only
    if _downscales(g) and not (fault == "whole_panorama" and g[:3] == (3, 9, 16)):
        assert over.mean() > 0.10


def test_unfused_coordinate_is_another_result():
    """scale * (dst + 0.5) - 0.5 with the product rounded first is not the definition: it shows at the true geometry."""
    f32 = np.float32
    for n_in, n_out in ((225, 216), (400, 384)):
        scale = f32(n_in) / f32(n_out)
        dst = np.arange(n_out, dtype=f32) + f32(0.5)
        unfused = ((scale * dst).astype(f32) - f32(0.5)).astype(f32)
        fused = R.fma32(np.full(n_out, scale, dtype=f32), dst, np.full(n_out, -0.5, dtype=f32))
        assert (unfused != fused).any()
    # fma32 rounds once: a product that float32 cannot hold, cancelled against its own rounding
    a = f32(1 + 2.0 ** -12)
    assert R.fma32(a, a, -(a * a).astype(f32))[()] == f32(2.0 ** -24)
    # ... also where float64 rounds the exact sum (1 + 2^-23) + 2^-24 - 2^-70 up to float32's tie, which would go to even
    a, b, c = f32(2.0 ** -24 * (1 + 2.0 ** -23)), f32(1 - 2.0 ** -23), f32(1 + 2.0 ** -23)
    assert float(a) * float(b) + float(c) == 1 + 2.0 ** -23 + 2.0 ** -24
    assert R.fma32(a, b, c)[()] == c


@pytest.mark.parametrize("pair", [(225, 216), (400, 384), (10, 8), (16, 14), (5, 7), (7, 9), (29, 27), (50, 48), (5, 5), (1, 3),
                                  (3, 1), (4608, 384)])
def test_host_tables_equal_the_restatement(pair):
    from dualdiff_amd import image_tables
    taps, weights = image_tables.bilinear_tables(*pair)
    assert taps.dtype == torch.int32 and weights.dtype == torch.float32
    assert tuple(taps.shape) == tuple(weights.shape) == (pair[1], 2)
    i0, i1, l0, l1 = R.axis_tables(*pair)
    assert np.array_equal(taps.numpy(), np.stack([i0, i1], axis=1))
    assert np.array_equal(weights.numpy().view(np.int32), np.stack([l0, l1], axis=1).view(np.int32))
    assert int(taps.min()) >= 0 and int(taps.max()) <= pair[0] - 1
    assert image_tables.bilinear_tables(*pair)[0] is taps                         # cached
    if pair[0] == pair[1]:
        assert torch.equal(weights, torch.tensor([[1.0, 0.0]]).expand(pair[1], 2))
        assert taps[:, 0].tolist() == list(range(pair[0]))


def test_host_table_arguments():
    from dualdiff_amd import image_tables
    for pair in ((0, 4), (4, 0), (-1, 4), (image_tables.BILINEAR_MAX + 1, 4), (4, image_tables.BILINEAR_MAX + 1)):
        with pytest.raises(ValueError):
            image_tables.bilinear_tables(*pair)
    taps, weights = image_tables.device_bilinear_tables(9, 4, "cpu")               # under the one rule of _consts
    assert image_tables.device_bilinear_tables(9, 4, "cpu")[0] is taps
    assert torch.equal(taps, image_tables.bilinear_tables(9, 4)[0]) and torch.equal(weights, image_tables.bilinear_tables(9, 4)[1])


# ---- host logic ---------------------------------------------------------------------------------------------------------------

def _cfg(size):
    return SimpleNamespace(dataset=SimpleNamespace(image_size=size))


def test_occ_condition_from_config():
    from dualdiff_amd.pipeline import png_input as PI
    for size in ([224, 400], [432, 768]):
        occ = PI.occ_condition_from_config(_cfg(size))
        assert type(occ) is PI.OccCondition and (occ.views, occ.in_hw, occ.out_hw) == (6, None, None)
    occ = PI.occ_condition_from_config({"dataset": {"image_size": [256, 704]}})
    assert type(occ) is PI.OccCondition and occ.crop(432, 4608) == (176, 32, 256, 704)
    for cfg in (_cfg([192, 384]), {"dataset": {"image_size": (192, 384)}}):
        occ = PI.occ_condition_from_config(cfg)
        assert type(occ) is PI.ResizedOccCondition
        assert (occ.views, occ.in_hw, occ.pad_top, occ.resize_hw, occ.out_hw) == (6, (224, 400), 1, (216, 384), (192, 384))
        assert occ.crop(224, 2400) == (24, 0, 192, 384) == R.TRUE[5:7] + R.TRUE[7]
    with pytest.raises(ValueError, match="image_size"):
        PI.occ_condition_from_config(_cfg([128, 256]))
    with pytest.raises(NotImplementedError, match="crop_drivewm") as e:            # OccCondition itself has no resize
        PI.OccCondition.from_config(_cfg([192, 384]))
    assert "occ_condition_from_config" in str(e.value)


def test_resized_occ_condition_arguments():
    from dualdiff_amd.pipeline import png_input as PI
    good = dict(views=6, in_hw=(224, 400), pad_top=1, resize_hw=(216, 384), out_hw=(192, 384))
    d = PI.ResizedOccCondition.drivewm()
    assert {k: getattr(d, k) for k in good} == good == {k: getattr(PI.ResizedOccCondition(**good), k) for k in good}
    with pytest.raises(ValueError, match="antialias"):
        PI.ResizedOccCondition(antialias=True, **good)
    assert PI.ResizedOccCondition(antialias=False, **good).resize_hw == (216, 384)
    for kw in ({"views": 0}, {"views": 2.0}, {"views": True}, {"pad_top": -1}, {"pad_top": 1.5}, {"in_hw": None}, {"resize_hw": None},
               {"out_hw": None}, {"in_hw": 224}, {"in_hw": (0, 400)}, {"resize_hw": (216, 0)}, {"out_hw": (217, 384)},
               {"out_hw": (192, 385)}, {"out_hw": (192, 383)}, {"out_hw": (0, 384)}):
        with pytest.raises(ValueError):
            PI.ResizedOccCondition(**{**good, **kw})
    # hd_crop: the rows dropped on top, the columns dropped on both sides
    occ = PI.ResizedOccCondition(views=3, in_hw=(9, 16), pad_top=1, resize_hw=(8, 14), out_hw=(5, 10))
    assert occ.crop(9, 48) == (3, 2, 5, 10)
    with pytest.raises(ValueError, match="defined for 9 x 3 x 16"):
        occ.crop(9, 96)
    with pytest.raises(ValueError, match="3 divides"):
        occ.crop(9, 49)
    with pytest.raises(ValueError, match="flat list"):
        occ(torch.zeros(1, 2, 9, 48, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="GPU only"):
        occ(torch.zeros(2, 9, 48, 3, dtype=torch.uint8))


def test_op_arguments():
    from dualdiff_amd import ops
    frames = torch.zeros(2, 9, 48, 3, dtype=torch.uint8)
    good = dict(frames=frames, views=3, pad_top=1, resize=(8, 14), top=2, left=1, size=(5, 11), out=None)

    def call(**kw):
        a = {**good, **kw}
        return ops.png_condition_resized(a.pop("frames"), **a)
    with pytest.raises(RuntimeError, match="GPU only"):
        call()
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.png_condition_resized(frames, views=3)                               # every default
    for kw in ({"views": 5}, {"views": 0}, {"views": 3.0}, {"pad_top": -1}, {"pad_top": 1.0}, {"top": -1}, {"left": -1},
               {"top": 4}, {"left": 4}, {"size": (0, 11)}, {"size": 11}, {"resize": 8}, {"resize": (0, 14)}, {"resize": (8, 1 << 15)},
               {"resize": None, "size": (11, 11)}, {"frames": frames.float()}, {"frames": frames[..., :2]},
               {"frames": frames[:, :, ::2]}, {"out": torch.zeros(2, 3, 5, 33, dtype=torch.float16)},
               {"out": torch.zeros(2, 3, 5, 32)}, {"out": torch.zeros(2, 3, 5, 66)[..., ::2]}):
        with pytest.raises(ValueError):
            call(**kw)


def test_the_sources_name_the_kernel():
    from dualdiff_amd import _build, _native
    hip = open(os.path.join(ROOT, "dualdiff_amd", "csrc", "png_decode.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "dualdiff_hip.h")).read()
    assert "png_decode.hip" in _build.SOURCES and 'extern "C" int dd_png_condition_resize(' in hip
    assert "int dd_png_condition_resize(" in hdr and "dataset/utils.py:355-358" in hdr and "define DD_ABI_VERSION 4" in hdr
    assert "dd_png_condition_resize" in _native.SIGNATURES and _native.ABI_VERSION == 4
    body = hip[hip.index("float dd_pngc_sample("):hip.index("void dd_png_condition_resize_kernel(")]
    assert body.count("__fmaf_rn(") == 3 and body.count("__fmul_rn(") == 3         # the combination is spelled out


def test_library_turns_down_bad_calls_without_a_gpu():
    """DD_ERR_BAD_ARG before any runtime call, so also on a machine without a GPU."""
    from dualdiff_amd import _build, _native
    if not os.path.exists(_build.lib_path()):
        pytest.skip("library not built (run __graft_entry__.build())")
    lib = _native.load(build_if_missing=False)
    P = ctypes.c_void_p(4096)

    def call(frames=P, out=P, lut=P, row_taps=P, row_weights=P, col_taps=P, col_weights=P, b=2, h=9, w=48, views=3, pad_top=1,
             rh=8, rw=14, top=2, left=1, oh=5, ow=11):
        return lib.dd_png_condition_resize(frames, out, lut, row_taps, row_weights, col_taps, col_weights, b, h, w, views,
                                           pad_top, rh, rw, top, left, oh, ow, None)
    for name in ("frames", "out", "lut", "row_taps", "row_weights", "col_taps", "col_weights"):
        assert call(**{name: None}) == -1, name
    for kw in ({"b": 0}, {"h": 0}, {"w": 0}, {"views": 0}, {"views": 5}, {"pad_top": -1}, {"rh": 0}, {"rw": 0}, {"top": -1},
               {"left": -1}, {"oh": 0}, {"ow": 0}, {"top": 4}, {"left": 4}, {"oh": 7}, {"ow": 14},
               {"out": ctypes.c_void_p(4100)}, {"out": ctypes.c_void_p(4104)}, {"lut": ctypes.c_void_p(4098)},
               {"row_taps": ctypes.c_void_p(4097)}, {"row_weights": ctypes.c_void_p(4098)}, {"col_taps": ctypes.c_void_p(4099)},
               {"col_weights": ctypes.c_void_p(4097)}):
        assert call(**kw) == -1, kw
    assert call(h=40000, w=39999, views=3) == -2                                  # positions inside a frame are 32-bit
