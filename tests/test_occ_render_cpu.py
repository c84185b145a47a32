"""ORS panorama without a GPU: the restatement against the fixture minted from the reference's own lines, the
conditions the fixture must keep, the launchers' argument validation and the host side of `OccRender`."""
import ctypes
import os

import numpy as np
import pytest
import torch

from dualdiff_amd import _build, _native
from tests import occ_render_reference as R
from tests.golden import cases as C

GOLD = os.path.join(os.path.dirname(__file__), "golden", "occ_render.npz")
BAD_ARG = -1
P = 16                                                   # non-null, 16-byte aligned, never dereferenced
PALETTE = (ctypes.c_uint8 * 54)(*R.PALETTE.reshape(-1).tolist())
# the share of rays with a hit per mode, measured with the oracle when the fixture was minted
HIT_SHARE = {"all": 0.543, "bg": 0.477, "fg": 0.164}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def restated():
    occ, Ks, Rts = C.ors_inputs()
    return {m: R.render(occ, Ks, Rts, C.ORS_H, C.ORS_W, C.ORS_RATIO, C.ORS_S, 0.2, m) for m in R.MODES}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_build.lib_path()):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _native.load(build_if_missing=False)


@pytest.mark.parametrize("mode", R.MODES)
def test_restatement_equals_the_reference_lines(gold, restated, mode):
    cls, pan, _ = restated[mode]
    assert cls.shape == (6, C.ORS_H, C.ORS_W) and pan.shape == (C.ORS_H, 6 * C.ORS_W, 3)
    assert np.array_equal(cls, gold["classes_" + mode])
    assert np.array_equal(pan, gold["frames_" + mode])
    cam = R.camera_panorama(R.camera_pictures())
    assert np.array_equal(R.overlay(pan, cam), gold["overlay_" + mode])


def test_palette_is_one_table():
    from dualdiff_amd.pipeline.occ_render import OCC_COLORS
    assert np.array_equal(np.asarray(OCC_COLORS, dtype=np.uint8), R.PALETTE)


def test_fixture_keeps_its_conditions(gold, restated):
    for mode in R.MODES:
        share = float((gold["classes_" + mode] != 17).mean())
        print(mode, "hit share", share)
        assert 0.1 <= share <= 0.9
        assert abs(share - HIT_SHARE[mode]) < 0.0005
    cls, _, idx = restated["all"]
    seen = set(np.unique(cls[cls != 17]).tolist())
    assert len(seen) >= 12 and 0 in seen
    depth = idx[cls != 17]
    shares = [float((depth >= k).sum()) / cls.size for k in (64, 128, 256)]
    print("hits at >= 64 / 128 / 256:", shares, "deepest", int(depth.max()))
    assert all(s > 0 for s in shares)
    assert [round(s, 3) for s in shares] == [0.131, 0.039, 0.001] and int(depth.max()) == 261
    # class 0 decides: "all" paints it black and hides what is behind, "bg" looks through it
    assert ((gold["classes_all"] == 0) & (gold["classes_bg"] != 0)).any()
    assert not (gold["classes_bg"] <= 10).any() and not ((gold["classes_fg"] >= 11) & (gold["classes_fg"] != 17)).any()


def test_all_17_ray_follows_the_argmax_rule():
    lab = torch.full((1, 1, 2, 8), 17)
    lab[0, 0, 1, 5], lab[0, 0, 1, 6] = 4, 12
    cls, idx = R.first_hit(lab, "all")
    assert cls.tolist() == [[[17, 4]]] and idx.tolist() == [[[0, 5]]]
    assert R.first_hit(lab, "bg")[0].tolist() == [[[17, 12]]]
    assert R.first_hit(lab, "fg")[0].tolist() == [[[17, 4]]]


def first_hit_args(**kw):
    a = dict(occ=P, origin=P, dir=P, rig=P, cls=P, frames=P, visited=None, palette=PALETTE, b=1, rigs=1, n=2, h=3, w=5,
             samples=8, step=0.2, mode=1, exits=3)
    a.update(kw)
    return tuple(a[k] for k in ("occ", "origin", "dir", "rig", "cls", "frames", "visited", "palette", "b", "rigs", "n", "h",
                                "w", "samples", "step", "mode", "exits")) + (None,)


@pytest.mark.parametrize("bad", [dict(occ=None), dict(origin=None), dict(dir=None), dict(rig=None), dict(palette=None),
                                 dict(cls=None, frames=None), dict(b=0), dict(b=-1), dict(rigs=0), dict(n=0), dict(h=0),
                                 dict(w=-3), dict(samples=0), dict(mode=3), dict(mode=-1), dict(exits=4), dict(step=0.0),
                                 dict(step=-0.2)], ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_first_hit_launcher_rejects_bad_arguments(lib, bad):
    """the bad-argument code, not the launch-failure code: validation comes before any HIP runtime call"""
    assert lib.dd_ors_first_hit(*first_hit_args(**bad)) == BAD_ARG


@pytest.mark.parametrize("bad", [dict(colour=None), dict(camera=None), dict(out=None), dict(parts=None), dict(flags=None),
                                 dict(b=0), dict(h=0), dict(w=-1)], ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_overlay_launcher_rejects_bad_arguments(lib, bad):
    a = dict(colour=P, camera=P, out=P, parts=P, flags=P, b=1, h=4, w=12)
    a.update(bad)
    assert lib.dd_ors_overlay_u8(*(a[k] for k in ("colour", "camera", "out", "parts", "flags", "b", "h", "w")), None) == BAD_ARG


def test_abi_has_both_entry_points_and_no_dtype_parameter(lib):
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "dualdiff_hip.h")).read(), flags=re.S)
    for name in ("dd_ors_first_hit", "dd_ors_overlay_u8"):
        assert name in _native.SIGNATURES and hasattr(lib, name)
        decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, hdr)
        assert decl is not None and "dtype" not in decl.group(1)
    assert "ors_render.hip" in _build.SOURCES
    assert lib.dd_abi_version() == 4


def test_for_image_size_gives_the_four_geometries():
    from dualdiff_amd.pipeline.occ_render import OccRender
    for size, shape, ratio, view in (([224, 400], (896, 1600), 400 / 1600, (224, 400)),
                                     ([192, 384], (896, 1600), 400 / 1600, (224, 400)),
                                     ([432, 768], (900, 1600), 768 / 1600, (432, 768)),
                                     ([256, 704], (900, 1600), 768 / 1600, (432, 768))):
        r = OccRender.for_image_size(size)
        assert r.projector.image_shape == shape and r.projector.compress_ratio == ratio and r.view_hw == view
        assert r.projector.sample_point == 320 and r.projector.sample_step == 0.2 and r.mode == "bg"
    assert OccRender.for_image_size((224, 400), mode="all", sample_point=200).projector.sample_point == 200


def test_occ_render_refuses_what_it_does_not_build():
    from dualdiff_amd.pipeline.occ_render import OccRender
    with pytest.raises(ValueError, match=r"image_size \[128, 256\]"):
        OccRender.for_image_size([128, 256])
    with pytest.raises(ValueError, match="mode must be one of all, bg, fg"):
        OccRender((896, 1600), 0.25, mode="background")
    with pytest.raises(ValueError, match="palette must be 18"):
        OccRender((896, 1600), 0.25, palette=[(0, 0, 0)] * 17)
    with pytest.raises(ValueError, match="palette must be 18"):
        OccRender((896, 1600), 0.25, palette=[(0, 0, 256)] * 18)
    with pytest.raises(ValueError, match="sample_point"):
        OccRender((896, 1600), 0.25, sample_point=0)
    with pytest.raises(ValueError, match="sample_step"):
        OccRender((896, 1600), 0.25, sample_step=0.0)
    with pytest.raises(ValueError, match="leaves no pixel"):
        OccRender((896, 1600), 1e-4)


def test_ops_refuse_cpu_tensors_and_wrong_types():
    from dualdiff_amd import ops as O
    if not os.path.exists(_build.lib_path()):
        pytest.skip("library not built")
    occ = torch.zeros((1, 200, 200, 16), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU only"):
        O.ors_first_hit(occ, torch.zeros(1, 1, 3), torch.zeros(1, 1, 4, 3), [0], (2, 2), 8, palette=R.PALETTE)
    with pytest.raises(TypeError, match="camera must be uint8"):
        O.ors_overlay(torch.zeros((1, 2, 2, 3), dtype=torch.uint8), torch.zeros((1, 2, 2, 3)))
    with pytest.raises(RuntimeError, match="GPU only"):
        O.ors_overlay(torch.zeros((1, 2, 2, 3), dtype=torch.uint8), torch.zeros((1, 2, 2, 3), dtype=torch.uint8))
