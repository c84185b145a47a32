"""Attention-map pictures without a GPU: the table look-up the kernel implements against the restatement's per-pixel
`cmap(...)` loop (tests/attn_output_reference.py), the committed colour table against matplotlib, `sheet_layout` against
view_images' arithmetic, and the bad-argument answers of the wrappers and of the two entry points (decided before any
runtime call: DD_ERR_LAUNCH on a machine without a GPU would mean a check came after one)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dualdiff_amd import _build, _native, image_tables, ops
from dualdiff_amd.pipeline import attn_output as AO
from tests import attn_output_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED = -1, -2
P = 16                                                   # non-null, aligned, never dereferenced


def has_matplotlib():
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return False
    return True


needs_matplotlib = pytest.mark.skipif(not has_matplotlib(), reason="matplotlib is not installed: nothing to compare with")


# ---- the colouring -----------------------------------------------------------------------------------------------------

def tiny_columns(hw=(4, 5)):
    """(h * w, 5) float32: softmax-like data, a constant column, the exact k / 256 edges, the edges' upper end, X = 1 twice."""
    q = hw[0] * hw[1]
    rng = np.random.RandomState(3)
    logits = rng.randn(q, 7).astype(np.float32) * 4
    soft = np.exp(logits) / np.exp(logits).sum(1, keepdims=True)
    edges = np.arange(q, dtype=np.float32) * np.float32(13) % 257 / np.float32(256)      # k / 256, k in 0..256, 0 and 1 first
    edges[0], edges[1] = 0.0, 1.0
    top = (np.float32(256) - np.arange(q, dtype=np.float32)) / np.float32(256)
    top[-1] = 0.0
    return np.stack([soft[:, 0], np.full(q, 0.25, np.float32), edges, top, soft[:, 1]], axis=1).astype(np.float32)


@needs_matplotlib
def test_table_lookup_equals_the_cmap_loop():
    hw = (4, 5)
    cols = tiny_columns(hw)
    for j in range(cols.shape[1]):
        x = R.normalise(cols[:, j], hw)
        loop = R.colour_loop(x)
        assert np.array_equal(R.colour_by_table(x, image_tables.COOLWARM_U8), loop), j
        assert np.array_equal(R.colour(x), loop), j
    const = R.colour_loop(R.normalise(cols[:, 1], hw))
    assert np.isnan(R.normalise(cols[:, 1], hw)).all() and not const.any()           # 0 / 0: black everywhere
    x = R.normalise(cols[:, 2], hw)[:, :, 0].ravel()
    assert x[0] == 0.0 and x[1] == 1.0 and set((x * 256).tolist()) <= set(range(257))  # every value sits on a bin edge
    got = R.colour_by_table(R.normalise(cols[:, 2], hw), image_tables.COOLWARM_U8).reshape(-1, 3)
    assert tuple(got[0]) == image_tables.COOLWARM_U8[0] and tuple(got[1]) == image_tables.COOLWARM_U8[255]


@needs_matplotlib
def test_committed_table_is_matplotlibs_coolwarm():
    want = (R.colormap("coolwarm")(np.arange(256))[:, :3] * 255).astype(np.uint8)
    assert np.array_equal(np.asarray(image_tables.COOLWARM_U8, dtype=np.uint8), want)


def test_table_constants_and_float_hand_off():
    t = image_tables.COOLWARM_U8
    assert len(t) == 256 and t[0] == (58, 76, 192) and t[128] == (221, 220, 219) and t[255] == (179, 3, 38)
    tab = image_tables.cmap_table("coolwarm")
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (257, 4)
    assert not tab[256].any() and not tab[:, 3].any()
    # the quantiser of dd_image_resample_u8 is rint(x * 255): the quotient gives the byte back, for every byte
    b = np.arange(256, dtype=np.float32)
    assert np.array_equal(np.rint(b / np.float32(255) * np.float32(255)), b)
    assert np.array_equal(np.rint(tab[:256, :3].numpy() * np.float32(255)).astype(np.uint8), np.asarray(t, dtype=np.uint8))
    own = np.arange(768, dtype=np.int64).reshape(256, 3) % 256
    assert image_tables.cmap_bytes(own.astype(np.uint8))[1] == (3, 4, 5)
    assert image_tables.cmap_bytes(torch.from_numpy(own.astype(np.uint8)))[255] == tuple(int(v) for v in own[255])
    for bad in ("viridis", own[:255].astype(np.uint8), own.astype(np.float32), own[:, :2].astype(np.uint8), 7):
        with pytest.raises(ValueError):
            image_tables.cmap_bytes(bad)


# ---- the layout --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("num_rows", [1, 4])
def test_sheet_layout_is_view_images_arithmetic(num_rows):
    for n in range(1, 21):
        num_empty, num_items, num_cols = R.layout(n, num_rows)
        if num_cols == 0:                                # n = 1 on 4 rows: 2 // 4 == 0, the reference's canvas is empty
            with pytest.raises(ValueError, match="no column"):
                AO.sheet_layout(n, num_rows)
            continue
        rows, cols, index = AO.sheet_layout(n, num_rows)
        assert (rows, cols) == (num_rows, num_cols) and len(index) == rows * cols
        images = list(range(n)) + [-1] * num_empty       # the reference's list: the tiles, then the empty ones
        assert index == [images[r * cols + c] for r in range(rows) for c in range(cols)]
    assert AO.sheet_layout(5, 4) == (4, 1, [0, 1, 2, 3])                              # the fifth tile is lost
    assert AO.sheet_layout(7, 4) == (4, 2, [0, 1, 2, 3, 4, 5, 6, -1])
    assert AO.sheet_layout(3, 4) == (4, 1, [0, 1, 2, -1])
    for bad in (0, -1):
        with pytest.raises(ValueError):
            AO.sheet_layout(bad, 4)
    with pytest.raises(ValueError):
        AO.sheet_layout(4, 0)


def test_sheet_restatement_drops_and_pads_as_the_layout_says():
    tiles = (np.arange(5, dtype=np.uint8)[:, None, None, None] + np.zeros((5, 10, 6, 3), dtype=np.uint8))
    sheet = R.view_images(tiles, num_rows=4)
    assert sheet.shape == (40, 6, 3) and [int(sheet[10 * r, 0, 0]) for r in range(4)] == [0, 1, 2, 3]
    sheet = R.view_images(tiles[:3], num_rows=4)
    assert [int(sheet[10 * r, 0, 0]) for r in range(4)] == [0, 1, 2, 255]
    sheet = R.view_images(np.zeros((2, 100, 6, 3), dtype=np.uint8), num_rows=1)        # offset = int(100 * 0.02) = 2
    assert sheet.shape == (100, 14, 3) and (sheet[:, 6:8] == 255).all() and not sheet[:, :6].any()


# ---- the module's host side ---------------------------------------------------------------------------------------------

def test_render_sizes_and_labels():
    r = AO.AttnMapRender()
    assert r.strip == 44 and r.gap(224 + 44) == 5 and r.gap(224) == 4
    strip = AO.draw_label("car", 44, 400)
    assert strip.shape == (44, 400, 3) and strip.dtype == np.uint8
    assert (strip == 255).any() and (strip != 255).any()
    ys, xs = np.nonzero((strip != 255).any(axis=2))
    assert abs((xs.min() + xs.max() + 1) / 2 - 200) <= 1                              # centred along the strip
    assert AO.draw_label("car", 44, 400) is strip                                     # drawn once
    with pytest.raises(ValueError):
        AO.AttnMapRender(cmap="viridis")
    with pytest.raises(ValueError):
        AO.AttnMapRender(hw=(0, 50))


def test_render_rejects_bad_arguments_without_a_gpu():
    r = AO.AttnMapRender(hw=(4, 5), size=(8, 10))
    maps = torch.zeros((2, 20, 9))
    with pytest.raises(ValueError, match="maps must be"):
        r.tiles(torch.zeros((2, 21, 9)), [1])
    with pytest.raises(ValueError, match="float32"):
        r.tiles(maps.double(), [1])
    with pytest.raises(ValueError, match="cols must be"):
        r.tiles(maps, [9])
    with pytest.raises(ValueError, match="cols must be"):
        r.tiles(maps, [])
    with pytest.raises(ValueError, match="n_text"):
        r.text_sheets(maps, 0)
    with pytest.raises(ValueError, match="n_text"):
        r.text_sheets(maps, 9)
    with pytest.raises(ValueError, match="labels must be"):
        r.text_sheets(maps, 3, labels=["a", "b"])
    with pytest.raises(ValueError, match="label strips"):
        r.text_sheets(maps, 3, labels=torch.zeros((3, 2, 10, 3), dtype=torch.uint8))
    assert r.box_sheets(maps, first=9) is None                                        # no box column: nothing to draw
    with pytest.raises(RuntimeError, match="GPU only"):                               # valid: there is no CPU fallback
        r.tiles(maps, [1, 2])


def test_ops_validate_without_a_gpu():
    maps, cols, tab = torch.zeros((2, 20, 9)), torch.tensor([1, 2], dtype=torch.int32), image_tables.cmap_table("coolwarm")
    for kw in (dict(maps=maps[:, :19]), dict(maps=maps.double()), dict(maps=maps.transpose(1, 2).contiguous().transpose(1, 2)),
               dict(cols=cols.long()), dict(cols=cols[:0]), dict(table=tab[:256]), dict(table=tab.double()), dict(hw=(4, 0)),
               dict(hw=4), dict(out=torch.zeros((4, 3, 4, 4)))):
        a = dict(maps=maps, cols=cols, table=tab, hw=(4, 5))
        a.update(kw)
        with pytest.raises(ValueError):
            ops.attn_heat(a["maps"], a["cols"], a["table"], a["hw"], out=a.get("out"))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.attn_heat(maps, cols, tab, (4, 5))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.attn_heat(torch.zeros((2, 20, 12))[:, :, :9], cols, tab, (4, 5))          # a padded pitch is inside the contract
    tiles, index = torch.zeros((4, 6, 5, 3), dtype=torch.uint8), torch.zeros((2, 2), dtype=torch.int32)
    lab = torch.zeros((4, 2, 5, 3), dtype=torch.uint8)
    for kw in (dict(tiles=tiles.float()), dict(tiles=tiles[..., :2]), dict(index=index.long()), dict(index=index[:, :1]),
               dict(rows=0), dict(cols=True), dict(gap=-1), dict(labels=lab[:3]), dict(labels=lab[:, :, :4]),
               dict(labels=torch.zeros((4, 7, 5, 3), dtype=torch.uint8)), dict(tiles=tiles.transpose(1, 2)),
               dict(out=torch.zeros((2, 6, 10, 3), dtype=torch.uint8))):
        a = dict(tiles=tiles, index=index, rows=1, cols=2, gap=1, labels=lab)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.attn_sheet_u8(a["tiles"], a["index"], a["rows"], a["cols"], a["gap"], a["labels"], out=a.get("out"))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.attn_sheet_u8(tiles, index, 1, 2, 1, lab)


# ---- the launchers' validation, without a GPU ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_build.lib_path()):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _native.load(build_if_missing=False)


def heat_args(**kw):
    a = dict(maps=P, cols=P, table=P, img=P, views=6, h=28, w=50, n=106, t=79, ldm=108, vs=1400 * 108)
    a.update(kw)
    return tuple(a[k] for k in ("maps", "cols", "table", "img", "views", "h", "w", "n", "t", "ldm", "vs")) + (None,)


def sheet_args(**kw):
    a = dict(tiles=P, index=P, labels=P, out=1, m=474, sheets=6, rows=4, cols=20, th=268, tw=400, lh=44, gap=5)
    a.update(kw)
    return tuple(a[k] for k in ("tiles", "index", "labels", "out", "m", "sheets", "rows", "cols", "th", "tw", "lh",
                                "gap")) + (None,)


HEAT_BAD = [dict(maps=None), dict(cols=None), dict(table=None), dict(img=None), dict(views=0), dict(h=0), dict(w=-50),
            dict(n=0), dict(t=0), dict(ldm=105), dict(vs=-1), dict(maps=18), dict(cols=17), dict(table=19), dict(img=2),
            dict(ldm=105, views=65535)]
HEAT_UNSUPPORTED = [dict(views=830), dict(views=65535, t=2), dict(h=1 << 16, w=1 << 15), dict(h=1 << 30, w=1 << 30)]
SHEET_BAD = [dict(tiles=None), dict(index=None), dict(out=None), dict(m=0), dict(sheets=0), dict(rows=0), dict(cols=-1),
             dict(th=0), dict(tw=0), dict(lh=-1), dict(gap=-1), dict(labels=None), dict(lh=0), dict(lh=269), dict(index=18),
             dict(index=18, sheets=65536)]
SHEET_UNSUPPORTED = [dict(sheets=65536), dict(rows=1 << 12, cols=1 << 12), dict(th=1 << 20, lh=0, labels=None, tw=1 << 12),
                     dict(rows=1, cols=1, th=8, tw=8, lh=0, labels=None, gap=(1 << 31) - 1)]


def test_launchers_validate_before_any_launch(lib):
    for kw in HEAT_BAD:
        assert lib.dd_attn_heat(*heat_args(**kw)) == BAD_ARG, kw
    for kw in HEAT_UNSUPPORTED:
        assert lib.dd_attn_heat(*heat_args(**kw)) == UNSUPPORTED, kw
    for kw in SHEET_BAD:
        assert lib.dd_attn_sheet_u8(*sheet_args(**kw)) == BAD_ARG, kw
    for kw in SHEET_UNSUPPORTED:
        assert lib.dd_attn_sheet_u8(*sheet_args(**kw)) == UNSUPPORTED, kw


def test_header_declares_and_cites():
    src = open(os.path.join(ROOT, "include", "dualdiff_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+dd_attn_heat\s*\(", code) and re.search(r"\bint\s+dd_attn_sheet_u8\s*\(", code)
    assert "#define DD_ABI_VERSION 4" in code
    comment = src[:src.index("int dd_attn_heat(")].rsplit("/*", 1)[1]
    for cite in ("tools/explore_attn.py:114-151", ":25-53", ":13-23", "DD_ERR_BAD_ARG", "DD_ERR_UNSUPPORTED"):
        assert cite in comment, cite


def test_abi_version_binding_and_build_flags(lib):
    assert lib.dd_abi_version() == _native.ABI_VERSION == 4
    res, args = _native.SIGNATURES["dd_attn_heat"]
    assert res is ctypes.c_int32 and len(args) == 12 and args[9] is args[10] is ctypes.c_int64
    res, args = _native.SIGNATURES["dd_attn_sheet_u8"]
    assert res is ctypes.c_int32 and len(args) == 13
    assert _build.SOURCES.index("attn_heat.hip") > _build.SOURCES.index("attn_probs.hip")      # behind the step's kernels
    assert "attn_heat.hip" not in _build.EXTRA_FLAGS                                  # IEEE fp64, NaNs honoured
