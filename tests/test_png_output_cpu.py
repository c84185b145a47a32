"""PNG output without a GPU: the reference encoder of the format (tests/png_reference.py) against its own decoder-side
checker, against PIL and against the properties its cases are there for; the package's constants, header and ctypes table;
the argument handling of the Python layer and of the built library; concat_views against the reference's concat_6_views."""
import ctypes
import io
import os
import re
import zlib

import numpy as np
import pytest
import torch

from tests import png_cases as C
from tests import png_reference as R

CASES = C.cases()
IDS = [c.name for c in CASES]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    z = np.load(C.GOLDEN)
    return {k: z[k] for k in z.files}


def test_fixture_pins_the_generated_inputs(golden):
    """Inputs re-derived from the generators AND stored: a drift of a generator shows as an input mismatch."""
    assert str(golden["pil_version"])
    for c in CASES:
        assert np.array_equal(golden["in_" + c.name], c.img), c.name
        assert golden["pil_" + c.name].shape == (2,)
    assert int(golden["crc_large"]) == zlib.crc32(C.large().tobytes())
    assert len(golden) == 2 * len(CASES) + 3
    for name in C.CROPS:
        assert golden["in_" + name].shape == (64, 96, 3)
    assert os.path.getsize(C.GOLDEN) < 512 * 1024


def test_cases_are_the_geometries_the_issue_names():
    shapes = {c.img.shape[:2] for c in CASES}
    assert shapes >= {(1, 1), (1, 7), (7, 1), (5, 3), (1, 5461), (2, 5461), (2, 5462), (64, 100)}
    lengths = {c.img.shape[0] * (1 + 3 * c.img.shape[1]) for c in CASES}
    assert lengths >= {R.CHUNK - 1, R.CHUNK, R.CHUNK + 1, 2 * R.CHUNK}
    assert any(c.img.shape[1] == 85 for c in CASES)                          # a row of 256 bytes
    assert C.large().shape == (900, 1600, 3) and C.batch().shape == (7, 37, 53, 3)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_file_passes_the_checker(case):
    data, _ = C.reference(case.name)
    pixels, types = R.check(data)
    assert np.array_equal(pixels, case.img)
    assert len(data) <= R.worst_case(*case.img.shape[:2])
    chunks = R.parse(data)
    n = case.img.shape[0] * (1 + 3 * case.img.shape[1])
    assert len(chunks) == 2 + -(-n // R.CHUNK)                               # one IDAT per chunk


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_file_opens_in_pil(case):
    Image = pytest.importorskip("PIL.Image")
    data, _ = C.reference(case.name)
    pil = Image.open(io.BytesIO(data))
    pil.load()
    assert pil.mode == "RGB" and pil.format == "PNG" and pil.size == (case.img.shape[1], case.img.shape[0])
    assert np.array_equal(np.array(pil), case.img)


def _filter_rule(img):
    """The rule of the issue, one byte at a time in plain Python."""
    h, w, _ = img.shape
    rows = [bytes(img[y].reshape(-1)) for y in range(h)]
    out = []
    for y, row in enumerate(rows):
        above = rows[y - 1] if y else bytes(len(row))
        sums = [0] * 5
        for k, x in enumerate(row):
            a, b, c = (row[k - 3], above[k], above[k - 3]) if k >= 3 else (0, above[k], 0)
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            paeth = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            for t, pred in enumerate((0, a, b, (a + b) // 2, paeth)):
                v = (x - pred) % 256
                sums[t] += v if v < 128 else 256 - v
        out.append(sums.index(min(sums)))
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_filter_byte_of_every_row_is_the_rules_choice(case):
    data, _ = C.reference(case.name)
    _, types = R.check(data)
    assert types.tolist() == R.choose_filters(case.img).tolist()
    if case.img.size <= 20000:
        assert types.tolist() == _filter_rule(case.img)
    assert len(types) == case.img.shape[0]


def test_cases_reach_the_paths_they_are_there_for():
    chunk = lambda name, i=0: C.reference(name)[1]["chunks"][i]             # noqa: E731
    # runs: every length behind the first literal that the issue lists; a run across a chunk end; one symbol
    rests = set(chunk("runs")["rest"].tolist())
    assert rests >= set(C.RUN_RESTS)
    zeros = C.reference("zeros_64x100")[1]["chunks"]
    assert len(zeros) == 2 and zeros[0]["rest"].tolist() == [R.CHUNK - 1] and zeros[1]["rest"].tolist() == [64 * 301 - R.CHUNK - 1]
    single = chunk("single_symbol")
    assert np.flatnonzero(single["hist"][:256]).tolist() == [0] and single["matches"] == 2
    # Huffman: all 256 literals equally often; trees deeper than both limits before they are limited
    uni = chunk("uniform256")
    assert uni["hist"][:256].tolist() == [64] * 256 and uni["matches"] == 0
    fib = chunk("fibonacci")
    assert not fib["stored"] and fib["matches"] == 0
    assert max(d for _, d in R.tree_depths(fib["hist"])) > 15 and max(fib["lens"]) == 15
    clf = chunk("cl_fibonacci")
    assert not clf["stored"]
    assert max(d for _, d in R.tree_depths(clf["cl_hist"])) > 7 and max(clf["cl_lens"]) == 7
    for c in (fib, clf):                                                     # complete codes after the limiting
        assert sum(2.0 ** -l for l in c["lens"] if l) == 1.0 and sum(2.0 ** -l for l in c["cl_lens"] if l) == 1.0
    # stored fallback: noise
    noise = C.reference("noise_64x100")
    assert all(c["stored"] for c in noise[1]["chunks"]) and len(noise[0]) == R.worst_case(64, 100)
    large = C.reference("large")[1]["chunks"]
    assert sum(c["stored"] for c in large) >= len(large) // 2 - 1 and not large[0]["stored"]


def test_size_conditions_hold_for_the_reference(golden):
    """The recorded margins over the model are what the reference needs, and every non-noise file is below PIL's
    compress_level=0 file; the ratio to PIL's default file on the natural crops is the one INTEGRATION.md 4n records."""
    for name in [c.name for c in CASES if not c.noise] + ["large"]:
        img = C.large() if name == "large" else next(c.img for c in CASES if c.name == name)
        data, _ = C.reference(name)
        assert C.margin(img, data) == C.MARGINS[name], name
        assert len(data) < int(golden["pil_" + name][1]), name
    assert set(C.MARGINS) == {c.name for c in CASES if not c.noise} | {"large"}
    for name in C.CROPS:
        ratio = len(C.reference(name)[0]) / float(golden["pil_" + name][0])
        assert 1.0 < ratio < 1.15, (name, ratio)
    for name in C.CROPS + ("64x85_one_chunk", "128x85_two_chunks", "large"):
        assert C.MARGINS[name] <= 3, name


def test_sources_header_and_ctypes_table_are_in_step():
    from dualdiff_amd import _build, _native, image_tables as T
    from dualdiff_amd.pipeline import image_output as IO
    assert "png.hip" in _build.SOURCES and "png.hip" not in _build.EXTRA_FLAGS
    hdr = open(os.path.join(ROOT, "include", "dualdiff_hip.h")).read()
    assert "tools/test.py:74-97" in hdr and "#define DD_ABI_VERSION 4" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("dd_png_workspace_bytes", "dd_png_encode_u8"):
        assert re.search(r"\b%s\s*\(" % name, code) and name in _native.SIGNATURES
    assert len(_native.SIGNATURES["dd_png_encode_u8"][1]) == code.split("dd_png_encode_u8(")[1].split(")")[0].count(",") + 1
    assert _native.ABI_VERSION == 4
    assert IO.PNG_MODES is T.PNG_MODES and "colour type 2" in T.PNG_MODES
    assert (T.PNG_CHUNK, T.PNG_FILE_FIXED, T.PNG_CHUNK_FIXED) == (R.CHUNK, R.FILE_FIXED, R.CHUNK_FIXED)
    for h, w in ((1, 1), (64, 85), (113, 48), (900, 1600)):
        assert T.png_capacity(h, w) == R.worst_case(h, w)
    src = open(os.path.join(ROOT, "dualdiff_amd", "ops.py")).read()
    assert not re.search(r"^\s*(from|import) .*pipeline", src, flags=re.M)      # ops stays below the pipeline


def test_python_layer_turns_down_bad_arguments():
    from dualdiff_amd import ops
    from dualdiff_amd.pipeline import image_output as IO
    good = torch.zeros((2, 16, 24, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.png_encode_u8(good)
    with pytest.raises(RuntimeError, match="GPU only"):
        IO.encode_png(good)
    for bad in (good[0], good[..., :2], good.float(), good.permute(0, 2, 1, 3), good[:0]):
        with pytest.raises(ValueError):
            ops.png_encode_u8(bad)
    for bad in (good[0, 0], good.float(), torch.zeros((2, 16, 24, 4), dtype=torch.uint8), good[:0]):
        with pytest.raises(ValueError, match="colour type 2"):
            IO.encode_png(bad)
    with pytest.raises(ValueError, match="out must be"):
        ops.png_encode_u8(good, out=torch.zeros((3, 4096), dtype=torch.uint8))
    with pytest.raises(ValueError, match="does not match"):
        ops.png_encode_u8(good, out=torch.zeros((2, 4096), dtype=torch.uint8), capacity=100)
    with pytest.raises(ValueError, match="capacity"):
        ops.png_encode_u8(good, capacity=50)
    for option in ({"compress_level": 9}, {"optimize": True}, {"bits": 16}, {"pnginfo": None}):
        with pytest.raises(ValueError, match="not built; available: 8-bit RGB"):
            IO.encode_png(good, **option)
        with pytest.raises(ValueError, match="not built"):
            IO.save_png(good, ["a.png", "b.png"], **option)


@pytest.fixture(scope="module")
def lib():
    from dualdiff_amd import _build, _native
    if not os.path.exists(_build.lib_path()):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _native.load(build_if_missing=False)


def test_library_turns_down_bad_calls_without_a_gpu(lib):
    """DD_ERR_BAD_ARG before any runtime call, so also on a box without a GPU."""
    P = ctypes.c_void_p(4096)
    need = lib.dd_png_workspace_bytes(2, 20, 32)
    # the filtered bytes, one slot of 5 + 16384 bytes per chunk, four counters and an offset per chunk, two words per frame
    assert need >= 2 * (20 * 97 + 16389 + 16 + 4 + 8) and need % 16 == 0
    assert lib.dd_png_workspace_bytes(6, 900, 1600) < 64 << 20
    for m, h, w in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, -8, 8), (65536, 8, 8), (1, 65535, 65535), (1, 1 << 30, 1)):
        assert lib.dd_png_workspace_bytes(m, h, w) == -1
    assert lib.dd_png_workspace_bytes(1, 1, 1) > 0 and lib.dd_png_workspace_bytes(1, 20000, 20000) > 0

    def call(frames=P, m=2, h=20, w=32, ws=P, ws_bytes=need, out=P, capacity=4096, lengths=P):
        return lib.dd_png_encode_u8(frames, m, h, w, ws, ws_bytes, out, capacity, lengths, None)
    bad = -1
    for name in ("frames", "ws", "out", "lengths"):
        assert call(**{name: None}) == bad, name
    for kw in ({"m": 0}, {"m": -3}, {"h": 0}, {"w": 0}, {"h": -8}, {"w": -8}, {"ws_bytes": need - 1}, {"ws_bytes": 0},
               {"capacity": 50}, {"capacity": 0}, {"capacity": -5}, {"ws": ctypes.c_void_p(4100)},
               {"lengths": ctypes.c_void_p(4098)}):
        assert call(**kw) == bad, kw
    assert call(h=65535, w=65535, ws_bytes=1 << 62) == -2                    # a file longer than the int32 lengths take
    assert call(m=65536, ws_bytes=1 << 62) == -2


def _concat_6_views(views, oneline=False):
    """runner/img_utils.py:5-40 for equal-sized views, in numpy: img_concat_h pastes left to right, img_concat_v top down"""
    if oneline:
        return np.concatenate(list(views), axis=1)
    return np.concatenate([np.concatenate(list(views[:3]), axis=1), np.concatenate(list(views[3:]), axis=1)], axis=0)


def test_concat_views_is_concat_6_views():
    from dualdiff_amd.pipeline.image_output import concat_views
    x = torch.from_numpy(np.random.RandomState(3).randint(0, 256, (2, 6, 5, 7, 3)).astype(np.uint8))
    grid = concat_views(x)
    assert grid.shape == (2, 10, 21, 3) and grid.dtype == torch.uint8
    line = concat_views(x, oneline=True)
    assert line.shape == (2, 5, 42, 3)
    for b in range(2):
        assert np.array_equal(grid[b].numpy(), _concat_6_views(x[b].numpy()))
        assert np.array_equal(line[b].numpy(), _concat_6_views(x[b].numpy(), oneline=True))
    assert np.array_equal(concat_views(x[:, :2], oneline=True)[1].numpy(), _concat_6_views(x[1, :2].numpy(), oneline=True))
    assert np.array_equal(concat_views(x.permute(0, 1, 3, 2, 4))[0].numpy(), _concat_6_views(x[0].numpy().transpose(0, 2, 1, 3)))
    with pytest.raises(ValueError, match="6 views"):
        concat_views(x[:, :5])
    with pytest.raises(ValueError, match="at least 2"):
        concat_views(x[:, :1], oneline=True)
    with pytest.raises(ValueError):
        concat_views(x[0])
