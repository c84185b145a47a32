"""JPEG output without a GPU: the numpy restatement of libjpeg's baseline encoder (tests/jpeg_reference.py) against the
fixture minted from PIL and against PIL itself, the package's header and tables against both, and the argument handling of
the Python layer and of the built library."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

from tests import jpeg_reference as J
from tests.golden import mint_jpeg as M

CASES = list(M.cases())
IDS = [c[0] for c in CASES]


@pytest.fixture(scope="module")
def golden():
    z = np.load(M.PATH)
    return {k: z[k] for k in z.files}


def test_fixture_holds_the_cases_the_issue_names(golden):
    assert str(golden["pil_version"])
    assert len(golden) == 1 + 2 * len(CASES)
    shapes = {c[2].shape[:2] for c in CASES if c[1] == 75}
    assert shapes == {(1, 1), (8, 8), (16, 16), (9, 17), (17, 31), (24, 40), (40, 24), (20, 32), (37, 53), (45, 80), (90, 160),
                      (57, 100)}
    for q in (1, 50, 95, 100):
        assert len({c[2].shape[:2] for c in CASES if c[1] == q}) >= 3
    assert os.path.getsize(M.PATH) < 512 * 1024


@pytest.mark.parametrize("name,quality,img", CASES, ids=IDS)
def test_restatement_equals_fixture(golden, name, quality, img):
    """Inputs re-derived from the seeds AND stored: a drift of the generator shows as an input mismatch."""
    assert np.array_equal(golden["in_" + name], img)
    want = golden["out_" + name].tobytes()
    got = J.encode(img, quality)
    assert len(got) == len(want) and got == want


def test_fixture_covers_the_code_paths(golden):
    """What tests/golden/mint_jpeg.py asserts when it mints, checked again on the stored bytes."""
    stats, stuffed = {}, 0
    for name, quality, img in CASES:
        J.encode(img, quality, stats)
        data = golden["out_" + name].tobytes()
        stuffed += data[len(J.header(img.shape[0], img.shape[1], quality)):].count(b"\xff\x00")
    assert stuffed > 0 and stats["zrl"] >= {1, 2, 3} and stats["dc_sizes"] == set(range(12))
    flat = golden["out_40x24_flat_q75"].tobytes()
    # DC difference 0 throughout: 4 x (2 + 4) + 2 x (2 + 2) bits = 4 bytes per MCU, 3 x 2 MCUs
    assert len(flat) - len(J.header(40, 24, 75)) - 2 == 4 * 6


@pytest.mark.parametrize("name,quality,img", CASES, ids=IDS)
def test_restatement_equals_pil(name, quality, img):
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=quality)
    assert J.encode(img, quality) == buf.getvalue()


@pytest.mark.parametrize("name,quality,img", CASES, ids=IDS)
def test_header_equals_fixture(golden, name, quality, img):
    from dualdiff_amd.pipeline.image_output import jpeg_header
    h, w = img.shape[:2]
    data = golden["out_" + name].tobytes()
    head = jpeg_header(h, w, quality)
    sos = data.index(b"\xff\xda")
    assert len(head) == sos + 2 + 12 == 623                                  # up to and including SOS
    assert data[:len(head)] == head == J.header(h, w, quality)


@pytest.mark.parametrize("quality", [1, 10, 30, 49, 50, 75, 90, 95, 100])
def test_tables_come_from_one_place(quality):
    """The quantisation values the kernels divide by are the header's DQT bytes; the Huffman entries are the codes the
    restatement derives from the header's DHT segments."""
    from dualdiff_amd.pipeline import image_output as IO
    t = IO.jpeg_tables(quality)
    assert t.dtype == torch.int32 and t.shape == (672,)
    t = t.tolist()
    head = IO.jpeg_header(16, 16, quality)
    at = head.index(b"\xff\xdb")
    assert list(head[at + 5:at + 69]) == t[:64] and list(head[at + 74:at + 138]) == t[64:128]
    ql, qc = J.quant_tables(quality)
    assert t[:64] == ql[J.ZIGZAG].tolist() and t[64:128] == qc[J.ZIGZAG].tolist()
    assert tuple(J.ZIGZAG.tolist()) == IO.JPEG_ZIGZAG
    for base, spec, size in ((128, J.DC_LUMA, 16), (144, J.DC_CHROMA, 16), (160, J.AC_LUMA, 256), (416, J.AC_CHROMA, 256)):
        codes = J.huff_codes(spec)
        for sym in range(size):
            code, length = codes.get(sym, (0, 0))
            assert t[base + sym] == (code << 8) | length, (base, sym)


def test_python_layer_turns_down_bad_arguments():
    from dualdiff_amd import ops
    from dualdiff_amd.pipeline import image_output as IO
    good = torch.zeros((2, 16, 24, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.jpeg_encode_u8(good)
    with pytest.raises(RuntimeError, match="GPU only"):
        IO.encode_jpeg(good)
    for bad in (good[0], good[..., :2], good.float(), good.permute(0, 2, 1, 3), good[:0]):
        with pytest.raises(ValueError):
            ops.jpeg_encode_u8(bad)
    for bad in (good[0, 0], good.float(), torch.zeros((2, 16, 24, 4), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            IO.encode_jpeg(bad)
    for q in (0, 101, -1, 75.0, True, None, "75"):
        with pytest.raises(ValueError, match="quality"):
            ops.jpeg_encode_u8(good, quality=q)
        with pytest.raises(ValueError, match="quality"):
            IO.jpeg_header(16, 24, q)
    for size in ((0, 8), (8, 0), (65536, 8), (8, 65536)):
        with pytest.raises(ValueError):
            IO.jpeg_header(size[0], size[1], 75)
    with pytest.raises(ValueError, match="out must be"):
        ops.jpeg_encode_u8(good, out=torch.zeros((3, 4096), dtype=torch.uint8))
    with pytest.raises(ValueError, match="capacity"):
        ops.jpeg_encode_u8(good, capacity=624)
    for option in ({"subsampling": 0}, {"optimize": True}, {"progressive": True}, {"exif": b""}):
        with pytest.raises(ValueError, match="not built; available: baseline, 4:2:0"):
            IO.encode_jpeg(good, **option)
        with pytest.raises(ValueError, match="not built"):
            IO.save_jpeg(good, ["a.jpg", "b.jpg"], **option)


@pytest.fixture(scope="module")
def lib():
    from dualdiff_amd import _build, _native
    if not os.path.exists(_build.lib_path()):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _native.load(build_if_missing=False)


def test_library_turns_down_bad_calls_without_a_gpu(lib):
    """DD_ERR_BAD_ARG before any runtime call, so also on a box without a GPU."""
    P = ctypes.c_void_p(4096)
    need = lib.dd_jpeg_workspace_bytes(2, 20, 32)
    # coefficients, two counters per MCU, the frame's bit total, the chunk counters, 64 stream words per block
    assert need >= 2 * 4 * (6 * 64 * 2 + 8 + 6 * 64 * 4) and need % 16 == 0
    assert lib.dd_jpeg_workspace_bytes(6, 900, 1600) < 128 << 20
    for m, h, w in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, 65536, 8), (1, 8, 65536), (1, 65535, 65535)):
        assert lib.dd_jpeg_workspace_bytes(m, h, w) == -1

    def call(frames=P, m=2, h=20, w=32, header=P, header_len=623, tables=P, ws=P, ws_bytes=need, out=P, capacity=4096,
             lengths=P):
        return lib.dd_jpeg_encode_u8(frames, m, h, w, header, header_len, tables, ws, ws_bytes, out, capacity, lengths, None)
    bad = -1
    for name in ("frames", "header", "tables", "ws", "out", "lengths"):
        assert call(**{name: None}) == bad, name
    for kw in ({"m": 0}, {"m": -3}, {"h": 0}, {"w": 0}, {"h": -8}, {"w": -8}, {"h": 65536}, {"w": 65536}, {"header_len": 0},
               {"header_len": -1}, {"ws_bytes": need - 1}, {"ws_bytes": 0}, {"capacity": 624}, {"capacity": 0},
               {"capacity": -5}, {"ws": ctypes.c_void_p(4100)}, {"tables": ctypes.c_void_p(4097)},
               {"lengths": ctypes.c_void_p(4098)}):
        assert call(**kw) == bad, kw
    assert call(h=65535, w=65535, ws_bytes=1 << 62) == -2                    # more MCUs than the 32-bit bit offsets take
