"""PNG input without a GPU: the constructed cases (tests/png_input_cases.py) against PIL and against the fixture minted
from PIL, the package's chunk walk and its refusals, the argument handling of the Python layer and of the built library,
the crop arithmetic of the ORS condition, and the decode core's bounds: the kernels' own functions, run by a stand-alone
host program under the address and undefined-behaviour sanitizers, over good and over broken streams."""
import ctypes
import io
import os
import re
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest
import torch

from tests import png_input_cases as C
from tests.golden import mint_png_input as MI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c.name for c in C.cases()]


@pytest.fixture(scope="module")
def golden():
    return {name: (data, pix) for name, data, pix in MI.files()}


def _case(name):
    return next(c for c in C.cases() if c.name == name)


def test_fixture_holds_the_files_the_issue_names(golden):
    z = MI.load()
    assert str(z["pil_version"]) and os.path.getsize(MI.PATH) < 100 * 1000
    assert set(golden) == {"crop_object", "crop_road", "panorama"}
    out = np.load(MI.OUTPUT)
    for name in ("crop_object", "crop_road"):
        assert golden[name][1].shape == (64, 96, 3) and np.array_equal(golden[name][1], out["in_" + name])
    pano = MI.panorama()
    assert pano.shape == (12, 60, 4) and 0 < int((pano[..., 3] != 255).sum()) < 12 * 60
    assert np.array_equal(golden["panorama"][1], pano[..., :3])
    for data, _ in golden.values():
        assert data[:8] == C.SIGNATURE


def test_the_cases_are_the_ones_the_issue_names():
    shapes = {c.name: (c.pixels.shape[:2], c.colour_type) for c in C.cases()}
    assert shapes["1x1_rgb"] == ((1, 1), 2) and shapes["2x3_rgb"] == ((2, 3), 2) and shapes["7x5_rgba"] == ((7, 5), 6)
    assert shapes["3x9_grey"] == ((3, 9), 0) and shapes["5x2_rgb_odd_row"] == ((5, 2), 2) and (1 + 3 * 2) % 2 == 1
    assert C.RGBA_FILTERS == (4, 2, 3, 1, 0, 4, 3)
    pix, filt, stream = C.rgba_7x5()
    assert len(filt) == 147 and len(stream) == 158
    assert [_case(n).idats for n in ("7x5_one_idat", "7x5_byte_idats", "7x5_empty_idats")] == [1, 158, 5]
    # level 0 of 76800 bytes: two stored blocks; the period of 126 rows is found by zlib, the one of 127 is out of its reach
    assert 300 * (1 + 3 * 85) == 76800 > 65535
    assert len(_case("300x85_period_126").data) < 40000 < 76800 < len(_case("300x85_period_127").data)
    assert len(C.broken()) == 13 and sorted({b.status for b in C.broken()}) == [1 << i for i in range(11)]


@pytest.mark.parametrize("name", NAMES)
def test_constructed_pixels_equal_pil(name):
    Image = pytest.importorskip("PIL.Image")
    c = _case(name)
    got = np.asarray(Image.open(io.BytesIO(c.data)).convert("RGB"))
    assert got.shape == c.pixels.shape and np.array_equal(got, c.pixels)


def test_fixture_pixels_equal_pil(golden):
    Image = pytest.importorskip("PIL.Image")
    for name, (data, pix) in golden.items():
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), pix), name
    f, pix = C.foreign_chunk_shaped()
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(f)).convert("RGB")), pix)
    for name, f, img in C.own_files()[:6]:
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(f)).convert("RGB")), img), name


@pytest.mark.parametrize("name", NAMES)
def test_parse_png_fields(name):
    from dualdiff_amd.pipeline import png_input as PI
    c = _case(name)
    info = PI.parse_png(c.data)
    assert (info.h, info.w) == c.pixels.shape[:2] and info.colour_type == c.colour_type and len(info.idats) == c.idats
    stream = b"".join(c.data[o:o + n] for o, n in info.idats)
    channels = C.CHANNELS[c.colour_type]
    assert len(zlib.decompress(stream)) == info.h * (1 + channels * info.w)
    for o, n in info.idats:
        assert c.data[o - 4:o] == b"IDAT" and struct.unpack(">I", c.data[o - 8:o - 4])[0] == n
    small = info.h * (1 + 3 * info.w) <= 16384
    assert info.chunked == (c.colour_type == 2 and small and c.idats == 1)


def test_parse_png_on_our_own_and_on_pil_files(golden):
    from dualdiff_amd.pipeline import png_input as PI
    for name, f, img in C.own_files():
        info = PI.parse_png(f)
        assert info.chunked and (info.h, info.w) == img.shape[:2] and len(info.idats) == -(-(info.h * (1 + 3 * info.w)) // 16384), name
    assert PI.parse_png(C.foreign_chunk_shaped()[0]).chunked                 # the shape proves nothing: the device verifies
    for name, (data, pix) in golden.items():
        info = PI.parse_png(data)
        assert (info.h, info.w) == pix.shape[:2] and info.colour_type == (6 if name == "panorama" else 2)


def _refused():
    """[(kind, file, the words its refusal holds)]"""
    pix, filt, stream = C.rgba_7x5()
    idat, end = C.chunk(b"IDAT", stream), C.chunk(b"IEND")

    def file(colour, depth=8, interlace=0, extra=b""):
        return C.SIGNATURE + C.ihdr(7, 5, colour, depth=depth, interlace=interlace) + extra + idat + end
    return [("palette", file(3, extra=C.chunk(b"PLTE", bytes(6))), "a palette image (colour type 3)"),
            ("palette_4bit", file(3, depth=4, extra=C.chunk(b"PLTE", bytes(6))), "a palette image (colour type 3)"),
            ("grey_alpha", file(4), "grey with alpha (colour type 4)"),
            ("16_bit", file(2, depth=16), "16-bit samples"),
            ("1_bit", file(0, depth=1), "1-bit samples"),
            ("4_bit", file(0, depth=4), "4-bit samples"),
            ("adam7", file(6, interlace=1), "Adam7 interlace"),
            ("apng", file(6, extra=C.chunk(b"acTL", struct.pack(">II", 1, 0))), "an animated PNG (acTL)"),
            ("not_a_png", b"\xff\xd8\xff\xe0" + bytes(64), "a file that is not a PNG")]


def test_every_refused_kind_raises_and_names_itself():
    from dualdiff_amd.pipeline import png_input as PI
    good = _case("7x5_rgba").data
    kinds = _refused()
    assert len(kinds) == 9
    for kind, data, word in kinds:
        with pytest.raises(ValueError, match=re.escape(word)) as e:
            PI.parse_png(data)
        assert "is not built; available: bit depth 8, no interlace, colour type 0 (grey), 2 (RGB) or 6 (RGBA" in str(e.value), kind
        # as frame 1 of a batch: refused on the host, by its index, before anything is uploaded (no GPU is there to upload to)
        with pytest.raises(ValueError, match="^frame 1: .*" + re.escape(word)):
            PI.decode_png([good, data, good])
        with pytest.raises(ValueError, match="^frame 3: "):
            PI.decode_png([[good, good], [good, data]])
    assert "import PIL" not in open(os.path.join(ROOT, "dualdiff_amd", "pipeline", "png_input.py")).read().replace(
        "does not import PIL", "")


def test_broken_framing_raises():
    from dualdiff_amd.pipeline import png_input as PI
    good = _case("7x5_rgba").data
    at = good.index(b"IDAT")
    flipped = bytearray(good)
    flipped[-13] ^= 1                                                         # the last byte of the IDAT's CRC
    with pytest.raises(ValueError, match="chunk IDAT at byte %d: the CRC does not match" % (at - 4)):
        PI.parse_png(bytes(flipped))
    flipped = bytearray(good)
    flipped[at + 10] ^= 0x40                                                  # a payload byte
    with pytest.raises(ValueError, match="^frame 2: chunk IDAT .* CRC"):
        PI.decode_png([good, good, bytes(flipped)])
    pix, filt, stream = C.rgba_7x5()
    idat, end, head = C.chunk(b"IDAT", stream), C.chunk(b"IEND"), C.SIGNATURE + C.ihdr(7, 5, 6)
    for data, word in ((head + end, "no IDAT chunk"), (head + idat, "no IEND chunk"), (head + idat + end + b"\x00", "behind the IEND"),
                       (C.SIGNATURE + idat + end, "the first chunk is not a 13-byte IHDR"),
                       (head + idat + C.chunk(b"tEXt", b"a\x00b") + idat + end, "not consecutive"),
                       (good[:-20], "cut short"), (head + C.chunk(b"ABCD") + idat + end, "critical chunk ABCD"),
                       (C.SIGNATURE + C.chunk(b"IHDR", struct.pack(">IIBBBBB", 5, 7, 8, 6, 1, 0, 0)) + idat + end, "compression method 1"),
                       (C.SIGNATURE + C.chunk(b"IHDR", struct.pack(">IIBBBBB", 0, 7, 8, 6, 0, 0, 0)) + idat + end, "a frame of 7 x 0")):
        with pytest.raises(ValueError, match=re.escape(word)):
            PI.parse_png(data)


def test_mixed_geometry_raises():
    from dualdiff_amd.pipeline import png_input as PI
    a, b, g = _case("7x5_rgba").data, _case("2x3_rgb").data, _case("3x9_grey").data
    with pytest.raises(ValueError, match="frame 2: 2 x 3 differs from frame 0 \\(7 x 5\\)"):
        PI.decode_png([a, a, b])
    with pytest.raises(ValueError, match="frame 1: 3 x 9 differs"):
        PI.decode_png([b, g])
    for bad in ([], a, [[a, a], [a]], [a, "x.png"]):
        with pytest.raises(ValueError):
            PI.decode_png(bad)


def test_cpu_tensors_raise_gpu_only(tmp_path):
    from dualdiff_amd import ops
    from dualdiff_amd.pipeline import png_input as PI
    rgba, one, ours = _case("7x5_rgba").data, _case("7x5_byte_idats").data, C.own_files()[3][1]      # 5 x 3
    with pytest.raises(RuntimeError, match="GPU only"):
        PI.decode_png([rgba], device="cpu")
    path = tmp_path / "a.png"
    path.write_bytes(rgba)
    with pytest.raises(RuntimeError, match="GPU only"):
        PI.load_png([[str(path)]], device="cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        PI.OccCondition()([rgba], device="cpu")
    # the upload: colour type per file, the streams one behind the other with the chunk framing stripped
    stream = C.rgba_7x5()[2]
    streams, files, tab, types, h, w = PI.upload_png([rgba, one], "cpu")
    assert (h, w, types, tab) == (7, 5, [6, 6], None) and files.tolist() == [[0, 158, 6, -1], [158, 158, 6, -1]]
    assert bytes(streams[:316].tolist()) == stream + stream
    info = PI.parse_png(ours)
    streams, files, tab, types, h, w = PI.upload_png([ours, ours], "cpu")
    n = sum(length for _, length in info.idats)
    assert files.tolist() == [[0, n, 2, 0], [n, n, 2, 2]] and tab.tolist() == [0, n, 0, n] and types == [2, 2]
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.png_decode_u8(streams, files, tab, types, h, w)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.png_condition(torch.zeros(1, 4, 12, 3, dtype=torch.uint8), views=6)
    for kw in ({"h": 0}, {"w": -1}, {"h": 5.0}, {"types": [2]}, {"types": [2, 3]}, {"types": [2, 4]}, {"chunked": True},
               {"streams": streams.float()}, {"files": files.long()}, {"files": files[:, :3]}, {"tab": tab.long()}):
        a = dict(streams=streams, files=files, tab=tab, types=types, h=h, w=w, chunked=None)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.png_decode_u8(a["streams"], a["files"], a["tab"], a["types"], a["h"], a["w"], chunked=a["chunked"])
    frames = torch.zeros(2, 9, 72, 3, dtype=torch.uint8)
    for kw in ({"views": 5}, {"views": 0}, {"top": -1}, {"top": 5, "size": (5, 8)}, {"left": 5, "size": (5, 8)}, {"size": (0, 8)},
               {"size": 8}, {"frames": frames.float()}, {"frames": frames[..., :2]}):
        a = dict(frames=frames, views=6, top=4, left=2, size=(5, 8))
        a.update(kw)
        with pytest.raises(ValueError):
            ops.png_condition(a["frames"], views=a["views"], top=a["top"], left=a["left"], size=a["size"])


def test_python_constants_are_the_sources():
    from dualdiff_amd import _build, image_tables, ops
    hdr = open(os.path.join(ROOT, "include", "dualdiff_hip.h")).read()
    core = open(os.path.join(ROOT, "dualdiff_amd", "csrc", "png_decode_core.h")).read()
    hip = open(os.path.join(ROOT, "dualdiff_amd", "csrc", "png_decode.hip")).read()
    names = ("TRUNCATED", "BAD_BLOCK", "BAD_STORED", "BAD_LENGTHS", "BAD_SYMBOL", "BAD_DISTANCE", "TOO_LONG", "TOO_SHORT",
             "BAD_ADLER", "BAD_ZLIB", "BAD_FILTER")

    def define(src, name):
        return int(re.search(r"#define %s (\d+)" % name, src).group(1))
    bits = [b for b, _ in ops.PNG_DECODE_STATUS]
    assert [define(hdr, "DD_PNG_" + n) for n in names] == bits == [define(core, "DD_PD_" + n) for n in names]
    assert bits == [1 << i for i in range(11)] == [getattr(C, n) for n in names]
    assert len({t for _, t in ops.PNG_DECODE_STATUS}) == 11
    assert "constexpr int kSeg = %d;" % ops.PNG_DECODE_CHUNK in hip and ops.PNG_DECODE_CHUNK == image_tables.PNG_CHUNK
    assert "png_decode.hip" in _build.SOURCES and _build.SOURCES.index("png_decode.hip") == _build.SOURCES.index("png.hip") + 1
    assert "define DD_ABI_VERSION 4" in hdr
    lut = image_tables.png_unit_lut()
    assert lut.dtype == torch.float32 and torch.equal(lut, torch.arange(256, dtype=torch.uint8).float().div(255))


@pytest.fixture(scope="module")
def lib():
    from dualdiff_amd import _build, _native
    if not os.path.exists(_build.lib_path()):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _native.load(build_if_missing=False)


def test_library_turns_down_bad_calls_without_a_gpu(lib):
    """DD_ERR_BAD_ARG before any runtime call, so also on a box without a GPU."""
    P = ctypes.c_void_p(4096)
    need = lib.dd_png_decode_workspace_bytes(2, 7, 5)
    # the filtered bytes at four bytes per pixel, and per frame a flag, the trailer and one pair of sums per segment
    assert need >= 2 * (7 * 21 + 4 + 4 + 8) and need % 16 == 0
    assert lib.dd_png_decode_workspace_bytes(6, 900, 1600) < 64 << 20
    for m, h, w in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, -8, 8), (65536, 8, 8), (1, 40000, 40000)):
        assert lib.dd_png_decode_workspace_bytes(m, h, w) == -1, (m, h, w)
    types = (ctypes.c_int32 * 2)(2, 6)

    def call(streams=P, streams_bytes=400, files=P, tab=P, ntab=4, colour_types=types, m=2, h=7, w=5, chunked=1, out=P,
             status=P, paths=P, ws=P, ws_bytes=need):
        return lib.dd_png_decode_u8(streams, streams_bytes, files, tab, ntab, colour_types, m, h, w, chunked, out, status,
                                    paths, ws, ws_bytes, None)
    bad = -1
    for name in ("streams", "files", "tab", "colour_types", "out", "status", "paths", "ws"):
        assert call(**{name: None}) == bad, name
    for kw in ({"m": 0}, {"m": -3}, {"h": 0}, {"w": 0}, {"h": -8}, {"streams_bytes": 0}, {"streams_bytes": -1}, {"ntab": -1},
               {"chunked": 2}, {"chunked": -1}, {"ws_bytes": need - 1}, {"ws_bytes": 0}, {"ws": ctypes.c_void_p(4100)},
               {"files": ctypes.c_void_p(4097)}, {"tab": ctypes.c_void_p(4098)}, {"status": ctypes.c_void_p(4099)},
               {"paths": ctypes.c_void_p(4097)}, {"colour_types": (ctypes.c_int32 * 2)(2, 3)},
               {"colour_types": (ctypes.c_int32 * 2)(4, 2)}, {"colour_types": (ctypes.c_int32 * 2)(2, -1)}):
        assert call(**kw) == bad, kw
    assert call(h=40000, w=40000, ws_bytes=1 << 62) == -2                    # positions in a frame are 32-bit
    assert call(m=65536, colour_types=(ctypes.c_int32 * 65536)(), ws_bytes=1 << 62) == -2

    def cond(frames=P, out=P, lut=P, b=2, h=9, w=72, views=6, top=4, left=2, oh=5, ow=8):
        return lib.dd_png_condition(frames, out, lut, b, h, w, views, top, left, oh, ow, None)
    for name in ("frames", "out", "lut"):
        assert cond(**{name: None}) == bad, name
    for kw in ({"b": 0}, {"h": 0}, {"w": 0}, {"views": 0}, {"views": 5}, {"top": -1}, {"left": -1}, {"oh": 0}, {"ow": 0}, {"top": 5},
               {"left": 5}, {"ow": 11}, {"oh": 6}, {"out": ctypes.c_void_p(4097)}, {"lut": ctypes.c_void_p(4098)}):
        assert cond(**kw) == bad, kw


# ---- the ORS condition's crop -------------------------------------------------------------------------------------------------

def _reference_crop(x, in_shape, out_shape, views):
    """dataset/utils.py:348-372 restated: hd_crop per view of width W / views, the views side by side again"""
    per_w = x.shape[-1] // views
    res = []
    for v in range(views):
        part = x[..., per_w * v:per_w * (v + 1)]
        h_crop = in_shape[0] - out_shape[0]
        w_crop = (in_shape[1] - out_shape[1]) // 2
        y = part[..., h_crop:, w_crop:(in_shape[1] - w_crop)]
        assert tuple(y.shape[-2:]) == tuple(out_shape)
        res.append(y)
    return np.concatenate(res, axis=-1)


def test_occ_condition_crop_arithmetic():
    from types import SimpleNamespace
    from dualdiff_amd.pipeline import png_input as PI

    def cfg(size):
        return SimpleNamespace(dataset=SimpleNamespace(image_size=size))
    for size, hw in (([224, 400], (224, 2400)), ([432, 768], (432, 4608))):
        occ = PI.OccCondition.from_config(cfg(size))
        assert (occ.views, occ.in_hw, occ.out_hw) == (6, None, None) and occ.crop(*hw) == (0, 0, hw[0], hw[1] // 6)
    occ = PI.OccCondition.from_config({"dataset": {"image_size": [256, 704]}})
    assert occ.crop(432, 4608) == (432 - 256, (768 - 704) // 2, 256, 704) == (176, 32, 256, 704)
    with pytest.raises(ValueError, match="defined for 432 x 6 x 768"):
        occ.crop(224, 2400)
    with pytest.raises(NotImplementedError, match="crop_drivewm"):
        PI.OccCondition.from_config(cfg([192, 384]))
    with pytest.raises(ValueError, match="image_size"):
        PI.OccCondition.from_config(cfg([128, 256]))
    # the indices the crop selects, against slicing as the reference slices
    occ = PI.OccCondition(views=6, in_hw=(9, 12), out_hw=(5, 8))
    top, left, oh, ow = occ.crop(9, 72)
    assert (top, left, oh, ow) == (4, 2, 5, 8)
    x = np.arange(3 * 9 * 72).reshape(3, 9, 72)
    mine = np.concatenate([x[:, top:top + oh, v * 12 + left:v * 12 + left + ow] for v in range(6)], axis=-1)
    assert np.array_equal(mine, _reference_crop(x, (9, 12), (5, 8), 6)) and mine.shape == (3, 5, 48)
    big = np.arange(432 * 4608).reshape(1, 432, 4608)
    t, l, h, w = PI.OccCondition.from_config(cfg([256, 704])).crop(432, 4608)
    mine = np.concatenate([big[:, t:t + h, v * 768 + l:v * 768 + l + w] for v in range(6)], axis=-1)
    assert np.array_equal(mine, _reference_crop(big, (432, 768), (256, 704), 6))
    for kw in ({"views": 0}, {"in_hw": (9, 12)}, {"in_hw": (9, 12), "out_hw": (5, 7)}, {"in_hw": (9, 12), "out_hw": (10, 8)}):
        with pytest.raises(ValueError):
            PI.OccCondition(**kw)
    with pytest.raises(ValueError, match="6 divides"):
        PI.OccCondition().crop(9, 70)


# ---- the decode core under the sanitizers -----------------------------------------------------------------------------------

def test_decode_core_on_the_host_under_sanitizers(golden, tmp_path):
    """tools/png_decode_host_check.cpp, built with -fsanitize=address,undefined: every good file — the constructed cases,
    PIL's files, a foreign file of our shape and our own format's files, those both sequentially and chunk by chunk —
    decodes to the expected pixels, and every broken stream runs clean and reports exactly its status."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    for static in (["-static-libasan", "-static-libubsan"], []):
        if subprocess.run([cxx] + flags + static + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0:
            break
    else:
        pytest.skip("the compiler links no sanitizer runtime")
    exe = tmp_path / "png_decode_host_check"
    build = subprocess.run([cxx] + flags + static + ["-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tools", "png_decode_host_check.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    good = [(c.name, c.data, c.pixels, None) for c in C.cases()]
    good += [("pil_" + name, data, pix, None) for name, (data, pix) in golden.items()]
    good += [("foreign", *C.foreign_chunk_shaped(), 0)]
    good += [("own_" + name, f, img, 1) for name, f, img in C.own_files()]
    want = {}
    for name, data, pix, chunked in good:
        (tmp_path / (name + ".png")).write_bytes(data)
        want[name] = (0, pix, chunked)
    for b in C.broken():
        (tmp_path / (b.name + ".png")).write_bytes(b.data)
        want[b.name] = (b.status, None, None)
    run = subprocess.run([str(exe)] + [str(tmp_path / (n + ".png")) for n in want], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-3000:])
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    lines = {os.path.basename(l.split()[0])[:-4]: l.split()[1:] for l in run.stdout.splitlines() if ".png " in l}
    assert run.stdout.splitlines()[-1] == "%d files, 0 failed" % len(want) and set(lines) == set(want)
    for name, (status, pix, chunked) in want.items():
        h, w, colour, got, was_chunked = (int(v) for v in lines[name])
        assert got == status, (name, got, status)
        if chunked is not None:
            assert was_chunked == chunked, name
        if pix is not None:
            out = np.fromfile(str(tmp_path / (name + ".png.rgb")), dtype=np.uint8)
            assert (h, w) == pix.shape[:2] and np.array_equal(out.reshape(h, w, 3), pix), name
