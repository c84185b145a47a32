"""JPEG input without a GPU: the numpy restatement of libjpeg's baseline decoder (tests/jpeg_decode_reference.py) against the
fixture minted from PIL and against PIL itself, the package's marker walk and its refusals, the argument handling of the
Python layer and of the built library, and the decode core's bounds: the kernels' own functions, run in the kernels' order
by a stand-alone host program under the address and undefined-behaviour sanitizers, over good and over broken streams."""
import ctypes
import io
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import jpeg_decode_reference as R
from tests.golden import mint_jpeg as M
from tests.golden import mint_jpeg_input as MI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c[0] for c in M.cases()] + list(MI.NEW)


@pytest.fixture(scope="module")
def accepted():
    return {name: (data, pix) for name, data, pix in MI.accepted(*MI.load())}


@pytest.fixture(scope="module")
def golden():
    return MI.load()[1]


def test_fixture_holds_the_cases_the_issue_names(golden, accepted):
    assert str(golden["pil_version"])
    assert len(accepted) == 36 + 11 and len(golden) == 1 + 36 + 2 * 11 + len(MI.REFUSED)
    assert {accepted[n][1].shape[:2] for n in ("8x8_444", "9x7_444", "33x47_444")} == {(8, 8), (9, 7), (33, 47)}
    assert {accepted[n][1].shape[:2] for n in ("17x31_optimize", "20x32_optimize", "37x53_optimize")} == {(17, 31), (20, 32), (37, 53)}
    # 4:2:0 frames whose chroma plane is one or two columns wide, taller than two rows, and one just wide enough to filter
    narrow = {accepted[n][1].shape[:2] for n in MI.NEW if n.endswith("_narrow")}
    assert narrow == {(3, 1), (9, 3), (17, 4), (33, 2), (7, 5)}
    assert set(MI.REFUSED) == {"progressive", "restart", "422", "grayscale", "cmyk"}
    assert os.path.getsize(MI.PATH) <= os.path.getsize(M.PATH)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_fixture(accepted, name):
    data, want = accepted[name]
    got = R.decode(data)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert int((got != want).sum()) == 0


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_pil(accepted, name):
    Image = pytest.importorskip("PIL.Image")
    data, want = accepted[name]
    fresh = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    assert np.array_equal(fresh, want) and np.array_equal(R.decode(data), fresh)


def test_fixture_covers_the_code_paths(accepted):
    """What tests/golden/mint_jpeg_input.py asserts when it mints, checked again on the stored bytes."""
    stats, stuffed = {}, 0
    for data, _ in accepted.values():
        R.decode(data, stats)
        stuffed += R.headers(data)["scan"].count(b"\xff\x00")
    assert stuffed > 0 and stats["zrl"] > 0 and stats["eob_only"] > 0 and stats["dc_sizes"] == set(range(12))
    standard = R.headers(accepted["37x53_uniform_q75"][0])["huffman"]
    for name in ("17x31_optimize", "20x32_optimize", "37x53_optimize"):
        assert R.headers(accepted[name][0])["huffman"] != standard
    for name in ("8x8_444", "9x7_444", "33x47_444"):
        assert R.headers(accepted[name][0])["factors"] == [(1, 1)] * 3


@pytest.mark.parametrize("name", NAMES)
def test_parse_jpeg_fields(accepted, name):
    from dualdiff_amd.pipeline import jpeg_input as JI
    data, pix = accepted[name]
    info, want = JI.parse_jpeg(data), R.headers(data)
    assert (info.h, info.w) == pix.shape[:2] == (want["h"], want["w"])
    assert info.sampling == (444 if name.endswith("_444") else 420)
    assert R.headers(data)["factors"][0] == ((1, 1) if name.endswith("_444") else (2, 2))
    assert data[info.scan[0] - 14:info.scan[0] - 12] == b"\xff\xda" and data[info.scan[1]:] == b"\xff\xd9"
    assert data[info.scan[0]:info.scan[1]] == want["scan"]
    assert [c[0] for c in info.components] == [1, 2, 3] and [c[1:] for c in info.components] == [(0, 0, 0), (1, 1, 1), (1, 1, 1)]
    for i, c in enumerate(info.components):
        assert list(info.qtables[c[1]]) == want["q"][i].tolist()                # natural order
    assert info.huffman == want["huffman"] and set(info.huffman) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    block = JI.table_block(info)
    assert len(block) == 4016
    assert np.frombuffer(block, dtype="<u2", count=192).tolist() == [int(v) for q in want["q"] for v in q]
    assert block[384:392] == bytes([0, 1, 1, 0, 1, 1, 0, 0])


def test_huffman_block_decodes_every_code(accepted):
    """The table block's look-up and limits find every code of an optimised and of the standard tables again."""
    from dualdiff_amd.pipeline import jpeg_input as JI
    for name in ("37x53_optimize", "37x53_uniform_q75"):
        for (bits, values) in R.headers(accepted[name][0])["huffman"].values():
            blk = JI.huffman_block(bits, values)
            lut = np.frombuffer(blk, dtype="<u2", count=256)
            lim = np.frombuffer(blk, dtype="<i4", count=17, offset=512)
            off = np.frombuffer(blk, dtype="<i4", count=17, offset=580)
            vals = np.frombuffer(blk, dtype=np.uint8, count=256, offset=648)
            for (length, code), sym in R.huffman_lookup(bits, values).items():
                for fill in (0, (1 << (16 - length)) - 1):
                    c = (code << (16 - length)) | fill
                    e = int(lut[c >> 8])
                    if e:
                        assert (e >> 8, e & 255) == (length, sym)
                    else:
                        got = next(n for n in range(9, 17) if c < lim[n])
                        assert got == length > 8 and vals[off[got] + (c >> (16 - got))] == sym
            assert all(0xFFFF >= lim[n] for n in range(1, 17))                  # the all-ones pattern is in no table


def test_every_refused_kind_raises_and_names_itself(golden, accepted):
    from dualdiff_amd.pipeline import jpeg_input as JI
    good = accepted["20x32_uniform_q75"][0]
    kinds = [(k, golden["refused_" + k].tobytes(), word) for k, (_, _, word) in MI.REFUSED.items()]
    kinds += [(k, MI.rewrite(k, good), word) for k, word in MI.REWRITTEN.items()]
    assert len(kinds) == 11
    for kind, data, word in kinds:
        with pytest.raises(ValueError, match=re.escape(word)) as e:
            JI.parse_jpeg(data)
        built = kind not in ("no_sos", "no_eoi")
        assert ("is not built; available: baseline (SOF0)" in str(e.value)) == built, kind
        # as frame 1 of a batch: refused on the host, by its index, before anything is uploaded (no GPU is there to upload to)
        with pytest.raises(ValueError, match="^frame 1: .*" + re.escape(word)):
            JI.decode_jpeg([good, data, good])
        with pytest.raises(ValueError, match="^frame 3: "):
            JI.decode_jpeg([[good, good], [good, data]])
    with pytest.raises(ValueError, match="not a JPEG"):
        JI.parse_jpeg(b"\x89PNG\r\n\x1a\n" + bytes(32))
    assert "4:2:0" in JI.JPEG_INPUT_MODES and "4:4:4" in JI.JPEG_INPUT_MODES
    from dualdiff_amd import image_tables
    assert image_tables.JPEG_MODES == "baseline, 4:2:0 chroma (subsampling 2), the standard Huffman tables, quality 1..100"


def test_mixed_geometry_raises(accepted):
    from dualdiff_amd.pipeline import jpeg_input as JI
    a, b, c = accepted["20x32_uniform_q75"][0], accepted["37x53_uniform_q75"][0], accepted["8x8_444"][0]
    with pytest.raises(ValueError, match="frame 2: 37 x 53 sampling 420 differs from frame 0"):
        JI.decode_jpeg([a, a, b])
    with pytest.raises(ValueError, match="frame 1: 8 x 8 sampling 444 differs"):
        JI.decode_jpeg([accepted["8x8_uniform_q75"][0], c])
    for bad in ([], a, [[a, a], [a]], [a, "x.jpg"]):
        with pytest.raises(ValueError):
            JI.decode_jpeg(bad)


def test_cpu_tensors_raise_gpu_only(accepted, tmp_path):
    from dualdiff_amd import ops
    from dualdiff_amd.pipeline import jpeg_input as JI
    data = accepted["20x32_uniform_q75"][0]
    with pytest.raises(RuntimeError, match="GPU only"):
        JI.decode_jpeg([data], device="cpu")
    path = tmp_path / "a.jpg"
    path.write_bytes(data)
    with pytest.raises(RuntimeError, match="GPU only"):
        JI.load_jpeg([[str(path)]], device="cpu")
    scan, offsets, lengths, tables, h, w, sampling, longest = JI.upload_jpeg([data, data], "cpu", lead=3)
    assert (h, w, sampling) == (20, 32, 420) and offsets.tolist() == [3, 3 + longest] and lengths.tolist() == [longest] * 2
    assert bytes(scan[3:3 + longest].tolist()) == R.headers(data)["scan"] and tables.shape == (2, 4016)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.jpeg_decode_u8(scan, offsets, lengths, tables, h, w, sampling, longest)
    for kw in ({"h": 0}, {"w": 65536}, {"sampling": 422}, {"longest": 0}, {"rounds": 65}, {"rounds": -1}, {"h": 20.0},
               {"scan": scan.float()}, {"offsets": offsets.long()}, {"tables": tables[:, :4000]}, {"lengths": lengths[:1]}):
        a = dict(scan=scan, offsets=offsets, lengths=lengths, tables=tables, h=h, w=w, sampling=sampling, longest=longest,
                 rounds=None)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.jpeg_decode_u8(a["scan"], a["offsets"], a["lengths"], a["tables"], a["h"], a["w"], a["sampling"], a["longest"],
                               rounds=a["rounds"])


def test_python_constants_are_the_sources():
    from dualdiff_amd import _build, ops
    hdr = open(os.path.join(ROOT, "include", "dualdiff_hip.h")).read()
    hip = open(os.path.join(ROOT, "dualdiff_amd", "csrc", "jpeg_decode.hip")).read()
    core = open(os.path.join(ROOT, "dualdiff_amd", "csrc", "jpeg_decode_core.h")).read()

    def define(src, name):
        return int(re.search(r"#define %s (\d+)" % name, src).group(1))
    assert define(hdr, "DD_JPEG_SUB_BITS") == define(core, "DD_JD_SUB_BITS")
    assert "constexpr int kThreads = " in hip and "constexpr int kScanThreads = " in hip       # test_jpeg_input_gpu.py reads them
    assert int(re.search(r"sizeof\(DdJdTables\) == (\d+)", core).group(1)) == ops.JPEG_DECODE_TABLE_BYTES
    assert [define(hdr, "DD_JPEG_" + n) for n in ("EXHAUSTED", "BAD_CODE", "BAD_RUN", "TRAILING")] == [b for b, _ in ops.JPEG_DECODE_STATUS]
    assert "jpeg_decode.hip" in _build.SOURCES and "jpeg_decode.hip" not in _build.EXTRA_FLAGS
    assert "import PIL" not in open(os.path.join(ROOT, "dualdiff_amd", "pipeline", "jpeg_input.py")).read().replace(
        "does not import PIL", "")


@pytest.fixture(scope="module")
def lib():
    from dualdiff_amd import _build, _native
    if not os.path.exists(_build.lib_path()):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _native.load(build_if_missing=False)


def test_library_turns_down_bad_calls_without_a_gpu(lib):
    """DD_ERR_BAD_ARG before any runtime call, so also on a box without a GPU."""
    P = ctypes.c_void_p(4096)
    need = lib.dd_jpeg_decode_workspace_bytes(2, 20, 32, 420, 1000)
    # coefficients, planes, the stream, three states of 16 bytes and a block index per subsequence
    assert need >= 2 * (4 * 6 * 128 + 32 * 32 * 3 // 2 + 1000 + 8 * (3 * 16 + 4)) and need % 16 == 0
    assert lib.dd_jpeg_decode_workspace_bytes(6, 900, 1600, 420, 1 << 20) < 128 << 20
    for m, h, w, s, n in ((0, 8, 8, 420, 100), (-1, 8, 8, 420, 100), (1, 0, 8, 420, 100), (1, 8, 0, 420, 100),
                          (1, 65536, 8, 420, 100), (1, 8, 65536, 444, 100), (1, 8, 8, 422, 100), (1, 8, 8, 0, 100),
                          (1, 8, 8, 420, 0), (1, 8, 8, 420, -4), (1, 8, 8, 420, (1 << 27) + 1), (1, 65535, 65535, 420, 100),
                          (65536, 8, 8, 420, 100)):
        assert lib.dd_jpeg_decode_workspace_bytes(m, h, w, s, n) == -1, (m, h, w, s, n)

    def call(scan=P, scan_bytes=2000, offsets=P, lengths=P, longest=1000, tables=P, m=2, h=20, w=32, sampling=420, out=P,
             status=P, ws=P, ws_bytes=need, rounds=-1):
        return lib.dd_jpeg_decode_u8(scan, scan_bytes, offsets, lengths, longest, tables, m, h, w, sampling, out, status, ws,
                                     ws_bytes, rounds, None)
    bad = -1
    for name in ("scan", "offsets", "lengths", "tables", "out", "status", "ws"):
        assert call(**{name: None}) == bad, name
    for kw in ({"m": 0}, {"m": -3}, {"h": 0}, {"w": 0}, {"h": -8}, {"w": 65536}, {"h": 65536}, {"sampling": 422},
               {"sampling": 0}, {"scan_bytes": 0}, {"scan_bytes": -1}, {"longest": 0}, {"longest": -1}, {"rounds": -2},
               {"rounds": 65}, {"ws_bytes": need - 1}, {"ws_bytes": 0}, {"ws": ctypes.c_void_p(4100)},
               {"tables": ctypes.c_void_p(4097)}, {"offsets": ctypes.c_void_p(4098)}, {"lengths": ctypes.c_void_p(4099)},
               {"status": ctypes.c_void_p(4097)}):
        assert call(**kw) == bad, kw
    assert call(h=65535, w=65535, ws_bytes=1 << 62) == -2                    # more MCUs than one call takes
    assert call(longest=(1 << 27) + 1, ws_bytes=1 << 62) == -2               # bit positions are 32-bit


# ---- the decode core under the sanitizers -----------------------------------------------------------------------------------

def _case(data, pixels, rounds, want_status, scan=None, lead=0):
    from dualdiff_amd.pipeline import jpeg_input as JI
    info = JI.parse_jpeg(data)
    scan = data[info.scan[0]:info.scan[1]] if scan is None else scan
    head = struct.pack("<8i", info.h, info.w, info.sampling, rounds, len(scan), lead, want_status, int(pixels is not None))
    return head + JI.table_block(info) + bytes(lead) + scan + (b"" if pixels is None else np.ascontiguousarray(pixels).tobytes())


def test_decode_core_on_the_host_under_sanitizers(accepted, tmp_path):
    """tools/jpeg_decode_host_check.cpp, built with -fsanitize=address,undefined: every accepted file decodes to the
    fixture's pixels at the default rounds and at rounds = 0 (everything through the repair pass), and every broken stream
    — cut to half, cut to one byte, seeded random bytes, all FF — runs clean and reports a non-zero status."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # Is there a sanitizer runtime to link?  Asked once, with a trivial program, before any work: first with the runtimes
    # inside the program (gcc's flags; clang links them so anyway), then as the compiler links them by default.
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    for static in (["-static-libasan", "-static-libubsan"], []):
        if subprocess.run([cxx] + flags + static + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0:
            break
    else:
        pytest.skip("the compiler links no sanitizer runtime")
    exe = tmp_path / "jpeg_decode_host_check"
    build = subprocess.run([cxx] + flags + static + ["-I", os.path.join(ROOT, "include"),
                            os.path.join(ROOT, "tools", "jpeg_decode_host_check.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    cases = []
    rs = np.random.RandomState(2024)
    for name in NAMES:
        data, pix = accepted[name]
        scan = R.headers(data)["scan"]
        cases += [_case(data, pix, -1, 0), _case(data, pix, 0, 0), _case(data, pix, 1, 0, lead=1 + len(cases) % 3)]
        cases += [_case(data, None, r, 1, scan=s) for r in (-1, 0)
                  for s in (scan[:len(scan) // 2], scan[:1], rs.randint(0, 256, len(scan)).astype(np.uint8).tobytes(),
                            b"\xff" * len(scan))]
    cases.append(_case(accepted["20x32_uniform_q75"][0], None, -1, 1, scan=b""))
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<2i", 0x43484444, len(cases)) + b"".join(cases))
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=300)
    tail = "\n".join(run.stdout.splitlines()[-5:])
    assert run.returncode == 0, (run.returncode, [l for l in run.stdout.splitlines() if "FAILED" in l][:10], run.stderr[-3000:])
    assert "%d cases, 0 failed" % len(cases) in tail and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    # the flat frame's periodic stream: the rounds alone do not align it, the repair pass does
    assert re.search(r"rounds 0 .*status 0, [1-9]\d* of", run.stdout)
