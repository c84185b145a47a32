"""JPEG input on the GPU against PIL's pixels (tests/golden/jpeg_input.npz) and against the numpy restatement of libjpeg's
decoder (tests/jpeg_decode_reference.py, pinned to PIL by tests/test_jpeg_input_cpu.py).  The decoder is integer arithmetic
from the first bit to the pixels, so every comparison is equality of bytes, with no tolerance.  The broken streams fed here
rest on the bounds that test_jpeg_input_cpu.py::test_decode_core_on_the_host_under_sanitizers checks on the host."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from dualdiff_amd import ops
from dualdiff_amd.pipeline import jpeg_input as JI
from tests import jpeg_decode_reference as R
from tests import jpeg_reference as J
from tests.golden import mint_jpeg as M
from tests.golden import mint_jpeg_input as MI

pytestmark = pytest.mark.gpu

NAMES = [c[0] for c in M.cases()] + list(MI.NEW)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source_int(path, pattern):
    return int(re.search(pattern, open(os.path.join(ROOT, path)).read()).group(1))


# the kernels' constants, from where they are defined
SUB_BITS = _source_int("include/dualdiff_hip.h", r"#define DD_JPEG_SUB_BITS (\d+)")              # bits of a stream per lane
LANES = _source_int("dualdiff_amd/csrc/jpeg_decode.hip", r"constexpr int kThreads = (\d+);")     # lanes per workgroup of the decode passes
SCAN_THREADS = _source_int("dualdiff_amd/csrc/jpeg_decode.hip", r"constexpr int kScanThreads = (\d+);")   # ... of the prefix sums
# The smallest square frame with more MCUs than the prefix sums' workgroup has threads: 33 x 33 MCUs of 16 x 16 pixels, the
# last row and column one pixel wide.  Its stream of noise spans more than three workgroups of the decode passes (asserted).
LARGE = 16 * math.isqrt(SCAN_THREADS) + 1


@functools.lru_cache(maxsize=None)
def _accepted():
    return {name: (data, pix) for name, data, pix in MI.accepted(*MI.load())}


@functools.lru_cache(maxsize=None)
def _want(data):
    """The restatement's pixels of a file: computed once per file, shared and never written to."""
    pix = R.decode(data)
    pix.setflags(write=False)
    return pix


@functools.lru_cache(maxsize=None)
def _large(kind):
    data = J.encode(M.content(kind, LARGE, LARGE, 77), 75)
    return data, _want(data)


def _decode(files, rounds=None, lead=0, out=None):
    scan, offsets, lengths, tables, h, w, sampling, longest = JI.upload_jpeg(files, "cuda", lead=lead)
    frames, status = ops.jpeg_decode_u8(scan, offsets, lengths, tables, h, w, sampling, longest, rounds=rounds, out=out)
    return frames, status


def _same(frames, want):
    return torch.equal(frames.cpu(), torch.from_numpy(np.array(want)))


def _batch(shape):
    """Files of one shape with a different content kind, quality and table kind per frame; flat and tiles among them."""
    h, w = shape
    acc = _accepted()
    files = [J.encode(M.content(kind, h, w, 900 + i), q)
             for i, (kind, q) in enumerate((("flat", 75), ("tiles", 100), ("uniform", 30), ("smooth", 95), ("lone", 75)))]
    files.append(acc["%dx%d_optimize" % shape][0])           # written by PIL with optimised Huffman tables
    if shape == (37, 53):
        files.append(acc["37x53_uniform_q1"][0])
    return files


@pytest.mark.parametrize("name", NAMES)
def test_equals_pil_pixels(gpu, name):
    data, want = _accepted()[name]
    frames, status = _decode([data])
    assert frames.shape == (1,) + want.shape and frames.dtype == torch.uint8 and status.tolist() == [0]
    assert _same(frames[0], want), "%d bytes differ" % int((frames[0].cpu().numpy() != want).sum())


@pytest.mark.parametrize("shape", [(3, 1), (9, 3), (17, 4), (6, 5)])
def test_narrow_frames(gpu, shape):
    """4:2:0 frames one to four pixels wide: libjpeg replicates a chroma plane of one or two columns 2 x 2 and runs the
    triangle filter only from three columns on (width 5).  Three frames per call, against the restatement."""
    files = [J.encode(M.content(kind, shape[0], shape[1], 950 + i), q)
             for i, (kind, q) in enumerate((("uniform", 75), ("saturated", 95), ("smooth", 50)))]
    frames, status = _decode(files)
    assert status.tolist() == [0, 0, 0]
    for i, f in enumerate(files):
        assert _same(frames[i], _want(f)), i


@pytest.mark.parametrize("shape", [(20, 32), (37, 53)])
def test_frames_of_one_call(gpu, shape):
    """Several frames in one call: each equals its single-frame result and the restatement (per-frame offsets into the
    upload, the tables, the workspace and the output).  The flat and the tiles frame are periodic streams."""
    files = _batch(shape)
    assert len(files) == (6 if shape == (20, 32) else 7)
    frames, status = _decode(files)
    assert status.tolist() == [0] * len(files)
    for i, f in enumerate(files):
        one, st = _decode([f])
        assert st.tolist() == [0] and torch.equal(frames[i], one[0]) and _same(one[0], _want(f)), i


def test_rounds_do_not_change_the_frames(gpu):
    """rounds = 0 sends every subsequence through the repair pass, rounds = 1 most of the flat frame's."""
    for files in (_batch((37, 53)), [J.encode(M.content("flat", 90, 160, 5), 75), J.encode(M.content("uniform", 90, 160, 6), 75)]):
        default, status = _decode(files)
        assert status.tolist() == [0] * len(files)
        for i, f in enumerate(files):
            assert _same(default[i], _want(f)), i
        for rounds in (0, 1, 7):
            got, st = _decode(files, rounds=rounds)
            assert st.tolist() == [0] * len(files) and torch.equal(got, default), rounds


@pytest.mark.parametrize("lead", [1, 2, 3])
def test_scan_bytes_at_any_byte_offset(gpu, lead):
    files = _batch((20, 32))
    scan, offsets, *_ = JI.upload_jpeg(files, "cuda", lead=lead)
    assert (scan.data_ptr() + int(offsets[0])) % 4 == lead
    frames, status = _decode(files, lead=lead)
    assert status.tolist() == [0] * len(files)
    for i, f in enumerate(files):
        assert _same(frames[i], _want(f)), i


@pytest.mark.parametrize("kind", ["uniform", "flat"])
def test_large_frame(gpu, kind):
    """More MCUs than a prefix-sum workgroup has threads and, for noise, a stream over more than three workgroups of the
    decode passes; the flat frame of that size is one long periodic stream."""
    data, want = _large(kind)
    assert math.ceil(LARGE / 16) ** 2 > SCAN_THREADS >= math.ceil((LARGE - 16) / 16) ** 2
    if kind == "uniform":
        assert 8 * len(R.headers(data)["scan"]) > 3 * LANES * SUB_BITS
    frames, status = _decode([data])
    assert status.tolist() == [0]
    assert _same(frames[0], want), "%d bytes differ" % int((frames[0].cpu().numpy() != want).sum())


def test_round_trip_with_the_encoder(gpu):
    from dualdiff_amd.pipeline.image_output import encode_jpeg
    frames = torch.from_numpy(np.stack([np.stack([M.content(k, 45, 80, 40 + i) for i, k in enumerate(kinds)])
                                        for kinds in (("uniform", "smooth", "lone"), ("saturated", "flat", "tiles"))])).cuda()
    files = encode_jpeg(frames)
    back = JI.decode_jpeg(files)
    assert back.shape == frames.shape and back.dtype == torch.uint8 and back.is_cuda
    for b in range(2):
        for v in range(3):
            assert _same(back[b, v], _want(files[b][v])), (b, v)
    assert torch.equal(JI.decode_jpeg(files[1]), back[1])


def test_load_jpeg_and_nesting(gpu, tmp_path):
    files = _batch((20, 32))
    paths = []
    for i, f in enumerate(files):
        paths.append(tmp_path / ("cam%d.jpg" % i))
        paths[-1].write_bytes(f)
    flat = JI.load_jpeg([str(p) for p in paths])
    nested, status = JI.load_jpeg([paths[:3], paths[3:]], check=False)
    assert flat.shape == (6, 20, 32, 3) and nested.shape == (2, 3, 20, 32, 3) and status.shape == (2, 3)
    assert torch.equal(nested.flatten(0, 1), flat) and int(status.abs().sum()) == 0
    for i, f in enumerate(files):
        assert _same(flat[i], _want(f))


def test_nothing_is_written_outside_the_frames(gpu):
    files = _batch((37, 53))
    n, guard = len(files) * 37 * 53 * 3, 4099
    store = torch.full((n + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    out = store[guard:guard + n].view(len(files), 37, 53, 3)
    frames, status = _decode(files, out=out)
    assert frames.data_ptr() == out.data_ptr() and status.tolist() == [0] * len(files)
    assert bool((store[:guard] == 0xA5).all()) and bool((store[guard + n:] == 0xA5).all())
    for i, f in enumerate(files):
        assert _same(out[i], _want(f)), i


def test_a_truncated_file_between_two_good_ones(gpu):
    good = _batch((37, 53))
    data = good[2]
    info = JI.parse_jpeg(data)
    cut = data[:info.scan[0] + (info.scan[1] - info.scan[0]) // 2] + b"\xff\xd9"
    files = [good[0], cut, good[3]]
    with pytest.raises(ValueError, match="^frame 1: .*exhausted"):
        JI.decode_jpeg(files)
    frames, status = JI.decode_jpeg(files, check=False)
    st = status.tolist()
    assert st[0] == 0 and st[2] == 0 and st[1] & 1
    assert _same(frames[0], _want(good[0])) and _same(frames[2], _want(good[3]))
    # noise and all-FF bytes in place of a scan: an invalid code or a run past 63, the neighbours untouched
    rs = np.random.RandomState(7)
    n = info.scan[1] - info.scan[0]
    for scan in (rs.randint(0, 256, n).astype(np.uint8).tobytes().replace(b"\xff\xd9", b"\xff\x00"), b"\xff" * n, b"\x00"):
        bad = data[:info.scan[0]] + scan + b"\xff\xd9"
        frames, status = JI.decode_jpeg([good[0], bad, good[3]], check=False)
        st = status.tolist()
        assert st[0] == 0 and st[2] == 0 and st[1] != 0
        assert _same(frames[0], _want(good[0])) and _same(frames[2], _want(good[3]))


def test_two_runs_are_identical(gpu):
    files = [_large("uniform")[0], _large("flat")[0]]
    a, sa = _decode(files)
    b, sb = _decode(files)
    assert torch.equal(a, b) and sa.tolist() == sb.tolist() == [0, 0]
    assert _same(a[0], _large("uniform")[1]) and _same(a[1], _large("flat")[1])


def test_one_library_call_per_batch(gpu, monkeypatch):
    from dualdiff_amd import _native
    lib = _native.load()
    calls = []
    real = lib.dd_jpeg_decode_u8

    class Spy:
        def __getattr__(self, name):
            return getattr(lib, name)

        def dd_jpeg_decode_u8(self, *a):
            calls.append(a[6])                               # m
            return real(*a)
    monkeypatch.setattr(_native, "load", lambda *a, **kw: Spy())
    files = _batch((20, 32))
    frames = JI.decode_jpeg([files[:3], files[3:]])
    assert calls == [6] and frames.shape == (2, 3, 20, 32, 3)
    timer = ops.KernelTimer()
    ops.set_timer(timer)
    try:
        JI.decode_jpeg(files)
    finally:
        ops.set_timer(None)
    booked = timer.summary()
    assert calls == [6, 6] and set(booked) == {"dd_jpeg_decode"} and booked["dd_jpeg_decode"]["count"] == 1
