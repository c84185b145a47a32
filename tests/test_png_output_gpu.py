"""PNG output on the GPU against the reference encoder of the format (tests/png_reference.py) and its decoder-side checker.
A lossless format has no tolerance: every device file must (a) pass the checker and unfilter to exactly the input, and (b)
equal the reference encoder's bytes.  The inputs come from tests/png_cases.py and the fixture alone."""
import functools

import numpy as np
import pytest
import torch

from dualdiff_amd import ops
from tests import png_cases as C
from tests import png_reference as R

pytestmark = pytest.mark.gpu

CASES = C.cases()


@functools.lru_cache(maxsize=None)
def _golden():
    z = np.load(C.GOLDEN)
    return {k: z[k] for k in z.files}


def _files(buf, lengths):
    n = lengths.cpu().tolist()
    raw = buf.cpu().numpy()
    return [raw[i, :min(k, raw.shape[1])].tobytes() for i, k in enumerate(n)], n


def _encode(frames, **kw):
    """-> (files, lengths) at the default capacity, the worst case of the format"""
    return _files(*ops.png_encode_u8(torch.from_numpy(np.array(frames)).cuda(), **kw))


def _first_difference(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


def _verify(name, img, got, n):
    want, _ = C.reference(name)
    print("%s: device %d bytes, reference %d, worst case %d" % (name, n, len(want), R.worst_case(*img.shape[:2])))
    assert n == len(got) <= R.worst_case(*img.shape[:2])
    pixels, types = R.check(got)                                             # (a)
    assert np.array_equal(pixels, img)
    assert types.tolist() == R.choose_filters(img).tolist()
    assert n == len(want)                                                    # (b)
    assert got == want, "first difference at byte %d of %d" % (_first_difference(got, want), len(want))


def _verify_size(name, img, n, noise):
    if noise:
        return
    model, pil0 = R.model_size(img), int(_golden()["pil_" + name][1])
    print("%s: %d bytes, model %d (+%.2f %%, margin %d %%), PIL level 0 %d" % (name, n, model, 100.0 * (n / model - 1), C.MARGINS[name], pil0))
    assert n <= model * (1 + C.MARGINS[name] / 100.0)
    assert n < pil0


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_equals_reference_and_decodes(gpu, case):
    assert np.array_equal(_golden()["in_" + case.name], case.img)
    (got,), (n,) = _encode(case.img[None])
    _verify(case.name, case.img, got, n)
    _verify_size(case.name, case.img, n, case.noise)


def test_noise_is_stored_within_the_worst_case(gpu):
    img = next(c.img for c in CASES if c.name == "noise_64x100")
    (got,), (n,) = _encode(img[None])
    assert n == R.worst_case(64, 100) == ops.png_capacity(64, 100)
    at = 0
    for kind, payload in R.parse(got)[1:-1]:                                 # every IDAT: a stored block of its chunk
        body = payload[2:] if at == 0 else payload
        k = min(R.CHUNK, 64 * 301 - at)
        assert body[0] in (0, 1) and int.from_bytes(body[1:3], "little") == k == int.from_bytes(body[3:5], "little") ^ 0xFFFF
        at += k
    assert at == 64 * 301


def test_frames_of_one_call(gpu):
    """7 frames of mixed content in one call: each equals its single-frame result byte for byte."""
    frames = C.batch()
    files, lengths = _encode(frames)
    for i in range(len(frames)):
        (one,), (n,) = _encode(frames[i:i + 1])
        assert lengths[i] == n == len(one)
        assert files[i] == one == R.encode(frames[i]), i
        assert np.array_equal(R.check(files[i])[0], frames[i])


def test_large_frame(gpu):
    """900 x 1600, half smooth gradient, half noise: 264 chunks, dynamic and stored."""
    img = C.large()
    (got,), (n,) = _encode(img[None])
    _verify("large", img, got, n)
    _verify_size("large", img, n, False)


def test_capacity(gpu):
    """A row of half the file's size: the length is the true one, the row is the file's first bytes, nothing behind the
    buffer is touched."""
    frames = torch.from_numpy(np.stack([C._mixed(37, 53, 31), C.batch()[0]])).cuda()
    full, n = _files(*ops.png_encode_u8(frames))
    assert [len(f) for f in full] == n and n[1] > n[0]
    for cap in (n[0] // 2, n[0] - 1, n[0], n[0] + 3, 51):
        guard = 256
        store = torch.full((2 * cap + guard,), 0xA5, dtype=torch.uint8, device="cuda")
        out = store[:2 * cap].view(2, cap)
        buf, lengths = ops.png_encode_u8(frames, out=out)
        assert buf.data_ptr() == out.data_ptr() and lengths.cpu().tolist() == n
        raw = out.cpu().numpy()
        for i in range(2):
            assert raw[i, :min(cap, n[i])].tobytes() == full[i][:cap]
            assert bool((out[i, min(cap, n[i]):] == 0xA5).all())             # the rest of a row that fits is untouched
        assert bool((store[2 * cap:] == 0xA5).all())
    with pytest.raises(ValueError, match="capacity"):
        ops.png_encode_u8(frames, capacity=50)


def test_decode_images_then_save(gpu, monkeypatch, tmp_path):
    """decode_images -> concat_views -> save_png on a 3 x 5 latent writes files the checker accepts."""
    from dualdiff_amd import tuning
    from dualdiff_amd.networks.layers import device_init_
    from dualdiff_amd.networks.vae_decoder import AutoencoderKLDecoder
    from dualdiff_amd.pipeline.image_output import concat_views, decode_images, encode_png, save_png
    monkeypatch.setattr(tuning, "_AUTOTUNE", False)
    with torch.device(gpu):
        vae = AutoencoderKLDecoder().to(torch.float16).eval()
    device_init_(vae, 17)
    lat = (torch.randn((1, 6, 4, 3, 5), generator=torch.Generator().manual_seed(4)) * 0.5).cuda()
    frames = decode_images(vae, lat)
    assert frames.shape == (1, 6, 24, 40, 3)
    grid = concat_views(frames)
    assert grid.shape == (1, 48, 120, 3)
    host = grid.cpu().numpy()
    paths = [str(tmp_path / "out" / "0_gen0.png")]
    assert save_png(grid, paths) == [len(R.encode(host[0]))]
    data = open(paths[0], "rb").read()
    assert data == R.encode(host[0]) and np.array_equal(R.check(data)[0], host[0])
    nested = encode_png(frames)
    assert len(nested) == 1 and len(nested[0]) == 6
    views = frames.cpu().numpy()
    for v in range(6):
        assert np.array_equal(R.check(nested[0][v])[0], views[0, v])
    line = concat_views(frames, oneline=True)
    assert np.array_equal(R.check(encode_png(line)[0])[0], line.cpu().numpy()[0])
    with pytest.raises(ValueError, match="one path per frame"):
        save_png(grid, paths + paths)


def test_files_open_in_pil(gpu):
    Image = pytest.importorskip("PIL.Image")
    import io
    for case in CASES[::4]:
        (got,), _ = _encode(case.img[None])
        pil = Image.open(io.BytesIO(got))
        pil.load()
        assert pil.mode == "RGB" and pil.format == "PNG" and np.array_equal(np.array(pil), case.img), case.name


def test_graph_replay(gpu):
    """The four launches captured after a warm-up and replayed on new frame content give the eager bytes."""
    h, w = 45, 80
    frames = torch.from_numpy(np.stack([C._mixed(h, w, 1), C._mixed(h, w, 2)])).cuda()
    out = torch.empty((2, ops.png_capacity(h, w)), dtype=torch.uint8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with ops.workspace_owner("png-graph-test"):              # one scratch buffer for the warm-up and the capture stream
        ops.png_encode_u8(frames, out=out)                   # warm-up outside the capture: the workspace
        torch.cuda.synchronize()
        with torch.cuda.graph(graph):
            _, lengths = ops.png_encode_u8(frames, out=out)
    for seed in (9, 10):
        new = np.stack([C.MJ.content("uniform" if seed == 9 else "lone", h, w, seed), C._mixed(h, w, seed)])
        frames.copy_(torch.from_numpy(new))
        out.fill_(0xA5)
        graph.replay()
        torch.cuda.synchronize()
        files, n = _files(out, lengths)
        eager, ne = _files(*ops.png_encode_u8(frames))
        assert n == ne and files == eager
        assert files == [R.encode(f) for f in new]


def test_two_runs_are_identical(gpu):
    frames = torch.from_numpy(np.stack([C._mixed(128, 85, 6), C.MJ.content("uniform", 128, 85, 1)])).cuda()
    a, la = ops.png_encode_u8(frames)
    b, lb = ops.png_encode_u8(frames)
    torch.cuda.synchronize()
    assert torch.equal(la, lb)
    fa, _ = _files(a, la)
    fb, _ = _files(b, lb)
    assert fa == fb and fa[0] == C.reference("128x85_two_chunks")[0]


def test_misaligned_frames_and_timer(gpu):
    """Frames that start at an odd address (a `frames[1:]`-like view into a larger buffer) encode to the same bytes, and
    under a KernelTimer the call is booked as one entry with its traffic."""
    img = C._mixed(37, 53, 41)
    store = torch.zeros((2, 37, 53, 3), dtype=torch.uint8, device="cuda")
    store[1].copy_(torch.from_numpy(img))
    frames = store[1:]
    assert frames.data_ptr() % 4 == 3 and frames.is_contiguous()             # 37 * 53 * 3 = 5883 bytes per frame
    timer = ops.KernelTimer()
    ops.set_timer(timer)
    try:
        files, _ = _files(*ops.png_encode_u8(frames))
    finally:
        ops.set_timer(None)
    assert files == [R.encode(img)]
    booked = timer.summary()
    assert set(booked) == {"dd_png_encode"} and booked["dd_png_encode"]["count"] == 1
    assert booked["dd_png_encode"]["bytes"] == 2 * img.size + 2 * 37 * (1 + 3 * 53)
