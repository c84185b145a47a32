"""JPEG output on the GPU against PIL's bytes (tests/golden/jpeg_output.npz) and against the numpy restatement of libjpeg
(tests/jpeg_reference.py, pinned to PIL by tests/test_jpeg_output_cpu.py).  The encoder is integer arithmetic from the
pixels to the last bit, so every comparison is equality of bytes, with no tolerance."""
import functools

import numpy as np
import pytest
import torch

from dualdiff_amd import ops
from tests import jpeg_reference as J
from tests.golden import mint_jpeg as M

pytestmark = pytest.mark.gpu

CASES = list(M.cases())
LARGE = (528, 520)                       # 33 x 33 = 1089 MCUs: more than the scan's 1024 threads, a 166 KB stream


@functools.lru_cache(maxsize=None)
def _golden():
    z = np.load(M.PATH)
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _large(kind):
    """(frame, the restatement's file) of the large case; computed once, shared and never written to."""
    img = M.content(kind, LARGE[0], LARGE[1], 77)
    img.setflags(write=False)
    return img, J.encode(img, 75)


def _files(buf, lengths):
    n = lengths.cpu().tolist()
    raw = buf.cpu().numpy()
    return [raw[i, :min(k, raw.shape[1])].tobytes() for i, k in enumerate(n)], n


def _encode(frames, quality=75, capacity=None):
    """-> (files, lengths).  The rows are sized for any content (the default capacity, header + H * W, is not: test_capacity)."""
    if capacity is None:
        capacity = 1024 + 3 * frames.shape[1] * frames.shape[2]
    return _files(*ops.jpeg_encode_u8(torch.from_numpy(np.array(frames)).cuda(), quality, capacity=capacity))


def _first_difference(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


@pytest.mark.parametrize("name,quality,img", CASES, ids=[c[0] for c in CASES])
def test_equals_pil_bytes(gpu, name, quality, img):
    want = _golden()["out_" + name].tobytes()
    assert np.array_equal(_golden()["in_" + name], img)
    (got,), (n,) = _encode(img[None], quality, capacity=len(want))          # a row that fits exactly
    assert n == len(want)
    assert got == want, "first difference at byte %d of %d" % (_first_difference(got, want), len(want))


@pytest.mark.parametrize("count,shape", [(6, (20, 32)), (7, (37, 53)), (6, (90, 160))])
def test_frames_of_one_call(gpu, count, shape):
    """Several frames in one call, different content per frame: each equals its single-frame result (per-frame offsets
    into the workspace, the output rows and the lengths)."""
    kinds = ("uniform", "saturated", "smooth", "lone", "flat", "tiles", "uniform")
    frames = np.stack([M.content(kinds[i], shape[0], shape[1], 900 + i) for i in range(count)])
    files, lengths = _encode(frames)
    for i in range(count):
        (one,), (n,) = _encode(frames[i:i + 1])
        assert lengths[i] == n == len(one)
        assert files[i] == one == J.encode(frames[i], 75), i


@pytest.mark.parametrize("kind", ["uniform", "saturated"])
def test_large_frame(gpu, kind):
    """More MCUs than the scan workgroup has threads, and many stuffing chunks."""
    img, want = _large(kind)
    (got,), (n,) = _encode(img[None])
    assert n == len(want) and len(want) > 8 * 4096
    assert got == want, "first difference at byte %d of %d" % (_first_difference(got, want), len(want))


def test_capacity(gpu):
    """A row of half the file's size: the length is the true one, the row is the file's first bytes, nothing behind the
    buffer is touched; encode_jpeg repeats the call and returns the whole files."""
    from dualdiff_amd.pipeline import image_output as IO
    frames = torch.from_numpy(np.stack([M.content("uniform", 37, 53, 31), M.content("smooth", 37, 53, 32)])).cuda()
    full, n = _files(*ops.jpeg_encode_u8(frames, capacity=8192))
    assert [len(f) for f in full] == n
    cap = n[0] // 2
    guard = 256
    store = torch.full((2 * cap + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    out = store[:2 * cap].view(2, cap)
    buf, lengths = ops.jpeg_encode_u8(frames, out=out)
    assert buf.data_ptr() == out.data_ptr() and lengths.cpu().tolist() == n
    raw = out.cpu().numpy()
    for i in range(2):
        assert raw[i, :min(cap, n[i])].tobytes() == full[i][:cap]
    assert bool((store[2 * cap:] == 0xA5).all())
    if n[1] < cap:                                           # the smooth frame fits: the rest of its row is untouched
        assert bool((out[1, n[1]:] == 0xA5).all())
    # the default capacity does not hold a file of noise at quality 100 on a frame this small
    noisy = M.content("uniform", 8, 8, 5)[None]
    header_len = len(IO.jpeg_header(8, 8, 100))
    want = J.encode(noisy[0], 100)
    assert len(want) > header_len + 64
    short, (k,) = _files(*ops.jpeg_encode_u8(torch.from_numpy(noisy).cuda(), 100))
    assert k == len(want) and short == [want[:header_len + 64]]
    assert IO.encode_jpeg(torch.from_numpy(noisy).cuda(), 100) == [want]
    with pytest.raises(ValueError, match="capacity"):
        ops.jpeg_encode_u8(frames, capacity=10)


def test_decode_images_then_encode(gpu, monkeypatch, tmp_path):
    """decode_images -> encode_jpeg / save_jpeg on a small synthetic latent == the restatement on the same frames."""
    from dualdiff_amd import tuning
    from dualdiff_amd.networks.layers import device_init_
    from dualdiff_amd.networks.vae_decoder import AutoencoderKLDecoder
    from dualdiff_amd.pipeline.image_output import ImagePostProcess, decode_images, encode_jpeg, save_jpeg
    monkeypatch.setattr(tuning, "_AUTOTUNE", False)
    with torch.device(gpu):
        vae = AutoencoderKLDecoder().to(torch.float16).eval()
    device_init_(vae, 17)
    lat = (torch.randn((1, 2, 4, 8, 12), generator=torch.Generator().manual_seed(4)) * 0.5).cuda()
    frames = decode_images(vae, lat, ImagePostProcess(resize=(90, 130), padding=(0, 4, 0, 0)))
    assert frames.shape == (1, 2, 94, 130, 3)
    host = frames.cpu().numpy()
    want = [[J.encode(host[0, v], 75) for v in range(2)]]
    files = encode_jpeg(frames)
    assert files == want
    assert encode_jpeg(frames.flatten(0, 1)) == want[0]
    paths = [[str(tmp_path / "samples" / "CAM_FRONT" / "a.jpg"), str(tmp_path / "samples" / "CAM_BACK" / "b.jpg")]]
    assert save_jpeg(frames, paths) == [[len(f) for f in want[0]]]
    for p, f in zip(paths[0], want[0]):
        assert open(p, "rb").read() == f


def test_files_open_in_pil(gpu):
    Image = pytest.importorskip("PIL.Image")
    import io
    for name, quality, img in CASES[::5]:
        (got,), _ = _encode(img[None], quality)
        pil = Image.open(io.BytesIO(got))
        pil.load()
        assert pil.size == (img.shape[1], img.shape[0]) and pil.mode == "RGB" and pil.format == "JPEG", name


def test_graph_replay(gpu):
    """The six launches captured after a warm-up and replayed on new frame content give the eager bytes."""
    h, w = 45, 80
    frames = torch.from_numpy(np.stack([M.content("uniform", h, w, 1), M.content("smooth", h, w, 2)])).cuda()
    out = torch.empty((2, 1024 + 3 * h * w), dtype=torch.uint8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with ops.workspace_owner("jpeg-graph-test"):             # one scratch buffer for the warm-up and the capture stream
        ops.jpeg_encode_u8(frames, out=out)                  # warm-up outside the capture: tables and workspace
        torch.cuda.synchronize()
        with torch.cuda.graph(graph):
            _, lengths = ops.jpeg_encode_u8(frames, out=out)
    for seed, kinds in ((9, ("saturated", "lone")), (10, ("smooth", "uniform"))):
        new = np.stack([M.content(k, h, w, seed + i) for i, k in enumerate(kinds)])
        frames.copy_(torch.from_numpy(new))
        out.fill_(0xA5)
        graph.replay()
        torch.cuda.synchronize()
        files, n = _files(out, lengths)
        eager, ne = _files(*ops.jpeg_encode_u8(frames, capacity=out.shape[1]))
        assert n == ne and files == eager
        assert files == [J.encode(f, 75) for f in new]


def test_two_runs_are_identical(gpu):
    img, want = _large("uniform")
    frames = torch.from_numpy(np.stack([img, M.content("saturated", LARGE[0], LARGE[1], 78)])).cuda()
    a, la = ops.jpeg_encode_u8(frames, capacity=3 * LARGE[0] * LARGE[1])
    b, lb = ops.jpeg_encode_u8(frames, capacity=3 * LARGE[0] * LARGE[1])
    torch.cuda.synchronize()
    assert torch.equal(la, lb)
    fa, _ = _files(a, la)
    fb, _ = _files(b, lb)
    assert fa == fb and fa[0] == want


def test_misaligned_frames_and_timer(gpu):
    """Frames that start at an odd address (a view into a larger buffer) encode to the same bytes, and under a
    KernelTimer the call is booked as one entry with its traffic."""
    img = M.content("uniform", 37, 53, 41)
    store = torch.zeros(img.size + 7, dtype=torch.uint8, device="cuda")
    frames = store[3:3 + img.size].view(1, 37, 53, 3)
    frames.copy_(torch.from_numpy(img))
    assert frames.data_ptr() % 4 == 3
    timer = ops.KernelTimer()
    ops.set_timer(timer)
    try:
        files, _ = _files(*ops.jpeg_encode_u8(frames, capacity=8192))
    finally:
        ops.set_timer(None)
    assert files == [J.encode(img, 75)]
    booked = timer.summary()
    assert set(booked) == {"dd_jpeg_encode"} and booked["dd_jpeg_encode"]["count"] == 1
    assert booked["dd_jpeg_encode"]["bytes"] == img.size + 3 * 768 * 3 * 4
