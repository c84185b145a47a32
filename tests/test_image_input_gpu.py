"""Image input on the GPU against the restatement of the dataset transform (tests/image_input_reference.py, pinned to
PIL's bytes and torch's arithmetic by tests/test_image_input_cpu.py).  The resample is PIL's fixed-point arithmetic and
the normalisation a table built with torch's own float32 ops, rounded once to the output dtype — so every comparison is
torch.equal, with no tolerance."""
import numpy as np
import pytest
import torch

from dualdiff_amd import ops
from tests import image_input_reference as RI
from tests import pil_resample_reference as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
LAYOUTS = ["nchw", "nhwc8"]
SENTINEL = 77.0                                              # exact in every output dtype, and no pixel value
# guard elements in front of `out`: an odd count for NCHW (element alignment only), 16 bytes' worth for channels-last
FRONT = {"nchw": 3, "nhwc8": 8}
GUARD = 64


def _guarded_out(shape, dtype, layout):
    n = int(np.prod(shape))
    front = FRONT[layout]
    buf = torch.full((front + n + GUARD,), SENTINEL, dtype=dtype, device="cuda")
    return buf, buf[front:front + n].view(shape)


def _guards_intact(buf, n, layout):
    front = FRONT[layout]
    return bool((buf[:front] == SENTINEL).all()) and bool((buf[front + n:] == SENTINEL).all())


def _misaligned(frames, offset):
    """The frames `offset` bytes into a larger device buffer (torch's own allocations are 256-byte aligned)."""
    n = frames.numel()
    buf = torch.zeros((offset + n + GUARD,), dtype=torch.uint8, device="cuda")
    view = buf[offset:offset + n].view(frames.shape)
    view.copy_(frames)
    assert view.data_ptr() % 4 == offset % 4 and view.is_contiguous()
    return view


_REFS = {}


def _ref(name, hw, size, box, kind, mean_std=RI.HALF):
    """fp32 NCHW reference of a case, computed once; the other dtypes and the channels-last form derive from it."""
    key = (name, box, kind, mean_std)
    if key not in _REFS:
        frames = RI.frame(name, hw, kind, m=2)
        _REFS[key] = (frames, RI.pixel_values(frames, size, box, *mean_std))
    return _REFS[key]


def _expect(ref32, dtype, layout):
    x = ref32.to(dtype)
    return x if layout == "nchw" else RI.nhwc8(x)


def _check(frames_dev, ref32, size, box, dtype, layout, mean_std=RI.HALF):
    exp = _expect(ref32, dtype, layout)
    buf, out = _guarded_out(tuple(exp.shape), dtype, layout)
    y = ops.image_load_u8(frames_dev, size, box, mean_std[0], mean_std[1], dtype=dtype, layout=layout, out=out)
    assert y is out
    got = out.cpu()
    assert torch.equal(got, exp), (size, box, dtype, layout, int((got != exp).sum()), (got != exp).nonzero()[:4].tolist())
    assert _guards_intact(buf, exp.numel(), layout)
    if layout == "nhwc8":                                    # written as zero although the buffer held the sentinel
        assert bool((out[:, 3:] == 0).all())
    return got


@pytest.mark.parametrize("kind", RI.KINDS, ids=[k.replace("/", "_") for k in RI.KINDS])
@pytest.mark.parametrize("name,hw,size,box", RI.CASES, ids=[c[0] for c in RI.CASES])
def test_image_load_u8(gpu, name, hw, size, box, kind):
    """Every small case with its off-origin box and with the whole image, three dtypes, both layouts.  The production
    ratios (4, 1 / 0.24, 1 / 0.48) select their tile from ksize alone, so these cases run the tiles the 900 x 1600 frames
    run, over several tiles in both axes."""
    for b in (box, None):
        frames, ref32 = _ref(name, hw, size, b, kind)
        dev = torch.from_numpy(frames).cuda()
        for dtype in DTYPES:
            for layout in LAYOUTS:
                _check(dev, ref32, size, b, dtype, layout)
    y = ops.image_load_u8(dev, size)                          # defaults: fp32 NCHW, the whole image, a fresh tensor
    assert y.dtype == torch.float32 and y.shape == ref32.shape and torch.equal(y.cpu(), ref32)


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_input_at_any_byte_offset(gpu, offset):
    """The frames 1, 2 and 3 bytes off a dword boundary: the staging copy takes dwords where a row segment is aligned and
    bytes at its ends.  320 * 3 and 150 * 3 bytes per row: the second case also changes alignment from row to row."""
    for name in ("down4", "down048", "up_both"):
        _, hw, size, box = next(c for c in RI.CASES if c[0] == name)
        frames, ref32 = _ref(name, hw, size, box, "uniform")
        dev = _misaligned(torch.from_numpy(frames), offset)
        _check(dev, ref32, size, box, torch.float32, "nchw")
        _check(dev, ref32, size, box, torch.bfloat16, "nhwc8")


def test_imagenet_normalisation(gpu):
    _, hw, size, box = RI.CASES[0]
    frames, ref32 = _ref("down4", hw, size, box, "uniform", RI.IMAGENET)
    dev = torch.from_numpy(frames).cuda()
    for dtype in DTYPES:
        _check(dev, ref32, size, box, dtype, "nchw", RI.IMAGENET)
    got = _check(dev, ref32, size, box, torch.float16, "nhwc8", RI.IMAGENET)
    assert not torch.equal(got[:, 0], got[:, 1])


def test_production_size(gpu):
    """2 views of 900 x 1600 -> 224 x 400 (resize to 225 x 400, one row off the top): uniform noise in the upper half,
    0/255 noise in the lower."""
    from dualdiff_amd.pipeline.image_input import ImagePreProcess
    image_size, lim, resized, box = RI.CONFIGS[0]
    frames = R.noise_u8((2, 900, 1600, 3), "uniform", 5)
    frames[:, 450:] = R.noise_u8((2, 450, 1600, 3), "0/255", 6)
    ref32 = RI.pixel_values(frames, resized, box)
    assert ref32.shape == (2, 3, 224, 400)
    dev = torch.from_numpy(frames).cuda()
    _check(dev, ref32, resized, box, torch.float32, "nchw")
    _check(dev, ref32, resized, box, torch.bfloat16, "nhwc8")
    pre = ImagePreProcess.from_config({"dataset": {"image_size": image_size, "augment2d": {"resize": [lim]}}}, (900, 1600))
    y = pre(dev[None])
    assert y.shape == (1, 2, 3, 224, 400) and y.dtype == torch.float32 and torch.equal(y[0].cpu(), ref32)


def test_pre_process_shapes(gpu):
    from dualdiff_amd.pipeline.image_input import ImagePreProcess
    _, hw, size, box = next(c for c in RI.CASES if c[0] == "down048")
    frames, ref32 = _ref("down048", hw, size, box, "uniform")
    dev = torch.from_numpy(frames).cuda()
    pre = ImagePreProcess(resize=size, box=box, dtype=torch.float16)
    y = pre(dev.view(1, 2, *dev.shape[1:]))
    assert y.shape == (1, 2, 3) + pre.size and y.dtype == torch.float16 and torch.equal(y[0].cpu(), ref32.half())
    assert torch.equal(pre(dev), y[0])
    assert torch.equal(pre.nhwc8(dev, torch.float16).cpu(), RI.nhwc8(ref32.half()))


def test_graph_replay(gpu):
    _, hw, size, box = RI.CASES[0]
    frames = torch.from_numpy(RI.frame("down4", hw, "uniform", m=2)).cuda()
    out = torch.empty((2 * 44 * 80, 8), dtype=torch.bfloat16, device="cuda")
    ops.image_load_u8(frames, size, box, dtype=torch.bfloat16, layout="nhwc8", out=out)    # builds the tables and the LUT
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.image_load_u8(frames, size, box, dtype=torch.bfloat16, layout="nhwc8", out=out)
    for seed, kind in ((9, "uniform"), (10, "0/255")):
        host = R.noise_u8(tuple(frames.shape), kind, seed)
        frames.copy_(torch.from_numpy(host))
        out.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        eager = ops.image_load_u8(frames, size, box, dtype=torch.bfloat16, layout="nhwc8")
        assert torch.equal(out, eager)
        assert torch.equal(eager.cpu(), RI.nhwc8(RI.pixel_values(host, size, box, dtype=torch.bfloat16)))


# ---- encode_images ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_encode_images(gpu, dtype, monkeypatch):
    """encode_images == encode_pixel_values(vae, pre(frames), ...) bit for bit, for the SD-v1.5 encoder layout with
    device-seeded weights: (1, 4, 64, 96, 3) frames at ratio 0.5 -> 32 x 48 pixel values -> (1, 4, 4, 4, 6) latents, with a
    `given` mask that leaves two views out, sampled (same seeded generator on both sides) and as the mode."""
    from dualdiff_amd import tuning
    from dualdiff_amd.networks.layers import device_init_
    from dualdiff_amd.networks.vae_encoder import AutoencoderKLEncoder, encode_pixel_values
    from dualdiff_amd.pipeline.image_input import ImagePreProcess, encode_images
    monkeypatch.setattr(tuning, "_AUTOTUNE", False)         # the library's own tile plan: no run-time sweep of new shapes
    with torch.device(gpu):
        vae = AutoencoderKLEncoder().to(dtype).eval()
    device_init_(vae, 23)
    frames = torch.from_numpy(R.noise_u8((1, 4, 64, 96, 3), "uniform", 12)).cuda()
    pre = ImagePreProcess.from_config({"dataset": {"image_size": [32, 48], "augment2d": {"resize": [[0.5, 0.5]]}}}, (64, 96))
    assert pre.resize == (32, 48) and pre.box == (0, 0, 48, 32)
    px = pre(frames)
    assert px.shape == (1, 4, 3, 32, 48) and px.dtype == torch.float32
    assert torch.equal(px[0].cpu(), RI.pixel_values(frames[0].cpu().numpy(), (32, 48)))
    given = torch.tensor([[True, False, True, False]])
    for g in (given, None):
        a = encode_images(vae, frames, pre, sample_posterior=False, given=g)
        b = encode_pixel_values(vae, px, sample_posterior=False, given=g)
        assert a.shape == (1, 4, 4, 4, 6) and a.dtype == torch.float32 and torch.isfinite(a).all()
        assert torch.equal(a, b)
        a = encode_images(vae, frames, pre, generator=torch.Generator().manual_seed(3), given=g)
        b = encode_pixel_values(vae, px, generator=torch.Generator().manual_seed(3), given=g)
        assert torch.equal(a, b)
    assert (a.std() > 1e-3) and (encode_images(vae, frames, pre, given=given)[0, 1] == 0).all()
