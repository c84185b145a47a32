"""Image output on the GPU against the numpy restatement of PIL (tests/pil_resample_reference.py, pinned to PIL's bytes
by tests/test_image_output_cpu.py).  Everything here is integer-exact by construction — the quantisation is one fp32
multiply and a round-to-nearest-even, the resample is PIL's fixed-point arithmetic — so every comparison is
torch.equal on bytes, with no tolerance."""
import numpy as np
import pytest
import torch

from dualdiff_amd import ops
from tests import pil_resample_reference as R

pytestmark = pytest.mark.gpu

GUARD = 64


def _guarded(shape, offset):
    """A sentinel-filled uint8 `out` of `shape` inside a larger buffer, `offset` bytes into it (13: every row segment and
    image starts misaligned; 16: aligned) -> (buffer, out view)."""
    n = int(np.prod(shape))
    buf = torch.full((offset + n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    return buf, buf[offset:offset + n].view(shape)


def _guards_intact(buf, offset, n):
    return bool((buf[:offset] == 0xA5).all()) and bool((buf[offset + n:] == 0xA5).all())


# ---- quantisation -----------------------------------------------------------------------------------------------------------

def _all_values(dtype):
    one = torch.ones((), dtype=dtype).view(torch.int16).item()
    return torch.arange(one + 1, dtype=torch.int32).to(torch.int16).view(dtype)


def _as_image(vals, h, w):
    """A flat value set laid out as an (m, 3, h, w) image batch (the tail repeats the first values)."""
    per = 3 * h * w
    m = -(-vals.numel() // per)
    return torch.cat([vals, vals[:m * per - vals.numel()]]).view(m, 3, h, w)


def _fp32_values():
    g = torch.Generator().manual_seed(11)
    n = np.arange(255, dtype=np.float64)
    ties = ((n + 0.5) / 255).astype(np.float32)              # the fp32 neighbours of every rounding boundary
    near = [ties]
    lo, hi = ties, ties
    for _ in range(3):
        lo, hi = np.nextafter(lo, np.float32(-1)), np.nextafter(hi, np.float32(2))
        near += [lo, hi]
    special = torch.tensor([0.0, 1.0, 0.5, -0.0, -0.25, 1.5, 1e-30, 1.0 - 2.0 ** -24, 127.5 / 255, 3e38, -3e38])
    return torch.cat([special, torch.from_numpy(np.concatenate(near)), torch.rand(5000, generator=g),
                      torch.rand(500, generator=g) * 1.5 - 0.25])


# (values, h, w): 33 x 79 = 2607 pixels per image — no multiple of 4, so images after the first start misaligned and take
# the byte path, with a ragged last group; 28 x 100 takes the dword path throughout
QUANT = {
    "f16_odd": lambda: (_all_values(torch.float16), 33, 79),
    "bf16_aligned": lambda: (_all_values(torch.bfloat16), 28, 100),
    "f16_aligned": lambda: (_all_values(torch.float16), 16, 52),
    "f32_odd": lambda: (_fp32_values(), 21, 13),
    "f32_aligned": lambda: (_fp32_values(), 8, 32),
}


@pytest.mark.parametrize("m11", [False, True], ids=["01", "m11"])
@pytest.mark.parametrize("case", list(QUANT))
def test_image_quantize_u8(gpu, case, m11):
    vals, h, w = QUANT[case]()
    if m11:
        vals = torch.cat([vals, -vals]) if vals.dtype != torch.float32 else torch.cat([vals, -vals, vals * 2 - 1])
    x = _as_image(vals, h, w)
    ref = torch.from_numpy(R.frames(x.float().numpy(), m11=m11))
    if not m11 and vals.dtype != torch.float32:              # the rule itself, as diffusers writes it (values in [0, 1])
        assert np.array_equal(ref.numpy(), (x.float().permute(0, 2, 3, 1).numpy() * 255).round().astype("uint8"))
    for offset in (16, 13):
        buf, out = _guarded(ref.shape, offset)
        y = ops.image_quantize_u8(x.cuda(), m11=m11, out=out)
        assert y is out and torch.equal(out.cpu(), ref), (case, offset, int((out.cpu() != ref).sum()))
        assert _guards_intact(buf, offset, ref.numel())
    y = ops.image_quantize_u8(x.cuda(), m11=m11)
    assert y.dtype == torch.uint8 and y.shape == ref.shape and torch.equal(y.cpu(), ref)


# ---- resample ---------------------------------------------------------------------------------------------------------------

def _inputs(kind, m, h, w, seed):
    """(m, 3, h, w) fp32 images: seeded uniform noise (floats, not multiples of 1/255), 0/1 noise, all ones, all zeros."""
    g = torch.Generator().manual_seed(seed)
    if kind == "uniform":
        return torch.rand((m, 3, h, w), generator=g)
    if kind == "0/255":
        return torch.randint(0, 2, (m, 3, h, w), generator=g).float()
    return torch.full((m, 3, h, w), 1.0 if kind == "255" else 0.0)


KINDS = [("uniform", 0), ("0/255", 0), ("255", 0), ("0", 7)]      # (input, fill): the last one shows the pad


def _check_resample(x, size, padding, fill, offset, dtype=torch.float32):
    x = x.to(dtype)
    ref = torch.from_numpy(R.frames(x.float().numpy(), size, padding, fill))
    buf, out = _guarded(ref.shape, offset)
    y = ops.image_resample_u8(x.cuda(), size, padding, fill, out=out)
    assert y is out
    got = out.cpu()
    assert torch.equal(got, ref), (size, padding, int((got != ref).sum()), (got != ref).nonzero()[:4].tolist())
    assert _guards_intact(buf, offset, ref.numel())
    return ref


SMALL = [(hw, size, (0, 0, 0, 0)) for hw, size in R.SMALL_SHAPES] + [
    ((8, 12), (19, 31), (1, 2, 3, 0)),          # a row is 105 bytes; the pad differs on every side
    ((24, 40), (96, 160), (0, 4, 0, 0)),        # the production 4x ratio, several tiles in both directions
    ((32, 88), (67, 183), (8, 46, 8, 0)),       # the 2.08x ratio of the 256 x 704 configuration, odd sizes
    ((300, 600), (70, 141), (2, 1, 0, 3)),      # in / out just above 4: ksize 19, and a footprint that needs the 32 x 16 tile
]


@pytest.mark.parametrize("kind,fill", KINDS, ids=[k[0].replace("/", "_") for k in KINDS])
@pytest.mark.parametrize("hw,size,padding", SMALL, ids=["%dx%d_%dx%d_p%d" % (c[0] + c[1] + (sum(c[2]),)) for c in SMALL])
def test_image_resample_u8(gpu, hw, size, padding, kind, fill):
    x = _inputs(kind, 2, hw[0], hw[1], 31 + hw[0])
    _check_resample(x, size, padding, fill, offset=13)
    if kind == "uniform":
        _check_resample(x, size, padding, 255, offset=16, dtype=torch.float16)
        _check_resample(x, size, padding, fill, offset=14, dtype=torch.bfloat16)


def test_image_resample_u8_production_size(gpu):
    """One 224 x 400 -> 896 x 1600 image with the default pad (0, 4, 0, 0): uniform noise in the upper half, 0/255 noise
    in the lower."""
    (h, w), size, padding = R.PRODUCTION[0]
    x = _inputs("uniform", 1, h, w, 5)
    x[:, :, h // 2:] = _inputs("0/255", 1, h - h // 2, w, 6)
    ref = _check_resample(x, size, padding, 0, offset=16)
    assert ref.shape == (1, 900, 1600, 3) and (ref[:, :4] == 0).all()


def test_image_resample_u8_m11_and_post_process(gpu):
    """The [-1, 1] form, and ImagePostProcess on (b, n, 3, h, w) with Pad's pair form."""
    from dualdiff_amd.pipeline.image_output import ImagePostProcess
    g = torch.Generator().manual_seed(3)
    x = (torch.rand((2, 3, 3, 10, 14), generator=g) * 2.4 - 1.2).to(torch.float16)
    ref = R.frames(x.flatten(0, 1).float().numpy(), (23, 29), (2, 5, 2, 5), 0, m11=True)
    y = ops.image_resample_u8(x.flatten(0, 1).cuda(), (23, 29), [2, 5], m11=True)
    assert torch.equal(y.cpu(), torch.from_numpy(ref))
    post = ImagePostProcess(resize=(23, 29), padding=[2, 5])
    x01 = (x.float() / 2 + 0.5).clamp_(0, 1)
    y = post(x01.cuda())
    assert y.shape == (2, 3, 33, 33, 3) and torch.equal(y.flatten(0, 1).cpu(), torch.from_numpy(ref))
    raw = ImagePostProcess()(x01.cuda())
    assert raw.shape == (2, 3, 10, 14, 3)
    assert torch.equal(raw.flatten(0, 1).cpu(), torch.from_numpy(R.frames(x01.flatten(0, 1).numpy())))


# ---- decode_images ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_decode_images(gpu, dtype, monkeypatch):
    """decode_images == post(decode_latents) == the restatement on decode_latents' output copied to the host, for the
    SD-v1.5 decoder layout with device-seeded weights on (1, 2, 4, 8, 12) latents (64 x 96 images)."""
    from dualdiff_amd import tuning
    from dualdiff_amd.networks.layers import device_init_
    from dualdiff_amd.networks.vae_decoder import AutoencoderKLDecoder, decode_latents
    from dualdiff_amd.pipeline.image_output import ImagePostProcess, decode_images
    monkeypatch.setattr(tuning, "_AUTOTUNE", False)         # the library's own tile plan: no run-time sweep of new shapes
    with torch.device(gpu):
        vae = AutoencoderKLDecoder().to(dtype).eval()
    device_init_(vae, 17)
    lat = (torch.randn((1, 2, 4, 8, 12), generator=torch.Generator().manual_seed(4)) * 0.5).cuda()
    img = decode_latents(vae, lat)
    assert img.shape == (1, 2, 3, 64, 96) and img.dtype == torch.float32 and img.std().item() > 1e-3
    host = img.cpu().flatten(0, 1).numpy()
    for post, size, padding in ((ImagePostProcess(resize=(150, 201), padding=(3, 2, 1, 0)), (150, 201), (3, 2, 1, 0)),
                                (ImagePostProcess(), None, (0, 0, 0, 0))):
        ref = torch.from_numpy(R.frames(host, size, padding))
        a = decode_images(vae, lat, post)
        b = post(img)
        assert a.dtype == torch.uint8 and a.shape == (1, 2) + tuple(ref.shape[1:])
        assert torch.equal(a, b)
        assert torch.equal(a.flatten(0, 1).cpu(), ref)
    assert torch.equal(decode_images(vae, lat), ImagePostProcess()(img))


# ---- graph replay -----------------------------------------------------------------------------------------------------------

def test_resample_graph_replay(gpu):
    (h, w), size, padding = (24, 40), (96, 160), (0, 4, 0, 0)
    x = _inputs("uniform", 2, h, w, 8).cuda().half()
    out = torch.empty((2, 100, 160, 3), dtype=torch.uint8, device="cuda")
    ops.image_resample_u8(x, size, padding, out=out)        # warm-up outside the capture: builds the device tables
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.image_resample_u8(x, size, padding, out=out)
    for seed in (9, 10):
        x.copy_(_inputs("uniform" if seed == 9 else "0/255", 2, h, w, seed))
        out.fill_(0xA5)
        graph.replay()
        torch.cuda.synchronize()
        eager = ops.image_resample_u8(x, size, padding)
        assert torch.equal(out, eager)
        assert torch.equal(eager.cpu(), torch.from_numpy(R.frames(x.float().cpu().numpy(), size, padding)))
