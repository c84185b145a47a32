"""VAE encode on the HIP path: the Downsample2D(padding=0) conv (dd_gemm_conv_pad, pad_lo = 0) and the posterior kernel
against fp64, the encoder against the CPU restatement (tests/vae_encoder_reference.py — parity unpinned, weights
seeded), encode_pixel_values on a scene, and given-view sampling started from pixel values.

Encoder rule, as for the decoder (tests/test_vae_gpu.py):  e(HIP) <= max(1e-3, 1.5 * e_floor)  with e_floor the error of
the restatement run with every module output rounded to the storage dtype."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

from dualdiff_amd import _native, ops
from oracle.init_utils import seeded_state_dict, seeded_tensor
from oracle.numerics import storage_emulation
from tests import gemm_reference as G
from tests import vae_encoder_reference as RE
from tests.gemm_reference import bound, check, epilogue  # noqa: F401
from tests.golden import cases as C
from tests.test_parity_r02_gpu import _denoiser, _to_dev, step_models  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, os.cpu_count() or 1))

DTYPES = [torch.float16, torch.bfloat16]
_DTC = {torch.float16: _native.DD_F16, torch.bfloat16: _native.DD_BF16}


# ---- Downsample2D(padding=0) conv against fp64 ---------------------------------------------------------------------------

def pad0_conv_acc(x, w, m, hin, win):
    """F.pad(x, (0, 1, 0, 1)) then a 3x3 / stride 2 / pad 0 conv of the NHWC batch x, as nine fp64 tap matmuls.
    Returns (acc, E_acc) in gemm_reference's form."""
    cin, cout = x.shape[1], w.shape[0]
    hout, wout = (hin - 2) // 2 + 1, (win - 2) // 2 + 1
    xp = F.pad(x.to(torch.float64).reshape(m, hin, win, cin), (0, 0, 0, 1, 0, 1))     # zero row / column at the end
    W = w.to(torch.float64).reshape(cout, 3, 3, cin)
    acc = torch.zeros((m * hout * wout, cout), dtype=torch.float64, device=x.device)
    n2 = torch.zeros((m * hout * wout,), dtype=torch.float64, device=x.device)
    for ky in range(3):
        for kx in range(3):
            tap = xp[:, ky:ky + 2 * (hout - 1) + 1:2, kx:kx + 2 * (wout - 1) + 1:2, :].reshape(-1, cin)
            acc += tap @ W[:, ky, kx, :].t()
            n2 += (tap * tap).sum(dim=1)
    return acc, G.TAU * torch.outer(n2.sqrt(), w.to(torch.float64).norm(dim=1))


class Pad0Case:
    def __init__(self, m, hin, win, cin, cout, dtype, seed):
        self.m, self.hin, self.win, self.cin, self.cout, self.dtype = m, hin, win, cin, cout, dtype
        self.hout, self.wout = (hin - 2) // 2 + 1, (win - 2) // 2 + 1
        self.rows = m * self.hout * self.wout
        self.x = G.rand((m * hin * win, cin), dtype, seed + 1)
        self.w = G.rand((cout, 9 * cin), dtype, seed + 2, (9 * cin) ** -0.5)
        self.bias = G.rand((cout,), dtype, seed + 3, 0.5)
        with torch.no_grad():
            self.ref, self.e = epilogue(*pad0_conv_acc(self.x, self.w, m, hin, win), bias=self.bias)

    def run(self, tile=0, split=0):
        out = torch.full((self.rows, self.cout), float("nan"), dtype=self.dtype, device="cuda")
        y = ops.conv3x3(self.x, self.w, self.bias, self.m, self.hin, self.win, stride=2, pad=0, out=out, tile=tile,
                        split_k=split)
        return check(y, self.ref, self.e, "pad0 conv %s tile %d split %d" % ((self.m, self.hin, self.win, self.cin,
                                                                               self.cout), tile, split))

    def desc(self, tile, split, pad_lo):
        d = _native.GemmDesc()
        d.rows, d.n, d.k, d.k1, d.conv, d.stride = self.rows, self.cout, 9 * self.cin, 9 * self.cin, 1, 2
        d.hin, d.win, d.cin, d.hv, d.wv, d.hout, d.wout = self.hin, self.win, self.cin, self.hin, self.win, self.hout, self.wout
        d.tile, d.split_k, d.dtype = tile, split, _DTC[self.dtype]
        d.a = d.w = d.out = 1 << 20
        d.alpha = 1.0
        return d


# (m, hin, win, cin, cout): the three encoder downsamples at m = 2, odd sizes, ragged row counts
PAD0 = [(2, 224, 400, 128, 128), (2, 112, 200, 256, 256), (2, 56, 100, 512, 512), (2, 27, 51, 64, 64),
        (3, 13, 9, 128, 192), (1, 2, 3, 64, 72)]
SWEEP = [(2, 56, 100, 512, 512), (2, 27, 51, 64, 64), (3, 13, 9, 128, 192), (1, 2, 3, 64, 72)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", PAD0, ids=["%dx%dx%dx%d_%d" % s for s in PAD0])
def test_pad0_conv_against_fp64(gpu, shape, dtype):
    case = Pad0Case(*shape, dtype, sum(shape))
    worst = case.run()                                              # the tuned launch conv3x3(pad=0) makes
    if shape in SWEEP:
        lib = _native.load()
        d = case.desc(0, 0, 0)
        n = 0
        for tile, split in ops.tune_candidates(lib, d):
            d.tile, d.split_k = tile, split
            if lib.dd_gemm_conv_pad_kernel_name(ctypes.byref(d), 0).decode() == "unsupported":
                continue
            worst = max(worst, case.run(tile, split))
            n += 1
        assert n >= 5
    print("\n[pad0 conv %s %s] max err/bound %.3f" % (shape, dtype, worst))


@pytest.mark.parametrize("dtype", DTYPES)
def test_pad1_entry_is_bit_identical_to_dd_gemm(gpu, dtype):
    """conv3x3 (pad 1, stride 1 and 2) through dd_gemm_conv_pad(pad_lo = 1) and through dd_gemm: same bits."""
    lib = _native.load()
    for (m, hin, win, cin, cout, stride), tile, split in (((2, 28, 50, 128, 128, 2), 1, 1), ((2, 28, 50, 128, 128, 2), 15, 3),
                                                          ((2, 28, 50, 320, 320, 1), 39, 1), ((6, 14, 25, 64, 64, 2), 0, 0)):
        x = G.rand((m * hin * win, cin), dtype, 11)
        w = G.rand((cout, 9 * cin), dtype, 12, (9 * cin) ** -0.5)
        b = G.rand((cout,), dtype, 13)
        hout, wout = (hin - 1) // stride + 1, (win - 1) // stride + 1
        outs = []
        for entry in ("dd_gemm", "dd_gemm_conv_pad"):
            out = torch.full((m * hout * wout, cout), float("nan"), dtype=dtype, device="cuda")
            d = _native.GemmDesc()
            d.a, d.w, d.bias, d.out = x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr()
            d.lda, d.ldc, d.alpha = cin, cout, 1.0
            d.rows, d.n, d.k, d.k1, d.conv, d.stride = m * hout * wout, cout, 9 * cin, 9 * cin, 1, stride
            d.hin, d.win, d.cin, d.hv, d.wv, d.hout, d.wout = hin, win, cin, hin, win, hout, wout
            d.tile, d.split_k, d.dtype = tile, split, _DTC[dtype]
            need = lib.dd_gemm_workspace_bytes(ctypes.byref(d))
            assert need == lib.dd_gemm_conv_pad_workspace_bytes(ctypes.byref(d), 1)
            if need:
                ws = ops.workspace(need, x.device)
                d.ws, d.ws_bytes = ws.data_ptr(), ws.numel() * 4
            rc = lib.dd_gemm(ctypes.byref(d), ops._stream()) if entry == "dd_gemm" else \
                lib.dd_gemm_conv_pad(ctypes.byref(d), 1, ops._stream())
            assert rc == 0, (entry, rc)
            outs.append(out)
        assert torch.equal(outs[0], outs[1])
        assert not torch.isnan(outs[0]).any()


# ---- posterior against fp64 ------------------------------------------------------------------------------------------------

U = 2.0 ** -24


def posterior_ref(moments, wq, bq, noise, scale):
    """fp64 quant_conv + DiagonalGaussianDistribution and the bound of the kernel's fp32 arithmetic: the 8-term FMA chain
    (<= 16 u of sum |w x| + |b|), the clamp (1-Lipschitz), expf and the products (a few u each)."""
    x = moments.double()
    p = x @ wq.double().t() + bq.double()
    ep = 16 * U * ((x.abs() @ wq.double().abs().t()) + bq.double().abs())
    mean, e = p[:, :4], ep[:, :4]
    z = mean
    if noise is not None:
        nz = noise.double().permute(0, 2, 3, 1).reshape(-1, 4)
        sd = torch.exp(0.5 * p[:, 4:].clamp(-30, 20))
        esd = sd * (0.5 * ep[:, 4:] * torch.exp(0.5 * ep[:, 4:]) + 4 * U)
        z = mean + sd * nz
        e = e + nz.abs() * esd + 2 * U * (mean.abs() + (sd * nz).abs())
    return scale * z, abs(scale) * e + U * (scale * z).abs()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("out_f32", [True, False])
def test_posterior_against_fp64(gpu, dtype, out_f32):
    m, h, w = 3, 28, 50
    g = torch.Generator().manual_seed(5)
    mom = torch.randn((m * h * w, 8), generator=g)
    mom[:, 4:] = torch.rand((m * h * w, 4), generator=g) * 70 - 40           # logvar over [-40, 30]: both clamps hit
    mom = mom.to(dtype)
    wq = torch.randn((8, 8), generator=g) * 0.05
    wq[4:, 4:] += torch.eye(4)
    bq = torch.randn((8,), generator=g) * 0.1
    noise = torch.randn((m, 4, h, w), generator=g).to(dtype)
    lv = (mom.double() @ wq.double().t() + bq.double())[:, 4:]
    assert (lv < -30).any() and (lv > 20).any()
    scale = 0.18215
    for nz in (None, noise):
        y = ops.vae_posterior(mom.cuda(), wq.cuda(), bq.cuda(), m, h, w, noise=None if nz is None else nz.cuda(),
                              scale=scale, out_f32=out_f32)
        assert y.shape == (m, 4, h, w) and y.dtype == (torch.float32 if out_f32 else dtype)
        ref, e = posterior_ref(mom, wq, bq, nz, scale)
        yy = y.cpu().permute(0, 2, 3, 1).reshape(-1, 4)
        r = check(yy, ref, e, "posterior %s out_f32=%s %s" % (dtype, out_f32, "mode" if nz is None else "sample"),
                  torch.float32 if out_f32 else dtype)
        print("[posterior %s f32=%s %s] max err/bound %.3f" % (dtype, out_f32, "mode" if nz is None else "sample", r))


# ---- encoder against the restatement ---------------------------------------------------------------------------------------

def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def rel_l2(y, ref):
    y, ref = y.detach().float().cpu(), ref.detach().float().cpu()
    return ((y - ref).norm() / (ref.norm() + 1e-20)).item()


@pytest.fixture(scope="module")
def enc_case(gpu):
    ora = RE.AutoencoderKLEncoder().eval()
    sd = {k: bf16_round(v) for k, v in seeded_state_dict(ora, 41).items()}
    ora.load_state_dict(sd)
    return ora, sd, {}


def _hip(case, dtype):
    from dualdiff_amd.networks.vae_encoder import AutoencoderKLEncoder
    ora, sd, nets = case
    if dtype not in nets:
        net = AutoencoderKLEncoder()
        net.load_state_dict(sd, strict=True)
        nets[dtype] = net.to("cuda", dtype).eval()
    return nets[dtype]


def _pixels(shape, seed):
    return bf16_round(seeded_tensor(shape, seed, 0.6).clamp(-1, 1))


def _bound(name, y, ref, emul, dtype):
    e, fl = rel_l2(y, ref), rel_l2(emul, ref)
    b = max(1e-3, 1.5 * fl)
    print("%-34s %-8s e_hip=%.3e e_floor=%.3e bound=%.3e" % (name, str(dtype).split(".")[-1], e, fl, b))
    assert torch.isfinite(y.float()).all()
    assert e <= b, (name, e, fl)
    return b


_MOMENTS = {}


def _ref_moments(ora, x, key, dtype=None):
    k = (key, dtype)
    if k not in _MOMENTS:
        with torch.no_grad():
            if dtype is None:
                _MOMENTS[k] = ora(x)
            else:
                with storage_emulation(ora, dtype):
                    _MOMENTS[k] = ora(x)
    return _MOMENTS[k]


@pytest.mark.parametrize("dtype", DTYPES)
def test_encoder_two_views(enc_case, dtype):
    """2 views of 96 x 160: every layer of the encoder, the three pad-0 downsamples, the 240-token attention; mode() and
    sample(generator) with the same seeded noise on both sides."""
    ora = enc_case[0]
    x = _pixels((2, 3, 96, 160), 3)
    ref_m, emul_m = _ref_moments(ora, x, "2v"), _ref_moments(ora, x, "2v", dtype)
    dist = _hip(enc_case, dtype).encode(x.cuda().to(dtype)).latent_dist
    y = dist.mode()
    assert y.shape == (2, 4, 12, 20) and y.dtype == dtype
    _bound("encode mode 2x96x160", y, RE.posterior(ref_m), RE.posterior(emul_m), dtype)
    y = dist.sample(torch.Generator().manual_seed(9))
    noise = torch.randn((2, 4, 12, 20), generator=torch.Generator().manual_seed(9), dtype=dtype).float()
    _bound("encode sample 2x96x160", y, RE.posterior(ref_m, noise), RE.posterior(emul_m, noise), dtype)


_SCENE_BOUND = {}


def test_encoder_full_size_view(enc_case):
    """One 224 x 400 view in bf16 (1400 attention tokens, the workload's size)."""
    ora, dtype = enc_case[0], torch.bfloat16
    x = _pixels((1, 3, 224, 400), 4)
    ref_m, emul_m = _ref_moments(ora, x, "1v"), _ref_moments(ora, x, "1v", dtype)
    y = _hip(enc_case, dtype).encode(x.cuda().to(dtype)).latent_dist.mode()
    _SCENE_BOUND[dtype] = _bound("encode mode 1x224x400", y, RE.posterior(ref_m), RE.posterior(emul_m), dtype)


def test_encode_pixel_values_scene(enc_case):
    """(1, 6, 3, 224, 400) in fp32 -> (1, 6, 4, 28, 50) fp32 latents; one view alone and a `given` subset agree with their
    slices of the whole scene within the 224 x 400 case's bound; a seeded generator reproduces the sample bit for bit."""
    from dualdiff_amd.networks.vae_encoder import SCALING_FACTOR, encode_pixel_values
    dtype = torch.bfloat16
    vae = _hip(enc_case, dtype)
    px = _pixels((1, 6, 3, 224, 400), 8).cuda()
    full = encode_pixel_values(vae, px, sample_posterior=False)
    assert full.shape == (1, 6, 4, 28, 50) and full.dtype == torch.float32 and torch.isfinite(full).all()
    b = _SCENE_BOUND.get(dtype, 1e-2)
    one = encode_pixel_values(vae, px[:, 4:5], sample_posterior=False)
    assert rel_l2(one[0, 0], full[0, 4]) <= b
    given = torch.tensor([[True, False, False, True, False, True]])
    sub = encode_pixel_values(vae, px, sample_posterior=False, given=given)
    assert sub.shape == full.shape
    assert (sub[0, ~given[0].cuda()] == 0).all()
    for v in (0, 3, 5):
        assert rel_l2(sub[0, v], full[0, v]) <= b
    mode = vae.encode(px[0].to(dtype)).latent_dist.mode().float() * SCALING_FACTOR
    assert rel_l2(full[0], mode) <= 1e-2
    s1 = encode_pixel_values(vae, px, generator=torch.Generator().manual_seed(3))
    s2 = encode_pixel_values(vae, px, generator=torch.Generator().manual_seed(3))
    assert torch.equal(s1, s2) and not torch.equal(s1, full)


# ---- given views from images ----------------------------------------------------------------------------------------------

def test_given_views_from_pixel_values(step_models, enc_case):
    """Views 0 and 3 encoded from seeded pixel values become the given views of the full-width two-branch step model:
    after set_inputs they hold add_noise(clean, n0, t0) within 1 ulp, and a 2-step run ends finite."""
    from dualdiff_amd.networks.vae_encoder import encode_pixel_values
    from dualdiff_amd.pipeline.pipeline_bev_controlnet import BEVDenoiser
    from tests.given_view_reference import alphas_cumprod
    dtype = torch.bfloat16
    H, W, NCAM = C.H, C.W, C.N_CAM
    vae = _hip(enc_case, dtype)
    px = _pixels((1, NCAM, 3, 8 * H, 8 * W), 12).cuda()
    given = torch.zeros((1, NCAM), dtype=torch.bool)
    given[0, 0] = given[0, 3] = True
    lat = encode_pixel_values(vae, px, generator=torch.Generator().manual_seed(2), given=given)
    assert lat.shape == (1, NCAM, 4, H, W)
    d = _denoiser(step_models, dtype, use_graph=False)
    den = BEVDenoiser(d.unet, d.controlnets, guidance_scale=2.0, num_inference_steps=50, sampler="ddim")
    inp = C.step_inputs(2)
    with torch.no_grad():
        den.set_inputs(C.step_latents().cuda().to(dtype), _to_dev(inp["text"], dtype), _to_dev(inp["camera_param"], dtype),
                       [_to_dev(inp["boxes_bg"], dtype), _to_dev(inp["boxes_fg"], dtype)],
                       [_to_dev(inp["cond_bg"], dtype), _to_dev(inp["cond_fg"], dtype)],
                       conditional_latents=lat, conditional_mask=given)
    acp = alphas_cumprod()
    t0 = int(den.timesteps[0])
    n0 = C.step_latents().to(dtype).double()[0]
    x = den.latents[0].double().cpu()
    c = lat[0].double().cpu()
    for v in (0, 3):
        ref = acp[t0].sqrt() * c[v] + (1 - acp[t0]).sqrt() * n0[v]
        bnd = G.ulp(ref, dtype) + 2.0 ** -20 * (c[v].abs() + n0[v].abs())
        assert ((x[v] - ref).abs() <= bnd).all(), v
    with torch.no_grad():
        den.run(2)
    assert torch.isfinite(den.latents.float()).all()
