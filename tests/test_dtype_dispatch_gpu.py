"""The (entry point, element type) pairs of the launchers' dtype dispatch that no other GPU test takes.

Every 16-bit-only launcher, the three image launchers, dd_fourier_embed with equal types and dd_fourier_embed_strided with
a 16-bit output run in each of their types elsewhere in the suite (test_ops_gpu, test_tokens_gpu, test_norm_fp64_gpu,
test_given_view_ops_gpu, test_text_encoder_gpu, test_fp8_mfma_gpu, test_vae_gpu, test_vae_encoder_gpu,
test_image_input_gpu, test_image_output_gpu, test_attention_fp64_gpu).  What is left are type PAIRS of the nested
dispatches:
  dd_fourier_embed          input type != output type (six pairs; ops.fourier_embed only asks for equal types, so these go
                            to the library directly, on the stream and pointers ops would pass)
  dd_fourier_embed_strided  fp32 output from each of the three input types (ops.camera_features)
  dd_box_tokens             fp16 points with bf16 tokens and bf16 points with fp16 tokens (ops.box_tokens)
A dispatch arm that launched the wrong instantiation would read bf16 bits as fp16 (1.0 becomes 1.875) or halve the
element stride: wrong by far more than any rounding.

Reference: the Fourier features of the rounded inputs, in fp32 on the host.  The kernels round each value to the input
type and then to the output type, one relative ulp-sized step each at most, so the bound is the coarser of the two types'
tolerances of test_ops_gpu.test_fourier_embed, times max(1, largest reference magnitude) as there.  Coordinates are of
order 1, so the bound resolves the sines and cosines themselves.  What is only copied (class tokens) is compared exactly."""
import ctypes
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
TOL = {F32: 2e-5, F16: 1e-3, BF16: 8e-3}                   # test_ops_gpu.test_fourier_embed
FREQS = [1.0, 2.0, 4.0, 8.0]


def rnd(shape, dtype, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def features(x):
    """[x | sin f0 x | cos f0 x | ...] on the last dim, fp32 (networks/embedder.py)."""
    x = x.float()
    return torch.cat([x] + [fn(x * f) for f in FREQS for fn in (torch.sin, torch.cos)], dim=-1)


def close(y, ref, in_dtype, out_dtype, what):
    tol = max(TOL[in_dtype], TOL[out_dtype]) * max(ref.abs().max().item(), 1.0)
    err = (y.float().cpu() - ref).abs().max().item()
    assert err <= tol, "%s %s -> %s: max err %.3e > %.3e" % (what, in_dtype, out_dtype, err, tol)


@pytest.mark.parametrize("in_dtype,out_dtype", [p for p in itertools.product((F16, BF16, F32), repeat=2) if p[0] != p[1]])
def test_fourier_embed_mixed_types(gpu, in_dtype, out_dtype):
    from dualdiff_amd import _native, ops
    x = rnd((37, 3), in_dtype, 1)
    xd = x.cuda()
    out = torch.full((37, 27), float("nan"), dtype=out_dtype, device="cuda")
    arr = (ctypes.c_float * len(FREQS))(*FREQS)
    rc = _native.load().dd_fourier_embed(ops._ptr(xd), ops._ptr(out), 37, 3, arr, len(FREQS), 1, ops._FDT[in_dtype],
                                         ops._FDT[out_dtype], ops._stream())
    assert rc == 0
    close(out, features(x), in_dtype, out_dtype, "fourier_embed")


@pytest.mark.parametrize("in_dtype", [F16, BF16, F32])
def test_camera_features_fp32_output(gpu, in_dtype):
    from dualdiff_amd import ops
    cam = rnd((2, 6, 3, 7), in_dtype, 2)
    out = ops.camera_features(cam.cuda(), FREQS, True, F32, 192)
    assert out.shape == (12, 192) and out.dtype == F32 and not out[:, 189:].any()
    close(out[:, :189], features(cam.permute(0, 1, 3, 2)).reshape(12, 189), in_dtype, F32, "camera_features")


@pytest.mark.parametrize("pts_dtype,dtype", [(F16, BF16), (BF16, F16)])
def test_box_tokens_mixed_types(gpu, pts_dtype, dtype):
    from dualdiff_amd import ops
    rows, npts, ctd, ncls = 5, 8, 16, 4
    pts = (torch.rand((rows, npts, 3), generator=torch.Generator().manual_seed(3)) * 2 - 1).to(pts_dtype)
    table, null_cls = rnd((ncls, ctd), dtype, 4).cuda(), rnd((ctd,), dtype, 5).cuda()
    null_pos = rnd((npts * 27,), dtype, 6).cuda()
    classes = torch.tensor([3, 0, 2, 1, 2], device="cuda")
    masks = torch.tensor([True, True, False, True, True], device="cuda")
    pos = torch.full((rows, npts * 27), float("nan"), dtype=dtype, device="cuda")
    cat = torch.zeros((rows, 2 * ctd), dtype=dtype, device="cuda")
    ops.box_tokens(pts.cuda(), classes, masks, table, null_pos, null_cls, FREQS, True, pos, cat, ctd)
    ref = features(pts).reshape(rows, npts * 27)
    ref[2] = null_pos.float().cpu()
    close(pos, ref, pts_dtype, dtype, "box_tokens pos")
    want = table[classes]
    want[2] = null_cls
    assert torch.equal(cat[:, ctd:], want) and not cat[:, :ctd].any()
