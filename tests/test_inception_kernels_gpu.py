"""The four kernels of csrc/conv2d.hip, per element against float64 (tests/inception_reference.py).

Conv: |y - ref| <= ulp_out(ref) + E (gemm_reference.check) with E built from TAU (accumulator) and the epilogue rule
extended by the fp32 scale / shift and the 1-Lipschitz ReLU (inception_reference.bn_relu).  The BatchNorm scale is drawn
log-uniformly over four orders of magnitude with either sign, as gamma / sqrt(var + eps) of real checkpoints does.
Outputs are NaN-prefilled and wider than the slice: the slice must be fully written and its neighbours untouched.
"""
import pytest
import torch

from dualdiff_amd import ops
from tests import gemm_reference as G
from tests import inception_reference as R

pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]

# (m, h, w, cin, cout, kh, kw, stride, (pad_h, pad_w))
CONV_CASES = [
    (2, 11, 13, 3, 32, 3, 3, 2, (0, 0)),          # stem: 3 channels zero-padded to 8
    (1, 7, 9, 32, 32, 3, 3, 1, (0, 0)),
    (2, 7, 9, 32, 64, 3, 3, 1, (1, 1)),
    (2, 5, 7, 64, 80, 1, 1, 1, (0, 0)),
    (2, 6, 5, 80, 192, 3, 3, 1, (0, 0)),          # K = 720
    (2, 6, 7, 48, 64, 5, 5, 1, (2, 2)),           # K = 1200
    (1, 3, 4, 48, 64, 5, 5, 1, (2, 2)),           # image smaller than the kernel
    (2, 5, 9, 128, 128, 1, 7, 1, (0, 3)),
    (1, 4, 3, 160, 192, 1, 7, 1, (0, 3)),         # width 3 < 7
    (2, 9, 5, 160, 160, 7, 1, 1, (3, 0)),
    (1, 3, 6, 192, 192, 7, 1, 1, (3, 0)),
    (2, 9, 8, 288, 384, 3, 3, 2, (0, 0)),
    (2, 7, 7, 96, 96, 3, 3, 2, (0, 0)),
    (1, 5, 6, 192, 320, 3, 3, 2, (0, 0)),
    (2, 4, 4, 384, 384, 1, 3, 1, (0, 1)),
    (2, 4, 4, 384, 384, 3, 1, 1, (1, 0)),
    (2, 3, 5, 448, 384, 3, 3, 1, (1, 1)),
    (2, 4, 5, 1280, 448, 1, 1, 1, (0, 0)),
    (1, 3, 3, 2048, 320, 1, 1, 1, (0, 0)),        # deepest K
    (1, 1, 1, 384, 384, 1, 3, 1, (0, 1)),         # one output row
]


def _operands(case, dtype, seed):
    m, h, w, cin, cout, kh, kw, stride, pad = case
    cp = -(-cin // 8) * 8                          # the kernel's cin multiple: the stem's 3 -> 8, zero-filled on both sides
    x = torch.zeros((m * h * w, cp), dtype=dtype, device="cuda")
    x[:, :cin] = G.rand((m * h * w, cin), dtype, seed)
    wt = torch.zeros((cout, kh, kw, cp), dtype=dtype, device="cuda")
    wt[..., :cin] = G.rand((cout, kh, kw, cin), dtype, seed + 1, scale=(2.0 / (kh * kw * cin)) ** 0.5)
    g = torch.Generator().manual_seed(seed + 2)
    scale = (10.0 ** (4 * torch.rand(cout, generator=g) - 2)) * (1 - 2 * torch.randint(0, 2, (cout,), generator=g))
    shift = torch.rand(cout, generator=g) * 0.2 - 0.1
    return x, wt.reshape(cout, -1).contiguous(), scale.float().cuda(), shift.float().cuda()


def _run_conv(case, dtype, seed, relu=True, tile=None, c_off=0, extra=64):
    m, h, w, cin, cout, kh, kw, stride, pad = case
    x, wt, scale, shift = _operands(case, dtype, seed)
    acc, e_acc = R.conv_acc(x, wt, m, h, w, kh, kw, stride, pad)
    ref, e = R.bn_relu(acc, e_acc, scale, shift, relu)
    rows = ref.shape[0]
    hout, wout = ops.conv2d_out_hw(h, w, kh, kw, stride, pad)
    assert rows == m * hout * wout
    buf = G.nan_like((rows, cout + extra), dtype, "cuda")
    y = ops.conv2d(x, wt, scale, shift, m, h, w, kh, kw, stride=stride, pad=pad, relu=relu, out=buf, c_off=c_off, tile=tile)
    assert y is buf
    what = "conv2d %s %s relu=%s tile=%s c_off=%d" % (case, dtype, relu, tile, c_off)
    r = G.check(buf[:, c_off:c_off + cout], ref, e, what)
    assert bool(torch.isnan(buf[:, :c_off]).all()) and bool(torch.isnan(buf[:, c_off + cout:]).all()), \
        what + ": columns outside the slice were written"
    print("%s max err/bound %.3f" % (what, r))
    return r


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "m%d_%dx%d_%dto%d_k%dx%d_s%d_p%d%d" % (c[:8] + c[8]))
def test_conv2d_cases(gpu, case, dtype):
    _run_conv(case, dtype, 100 + CONV_CASES.index(case))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile,case", [("64x64", (1, 5, 13, 64, 80, 1, 1, 1, (0, 0))),       # 65 rows: one past the tile
                                       ("128x64", (1, 3, 43, 64, 80, 1, 1, 1, (0, 0))),     # 129 rows
                                       ("128x64", (1, 9, 9, 48, 64, 5, 5, 1, (2, 2))),      # 81 rows in a 128-row tile
                                       ("64x64", (3, 7, 7, 96, 96, 3, 3, 2, (0, 0)))])
def test_conv2d_tile_edges(gpu, tile, case, dtype):
    _run_conv(case, dtype, 300, tile=tile)


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv2d_relu_off(gpu, dtype):
    _run_conv((2, 7, 9, 32, 64, 3, 3, 1, (1, 1)), dtype, 310, relu=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv2d_channel_offset(gpu, dtype):
    """A branch's slice inside a concatenated tensor: offset 32, buffer 96 columns wider than the slice."""
    _run_conv((2, 6, 7, 48, 64, 5, 5, 1, (2, 2)), dtype, 320, c_off=32, extra=96)


def test_conv2d_kernel_name_follows_the_tile(gpu):
    assert "64, 64" in ops.conv2d_kernel_name(3200, 320)
    assert "128, 64" in ops.conv2d_kernel_name(61250, 96)
    assert "128, 64" in ops.conv2d_kernel_name(10, 64, tile="128x64")
    assert "__bf16" in ops.conv2d_kernel_name(10, 64, torch.bfloat16)


# ---- pools ---------------------------------------------------------------------------------------------------------------

def _pool(mode, m, h, w, c, dtype, seed, c_off=8, extra=24):
    x = G.rand((m * h * w, c), dtype, seed)
    ref = R.pool3x3(x, m, h, w, mode)
    buf = G.nan_like((ref.shape[0], c + extra), dtype, "cuda")
    ops.pool3x3(x, m, h, w, mode, out=buf, c_off=c_off)
    assert bool(torch.isnan(buf[:, :c_off]).all()) and bool(torch.isnan(buf[:, c_off + c:]).all())
    return buf[:, c_off:c_off + c], ref


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode,h,w", [("max_s2", 7, 9), ("max_s2", 8, 8), ("max_s2", 3, 3),
                                      ("max_s1", 5, 4), ("max_s1", 1, 1), ("max_s1", 2, 3)])
def test_max_pool_is_bit_exact(gpu, mode, h, w, dtype):
    y, ref = _pool(mode, 2, h, w, 24, dtype, 400 + h * 10 + w)
    assert torch.equal(y, ref.to(dtype)), (mode, h, w)        # a maximum of storage values is a storage value


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h,w", [(5, 4), (1, 1), (2, 3)])
def test_exclusive_avg_pool_within_one_ulp(gpu, h, w, dtype):
    """fp32 sum of <= 9 storage values / an integer is within a few 2^-24 relative of exact, so the stored value is the
    correctly rounded one or its neighbour: corners divide by 4, edges by 6, the 1 x 1 image by 1."""
    y, ref = _pool("avg_s1", 2, h, w, 24, dtype, 450 + h * 10 + w)
    err = (y.to(torch.float64) - ref).abs()
    assert bool((err <= G.ulp(ref, dtype)).all()), float((err / G.ulp(ref, dtype)).max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h,w", [(1, 1), (8, 8), (3, 5)])
def test_global_avgpool(gpu, h, w, dtype):
    m, c = 3, 40
    x = G.rand((m * h * w, c), dtype, 500 + h * w)
    y = ops.global_avgpool(x, m, h * w)
    assert y.dtype == torch.float32 and y.shape == (m, c)
    ref = R.global_avgpool(x, m, h * w)
    bound = h * w * 2.0 ** -24 * x.to(torch.float64).abs().reshape(m, h * w, c).mean(dim=1)
    err = (y.to(torch.float64) - ref).abs()
    assert bool((err <= bound).all()), float((err / bound).max())


# ---- input ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("src,size,resize", [((20, 33), (299, 299), True), ((5, 4), (7, 9), True),
                                             ((9, 7), (4, 5), True), ((6, 11), None, False)])
def test_inception_input(gpu, src, size, resize, dtype):
    """Bound: the fp32 evaluation lies within e of the float64 value (inception_reference.inception_input: the coordinate
    terms from the source index range, the lerp and 2 x - 1 on values in [-1, 1]); the store rounds it by half a unit of
    the storage type at a magnitude <= |ref| + e."""
    m = 2
    x = R.seeded_images((m, 3) + src, 600 + src[0]).cuda()
    y = ops.inception_input(x, size or src, resize=resize, dtype=dtype)
    ref, e = R.inception_input(x.cpu(), size, resize=resize)
    ref, e = ref.cuda(), e.cuda()
    assert y.shape == (ref.shape[0], 8) and y.dtype == dtype
    assert bool((y[:, 3:] == 0).all()), "padded channels must be exactly zero"
    bound = 0.5 * G.ulp(ref.abs() + e, dtype) + e
    err = (y[:, :3].to(torch.float64) - ref).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    assert float(ref.min()) >= -1.0 and float(ref.max()) <= 1.0


@pytest.mark.parametrize("in_dtype", [torch.float16, torch.bfloat16])
def test_inception_input_takes_16_bit_images(gpu, in_dtype):
    x = R.seeded_images((1, 3, 5, 4), 610).to(in_dtype).cuda()
    y = ops.inception_input(x, (7, 9), dtype=torch.float16)
    ref, e = R.inception_input(x.cpu(), (7, 9))
    bound = 0.5 * G.ulp(ref.abs() + e, torch.float16) + e
    assert bool(((y[:, :3].cpu().to(torch.float64) - ref).abs() <= bound).all())
