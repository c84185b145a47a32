"""Self-test of the fp64 reference / error bound in norm_reference.py (CPU only).

`emulate_groupnorm` is the GroupNorm kernels' arithmetic in fp32 torch: sums of d = x - pivot and d^2 in one pass, mean =
pivot + sum / n, var = max(sumsq / n - (sum / n)^2, 0), rsqrt, then sc = rstd gamma, sh = beta - mean sc, y = x sc + sh
(+ SiLU).  `emulate_layernorm` is the two-pass form of both LayerNorm kernels.  The bound must pass them and a correctly
rounded fp64 result on every data kind and both types, and must fail every fault below, injected one at a time."""
import pytest
import torch

from tests import norm_reference as N

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
M = 2
# hw, c, groups: 10 channels per group (vectors straddle groups), 4 (two whole groups per vector), 80 (a group of 10 vectors)
GN_SHAPES = [(91, 320, 32), (28, 128, 32), (97, 160, 16), (37, 2560, 32)]
LN_SHAPES = [(33, 320), (9, 1280), (5, 8), (7, 520), (5, 2048)]


def emulate_groupnorm(x, gamma, beta, m, hw, groups, eps, silu, *, pixel_weight=None, stat_group=None, pivot=True,
                      use_eps=True):
    """-> the fp32 result (m * hw, c) before its rounding.  pixel_weight (hw,): how often each pixel enters the
    statistics (1 everywhere in the kernel); stat_group (c,): the group each channel's sums are added to (its own in the
    kernel); pivot False: the textbook E[x^2] - mean^2; use_eps False: rsqrt(var)."""
    c = x.shape[1]
    cpg = c // groups
    X = x.float().reshape(m, hw, c)
    own = torch.arange(c) // cpg
    sg = own if stat_group is None else stat_group
    w = torch.ones(hw) if pixel_weight is None else pixel_weight.float()
    piv = X[:, 0, ::cpg] if pivot else torch.zeros((m, groups))              # (m, groups)
    d = X - piv[:, sg][:, None, :]
    cs = (d * w[None, :, None]).sum(dim=1)                                    # per channel, over the pixels
    cq = (d * d * w[None, :, None]).sum(dim=1)
    s = torch.zeros((m, groups)).index_add_(1, sg, cs)
    q = torch.zeros((m, groups)).index_add_(1, sg, cq)
    inv_n = torch.tensor(1.0 / (float(hw) * float(cpg)), dtype=torch.float32)
    dm = s * inv_n
    var = torch.clamp(q * inv_n - dm * dm, min=0.0)
    mean = piv + dm
    rstd = torch.rsqrt(var + torch.tensor(eps if use_eps else 0.0, dtype=torch.float32))
    sc = rstd[:, own] * gamma.float()[None, :]                                # (m, c)
    sh = beta.float()[None, :] - mean[:, own] * sc
    y = X * sc[:, None, :] + sh[:, None, :]
    if silu:
        y = y * torch.sigmoid(y)
    return y.reshape(m * hw, c)


def emulate_layernorm(x, gamma, beta, eps, *, skip_last_vector=False, use_eps=True):
    X = x.float()
    c = X.shape[1]
    S = X[:, :-8] if skip_last_vector else X
    mean = S.sum(dim=1, keepdim=True) / float(c)
    var = ((S - mean) ** 2).sum(dim=1, keepdim=True) / float(c)
    rstd = torch.rsqrt(var + torch.tensor(eps if use_eps else 0.0, dtype=torch.float32))
    return (X - mean) * rstd * gamma.float()[None, :] + beta.float()[None, :]


def _gn(kind, shape, dtype, silu, eps=1e-5, seed=3):
    hw, c, groups = shape
    x = N.groupnorm_data(kind, M, hw, c, groups, dtype, seed, "cpu")
    gamma, beta = N.affine(c, dtype, seed + 1, "cpu")
    ref, e = N.groupnorm_reference(x, gamma, beta, M, hw, groups, eps, silu)
    return x, gamma, beta, ref, e


def _ratio(y, ref, e):
    """(max err / bound, share of elements outside it) — for the messages; NaN counts as outside."""
    r = torch.nan_to_num((y.to(torch.float64) - ref).abs() / (N.ulp(ref, y.dtype) + e), nan=float("inf"))
    return float(r.max()), float((r > 1).float().mean())


def _fails(y, ref, e, what, min_ratio=1.0):
    with pytest.raises(AssertionError, match="outside the bound"):
        N.check(y, ref, e, what)
    r, share = _ratio(y, ref, e)
    print("  fault  %-58s max err/bound %9.3g   outside %5.1f %%" % (what, r, 100 * share))
    assert r >= min_ratio, "%s: err / bound %.3g, expected at least %.3g" % (what, r, min_ratio)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("silu", [False, True], ids=["plain", "silu"])
@pytest.mark.parametrize("kind", N.KINDS)
@pytest.mark.parametrize("shape", GN_SHAPES, ids=lambda s: "hw%d_c%d_g%d" % s)
def test_groupnorm_bound_passes_correct_results(dtype, silu, kind, shape):
    hw, c, groups = shape
    for eps in (1e-5, 1e-6):
        x, gamma, beta, ref, e = _gn(kind, shape, dtype, silu, eps)
        N.check(ref.to(dtype), ref, e, "correctly rounded")
        y = emulate_groupnorm(x, gamma, beta, M, hw, groups, eps, silu).to(dtype)
        r = N.check(y, ref, e, "emulation")
        assert r <= 0.75, "the emulation's own error should be output rounding (0.5), got %.3f of the bound" % r
        if kind == "const":
            ok, val = N.settled(ref, e, dtype)
            assert float(ok.float().mean()) > 0.9 and torch.equal(y[ok], val[ok])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", N.KINDS)
@pytest.mark.parametrize("shape", LN_SHAPES, ids=lambda s: "%dx%d" % s)
def test_layernorm_bound_passes_correct_results(dtype, kind, shape):
    rows, c = shape
    for eps in (1e-5, 1e-6):
        x = N.layernorm_data(kind, rows, c, dtype, 5, "cpu")
        gamma, beta = N.affine(c, dtype, 6, "cpu")
        ref, e = N.layernorm_reference(x, gamma, beta, eps)
        N.check(ref.to(dtype), ref, e, "correctly rounded")
        y = emulate_layernorm(x, gamma, beta, eps).to(dtype)
        r = N.check(y, ref, e, "emulation")
        assert r <= 0.75, "the emulation's own error should be output rounding (0.5), got %.3f of the bound" % r
        if kind == "const":
            ok, val = N.settled(ref, e, dtype)
            assert float(ok.float().mean()) > 0.9 and torch.equal(y[ok], val[ok])


def test_bound_is_not_vacuous():
    """E stays a fraction of the output unit: on randn data the bound is within 25 % of one unit of the output type."""
    for dtype in DTYPES:
        x, gamma, beta, ref, e = _gn("randn", (91, 320, 32), dtype, False)
        share = float((e / (N.ulp(ref, dtype) + e)).median())
        assert share < 0.25, share


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("silu", [False, True], ids=["plain", "silu"])
@pytest.mark.parametrize("kind", ["randn", "offset", "spike"])
def test_bound_catches_each_groupnorm_statistics_fault(dtype, silu, kind):
    """hw = 91, c = 320: 910 elements per group, 10 channels per group.  A pixel left out, a pixel counted twice, a seam
    channel added to the neighbouring group."""
    shape = (91, 320, 32)
    hw, c, groups = shape
    x, gamma, beta, ref, e = _gn(kind, shape, dtype, silu)
    emu = lambda **kw: emulate_groupnorm(x, gamma, beta, M, hw, groups, 1e-5, silu, **kw).to(dtype)
    N.check(emu(), ref, e, "correct")
    w = torch.ones(hw)
    w[hw - 1] = 0.0
    _fails(emu(pixel_weight=w), ref, e, "%s %s: last pixel left out" % (kind, dtype))
    w = torch.ones(hw)
    w[hw // 2] = 2.0
    _fails(emu(pixel_weight=w), ref, e, "%s %s: pixel %d counted twice" % (kind, dtype, hw // 2))
    sg = torch.arange(c) // (c // groups)
    sg[9] = 1                        # vector 1 holds channels 8-9 of group 0 and 10-15 of group 1
    _fails(emu(stat_group=sg), ref, e, "%s %s: channel 9 counted in group 1" % (kind, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", GN_SHAPES, ids=lambda s: "hw%d_c%d_g%d" % s)
def test_bound_catches_missing_pivot_on_offset_data(shape, dtype):
    """E[x^2] - mean^2 at |mean| ~ 100 sigma loses ~13 of the 24 bits of the variance.  fp16: 7 to 34 times the bound on
    10 - 25 % of the elements.  bf16: the output unit is eight times wider and the fault stays NEAR the bound for the
    small groups, 2 to 8 times it on about 1 % of the elements (13 to 28 times at 80 channels per group); this emulation
    shows it outside for every shape and seed tried, so that much is asserted for bf16 and no more.  On randn / spike
    data the fault is invisible in both types (norm_reference's docstring)."""
    hw, c, groups = shape
    for silu in (False, True):
        x, gamma, beta, ref, e = _gn("offset", shape, dtype, silu)
        y = emulate_groupnorm(x, gamma, beta, M, hw, groups, 1e-5, silu, pivot=False).to(dtype)
        _fails(y, ref, e, "offset %s hw%d c%d silu=%d: no pivot" % (dtype, hw, c, silu))
        x, gamma, beta, ref, e = _gn("randn", shape, dtype, silu)
        y = emulate_groupnorm(x, gamma, beta, M, hw, groups, 1e-5, silu, pivot=False).to(dtype)
        N.check(y, ref, e, "randn, no pivot: not visible")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bound_catches_missing_eps_and_unasked_silu(dtype):
    shape = (91, 320, 32)
    hw, c, groups = shape
    x, gamma, beta, ref, e = _gn("const", shape, dtype, False)
    y = emulate_groupnorm(x, gamma, beta, M, hw, groups, 1e-5, False, use_eps=False).to(dtype)
    _fails(y, ref, e, "const %s: eps left out (GroupNorm)" % dtype)
    for kind in ("randn", "offset", "spike", "const"):
        x, gamma, beta, ref, e = _gn(kind, shape, dtype, False)
        y = emulate_groupnorm(x, gamma, beta, M, hw, groups, 1e-5, True).to(dtype)
        _fails(y, ref, e, "%s %s: SiLU applied when not asked for" % (kind, dtype))
    xl = N.layernorm_data("const", 9, 320, dtype, 5, "cpu")
    gamma, beta = N.affine(320, dtype, 6, "cpu")
    ref, e = N.layernorm_reference(xl, gamma, beta, 1e-5)
    _fails(emulate_layernorm(xl, gamma, beta, 1e-5, use_eps=False).to(dtype), ref, e,
           "const %s: eps left out (LayerNorm)" % dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["randn", "offset", "spike"])
@pytest.mark.parametrize("shape", [(33, 320), (9, 1280), (7, 520)], ids=lambda s: "%dx%d" % s)
def test_bound_catches_layernorm_vector_left_out(dtype, kind, shape):
    rows, c = shape
    x = N.layernorm_data(kind, rows, c, dtype, 5, "cpu")
    gamma, beta = N.affine(c, dtype, 6, "cpu")
    ref, e = N.layernorm_reference(x, gamma, beta, 1e-5)
    N.check(emulate_layernorm(x, gamma, beta, 1e-5).to(dtype), ref, e, "correct")
    _fails(emulate_layernorm(x, gamma, beta, 1e-5, skip_last_vector=True).to(dtype), ref, e,
           "%s %s %dx%d: last 8-channel vector left out" % (kind, dtype, rows, c))
