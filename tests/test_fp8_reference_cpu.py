"""CPU self-test of tests/fp8_reference.py: the e4m3 decode / round against torch's cast, the fp32 recipe against the
per-element acceptance, and mutation tests — an fp32 emulation of dd_rowquant_fp8 / dd_gemm8 with ONE defect each must be
rejected by the very functions test_fp8_fp64_gpu.py checks the kernels with (and the faultless emulation accepted).
ops.quantize_fp8[_padded] are plain torch and are checked here as well."""
import pytest
import torch
import torch.nn.functional as F

from tests import fp8_reference as R
from tests import gemm_reference as G
from tests import norm_reference as N

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
F64 = torch.float64


# ---- the format ---------------------------------------------------------------------------------------------------------

def test_decode_all_codes():
    b = torch.arange(256, dtype=torch.uint8)
    d, t = R.decode(b), b.view(torch.float8_e4m3fn).to(F64)
    assert torch.equal(torch.isnan(d), torch.isnan(t)) and int(torch.isnan(d).sum()) == 2
    assert torch.equal(d[~torch.isnan(d)], t[~torch.isnan(t)])
    assert float(d[0x7E]) == 448.0 and float(d[0x01]) == 2.0 ** -9 and float(d[0x08]) == 2.0 ** -6
    assert torch.equal(torch.signbit(d[128:255]), torch.ones(127, dtype=torch.bool))


def test_rne_against_torch_cast():
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(200000, generator=g, dtype=F64) * s for s in (600.0, 30.0, 1.0, 2.0 ** -5, 2.0 ** -8)])
    want = x.float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    x = x.float().to(F64)                                     # the values the cast saw
    assert torch.equal(R.rne(x), want)
    mags = R.decode(torch.arange(127, dtype=torch.uint8))
    mid = 0.5 * (mags[1:] + mags[:-1])                        # the 126 midpoints between finite neighbours, both signs
    mid = torch.cat([mid, -mid, torch.zeros(1, dtype=F64)])
    assert mid.numel() == 253
    got = R.rne(mid)
    assert torch.equal(got, mid.float().to(torch.float8_e4m3fn).view(torch.uint8))
    assert bool(((got & 1) == 0).all()), "a tie must go to the even code"
    assert torch.equal(R.rne(torch.tensor([1e9, -1e9, 464.0, float("nan")], dtype=F64)),
                       torch.tensor([0x7E, 0xFE, 0x7E, 0x7F], dtype=torch.uint8))
    assert torch.equal(R.spacing(torch.tensor([0.0, 2.0 ** -7, 2.0 ** -6, 1.0, 1.99, 256.0, 448.0], dtype=F64)),
                       torch.tensor([2.0 ** -9, 2.0 ** -9, 2.0 ** -9, 0.125, 0.125, 32.0, 32.0], dtype=F64))


# ---- the row quantiser ---------------------------------------------------------------------------------------------------

def _ln_T(x, gamma, beta, eps):
    """fp32 LayerNorm rounded to the storage type: the y the kernel quantises."""
    return F.layer_norm(x.float(), (x.shape[1],), gamma.float(), beta.float(), eps).to(x.dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", R.ROWQUANT_KINDS)
def test_fp32_recipe_inside_candidates(dtype, kind):
    for rows, c in ((9, 520), (5, 8), (4, 1536)):
        y = R.rowquant_data(kind, rows, c, dtype, 3)
        q, s = R.fp32_recipe(y)
        assert R.check_rowquant(q, s, y, kind) == 0
        lo, hi, exact = R.candidates(y, *R.scale_spec(y))
        assert bool((hi.to(torch.int16) - lo.to(torch.int16)).abs().le(1).logical_or(R.canon(lo) == R.canon(hi)).all())
        assert bool((lo == hi)[exact].all())
        gamma, beta = N.affine(c, dtype, 5, "cpu")
        q, s = R.fp32_recipe(_ln_T(y, gamma, beta, 1e-5))
        ratio, pos = R.check_rowquant_ln(q, s, y, gamma, beta, 1e-5, kind)
        assert ratio <= 1.0 and pos <= 1.0


def test_pow2_rows_hit_exact_ties():
    y = R.rowquant_data("pow2", 64, 128, torch.bfloat16, 1)
    sc, amax = R.scale_spec(y)
    lo, hi, exact = R.candidates(y, sc, amax)
    assert bool(exact.all())
    t = y.to(F64) / sc.to(F64)[:, None]
    ties = (R.decode(R.rne(t)) - t).abs() == 0.5 * R.spacing(t)
    assert 1 / 32 < float(ties.double().mean()) < 1 / 4


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_tiny_and_nonfinite_rows(dtype):
    """What the 2^-126 floor and the NaN scale are for: the recipe without the floor turns the zeros of a tiny bf16 row
    into NaN codes (the kernel's fminf / fmaxf made -448 of them), and the checks reject both."""
    y = R.rowquant_data("edge", 5, 16, dtype, 1)
    q, s = R.fp32_recipe(y)
    assert R.check_rowquant(q, s, y, "edge") == 0
    back = R.decode(q) * s.to(F64)[:, None]
    assert bool(((back - y.to(F64)).abs() <= 0.5 * R.spacing(y.to(F64) / s.to(F64)[:, None]) * s.to(F64)[:, None] * (1 + R.DELTA)).all())
    if dtype == torch.bfloat16:
        q0, s0 = R.fp32_recipe(y, floor=False)
        assert int(q0[1, 1]) == R.NAN_CODE
        q0[1, 1] = 0xFE                                       # -448: what the clamp makes of the NaN
        with pytest.raises(AssertionError):
            R.check_rowquant(q0, s0, y, "edge, no floor")
    for bad in (float("nan"), float("inf"), float("-inf")):
        z = y.clone()
        z[3, 7] = bad
        q, s = R.fp32_recipe(z)
        assert bool(torch.isnan(s[3])) and int(torch.isnan(s).sum()) == 1
        R.check_rowquant(q, s, z, "non-finite")
        s2 = s.clone()
        s2[3] = 1.0                                           # the old kernel on a NaN row behind the LayerNorm
        with pytest.raises(AssertionError):
            R.check_rowquant(q, s2, z, "non-finite, finite scale")
        gamma, beta = N.affine(16, dtype, 5, "cpu")
        with pytest.raises(AssertionError):
            R.check_rowquant_ln(q, s2, z, gamma, beta, 1e-5, "non-finite, finite scale")


def _rne_half_away(t):
    a = t.abs().clamp(max=448.0)
    sp = R.spacing(a)
    v = torch.floor(a / sp + 0.5) * sp
    code = torch.searchsorted(R.decode(torch.arange(127, dtype=torch.uint8)), v.contiguous())
    return (code + torch.where(torch.signbit(t), 128, 0)).to(torch.uint8)


def _recipe_with(y, round_fn=R.rne, scale_shift=0):
    y = y.float()
    sc = (y.abs().amax(dim=1) / 448.0).clamp(min=R.SCALE_FLOOR).roll(scale_shift)
    q = round_fn((y * (1.0 / sc)[:, None]).clamp(-448, 448).to(F64))
    return q, sc


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rowquant_mutations_are_rejected(dtype):
    rows, c = 9, 520
    gamma, beta = N.affine(c, dtype, 5, "cpu")
    x = R.rowquant_data("spike", rows, c, dtype, 3)
    y = _ln_T(x, gamma, beta, 1e-5)
    # control: the faultless emulation passes both checks
    q, s = _recipe_with(x)
    R.check_rowquant(q, s, x, "control")
    ql, sl = _recipe_with(y)
    R.check_rowquant_ln(ql, sl, x, gamma, beta, 1e-5, "control ln")
    # a byte one code off (an element whose two candidates agree, away from the ends of the code range)
    lo, hi, _ = R.candidates(x, *R.scale_spec(x))
    r, j = ((lo == hi) & ((q & 0x7F) > 8) & ((q & 0x7F) < 0x70)).nonzero()[0].tolist()
    for step in (1, -1):
        m = q.clone()
        m[r, j] = int(m[r, j]) + step
        with pytest.raises(AssertionError, match="neither candidate"):
            R.check_rowquant(m, s, x, "one code off")
    # the same behind the LayerNorm, where the check is the dequantised value: a code of the top two binades moved one
    # step further from the reference is off by at least a whole spacing, the bound allows half of one (+ ulp_T + e)
    xr = R.rowquant_data("randn", rows, c, dtype, 6)
    qr, sr = _recipe_with(_ln_T(xr, gamma, beta, 1e-5))
    y64, _ = N.layernorm_reference(xr, gamma, beta, 1e-5)
    j = int((((qr[0] & 0x7F) >= 0x70) & ((qr[0] & 0x7F) <= 0x7C)).nonzero()[0])
    d = float(R.decode(qr[0, j]) * sr[0] - y64[0, j])
    m = qr.clone()
    m[0, j] = int(m[0, j]) + (1 if (d > 0) == (float(y64[0, j]) > 0) else -1)
    R.check_rowquant_ln(qr, sr, xr, gamma, beta, 1e-5, "control ln randn")
    with pytest.raises(AssertionError, match="dequantised"):
        R.check_rowquant_ln(m, sr, xr, gamma, beta, 1e-5, "one code off behind the LayerNorm")
    # round-half-away on rows whose scale is a power of two
    p2 = R.rowquant_data("pow2", rows, c, dtype, 4)
    qa, sa = _recipe_with(p2, _rne_half_away)
    assert int((qa != R.fp32_recipe(p2)[0]).sum()) > rows * c // 64
    R.check_rowquant(*_recipe_with(p2), p2, "control pow2")
    with pytest.raises(AssertionError, match="neither candidate"):
        R.check_rowquant(qa, sa, p2, "half away")
    # the scale (and so the bytes) of the neighbouring row
    qn, sn = _recipe_with(x, scale_shift=1)
    with pytest.raises(AssertionError, match="scale"):
        R.check_rowquant(qn, sn, x, "neighbour's scale")
    qn, sn = _recipe_with(y, scale_shift=1)
    with pytest.raises(AssertionError, match="scale"):
        R.check_rowquant_ln(qn, sn, x, gamma, beta, 1e-5, "neighbour's scale ln")
    # padding not written
    m = torch.cat([q, torch.zeros((rows, 120), dtype=torch.uint8)], dim=1)
    R.check_rowquant(m, s, x, "control padded")
    m[rows - 1, -1] = 1
    with pytest.raises(AssertionError, match="padding"):
        R.check_rowquant(m, s, x, "padding")


# ---- the GEMM ------------------------------------------------------------------------------------------------------------

def emulate_gemm8(a8, sa, w8, sw, dtype, bias=None, res=None, head_major=None, geglu=False, defect=None):
    """dd_gemm8 in torch fp32 (exact products, fp32 sums, the kernel's epilogue order), with one optional defect."""
    A, W = R.decode(a8).float(), R.decode(w8).float()
    if defect == "chunk dropped":
        A[:, 16:32] = 0
    elif defect == "chunk of the neighbouring row":
        A[:-1, 16:32] = A[1:, 16:32].clone()
    v = (A @ W.t()) * sa[:, None] * sw[None, :]
    if bias is not None:
        v = v + bias.float()[None, :]
    if geglu:
        n = v.shape[1] // 2
        h, g = (v[:, n:], v[:, :n]) if defect == "h and g swapped" else (v[:, :n], v[:, n:])
        return (h * F.gelu(g)).to(dtype)
    if res is not None:
        v = v + res.float()
    if head_major is not None:
        d, planes, scale = head_major
        v = v.reshape(v.shape[0], -1, d).permute(1, 0, 2).clone()
        v[:planes + (1 if defect == "one plane too many scaled" else 0)] *= scale
    return v.to(dtype)


ROWS, NN, KP = 37, 120, 256


def _operands(dtype, kind="randn", n=NN, sw_exp=0):
    a8, sa, w8, sw = R.operands(kind, ROWS, n, KP, 7, k=200, sw_exp=sw_exp)
    return a8, sa, w8, sw, G.rand((n,), dtype, 8, device="cpu"), G.rand((ROWS, n), dtype, 9, device="cpu")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gemm8_emulation_passes(dtype):
    for kind in R.KINDS:
        a8, sa, w8, sw, bias, res = _operands(dtype, kind)
        exact = kind in ("onehot", "exact-sum")
        chk = R.check_exact if exact else R.check_gemm8
        chk(emulate_gemm8(a8, sa, w8, sw, dtype), a8, sa, w8, sw, kind)
        chk(emulate_gemm8(a8, sa, w8, sw, dtype, head_major=(40, 1, 0.25 if exact else 0.158)), a8, sa, w8, sw, kind,
            head_major=(40, 1, 0.25 if exact else 0.158))
        r = R.check_gemm8(emulate_gemm8(a8, sa, w8, sw, dtype, bias, res), a8, sa, w8, sw, kind, bias=bias, res=res)
        assert r <= 1.0
        a8, sa, w8, sw, bias, res = _operands(dtype, kind, sw_exp=-7)
        r = R.check_gemm8(emulate_gemm8(a8, sa, w8, sw, dtype, bias, geglu=True), a8, sa, w8, sw, kind, bias=bias, geglu=True)
        assert r <= 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("defect", ["chunk dropped", "chunk of the neighbouring row"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_gemm8_chunk_mutations_are_rejected(dtype, defect, kind):
    a8, sa, w8, sw, bias, res = _operands(dtype, kind)
    with pytest.raises(AssertionError):
        (R.check_exact if kind in ("onehot", "exact-sum") else R.check_gemm8)(
            emulate_gemm8(a8, sa, w8, sw, dtype, defect=defect), a8, sa, w8, sw, defect)
    with pytest.raises(AssertionError):
        R.check_gemm8(emulate_gemm8(a8, sa, w8, sw, dtype, bias, res, defect=defect), a8, sa, w8, sw, defect, bias=bias, res=res)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gemm8_epilogue_mutations_are_rejected(dtype):
    a8, sa, w8, sw, bias, _ = _operands(dtype)
    for b in (bias, None):
        with pytest.raises(AssertionError):
            R.check_gemm8(emulate_gemm8(a8, sa, w8, sw, dtype, b, geglu=True, defect="h and g swapped"), a8, sa, w8, sw,
                          "swap", bias=b, geglu=True)
    for kind, scale in (("randn", 0.158), ("onehot", 0.25)):
        a8, sa, w8, sw, _, _ = _operands(dtype, kind)
        for planes in (0, 1, 2):
            hm = (40, planes, scale)
            y = emulate_gemm8(a8, sa, w8, sw, dtype, head_major=hm, defect="one plane too many scaled")
            with pytest.raises(AssertionError):
                (R.check_exact if kind == "onehot" else R.check_gemm8)(y, a8, sa, w8, sw, "planes + 1", head_major=hm)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_small_row_error_old_criterion_accepts_new_rejects(dtype):
    a8, sa, w8, sw, _, _ = _operands(dtype, "rowscale")
    ref, _ = R.gemm8_reference(a8, sa, w8, sw)
    y = emulate_gemm8(a8, sa, w8, sw, dtype)
    assert R.old_criterion(y, ref, dtype)
    R.check_gemm8(y, a8, sa, w8, sw, "control")
    r = int(sa.argmin())
    y[r, 5] = (float(ref[r, 5]) + 2.0 ** -10 * float(ref.abs().max()))
    assert abs(float(y[r, 5]) - float(ref[r, 5])) > 100 * float(ref[r].abs().max())     # far outside the row's own range
    assert R.old_criterion(y, ref, dtype), "the rel-to-max criterion was expected to accept this"
    with pytest.raises(AssertionError):
        R.check_gemm8(y, a8, sa, w8, sw, "error in a small-scale row")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_nonfinite_rows_of_the_gemm(dtype):
    a8, sa, w8, sw, bias, _ = _operands(dtype)
    sa = sa.clone()
    sa[3] = float("nan")
    y = emulate_gemm8(a8, sa, w8, sw, dtype, bias)
    assert R.check_gemm8(y, a8, sa, w8, sw, "nan row", bias=bias) <= 1.0
    y[3, 11] = 0.5                                            # a finite number made of saturated bytes
    with pytest.raises(AssertionError, match="non-finite"):
        R.check_gemm8(y, a8, sa, w8, sw, "nan row", bias=bias)


# ---- ops.quantize_fp8 / quantize_fp8_padded: plain torch ----------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("k", [8, 128, 136])
def test_quantize_fp8_torch(dtype, k):
    from dualdiff_amd import ops
    w = G.rand((24, k), dtype, k, k ** -0.5, device="cpu")
    w[5] = 0
    w[7] *= 2.0 ** -9
    w[9] *= 2.0 ** 6
    q, s = ops.quantize_fp8(w)
    assert q.shape == (24, k) and s.shape == (24,) and s.dtype == torch.float32
    r1 = R.check_quantize_torch(q.view(torch.uint8), s, w, "quantize_fp8 k=%d" % k)
    qp, sp = ops.quantize_fp8_padded(w)
    kp = (k + 127) // 128 * 128
    assert qp.shape == (24, kp) and qp.is_contiguous() and torch.equal(sp, s)
    assert torch.equal(qp.view(torch.uint8)[:, :k], q.view(torch.uint8))
    r2 = R.check_quantize_torch(qp.view(torch.uint8), sp, w, "quantize_fp8_padded k=%d" % k)
    assert max(r1, r2) <= 1.0
    assert bool((q.view(torch.uint8)[5] & 0x7F == 0).all()) and bool(torch.isfinite(s[5]))
