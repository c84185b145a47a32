"""fp64 reference, per-element acceptance and data for the W8A8 projection path of csrc/gemm8.hip (dd_rowquant_fp8,
dd_gemm8) and for ops.quantize_fp8[_padded], shared by test_fp8_reference_cpu.py and test_fp8_fp64_gpu.py.  `ulp`,
`epilogue`, `geglu`, `head_major`, `check`, TAU and EPI_REL are gemm_reference's, `layernorm_reference` is
norm_reference's.  No GPU import: everything runs on the device that holds its operands.

The number format
-----------------
OCP e4m3fn: sign, 4 exponent bits (bias 7), 3 mantissa bits; exponent field 0 holds the subnormals m / 8 * 2^-6; there
is no infinity, and S.1111.111 (0x7f, 0xff) is the only NaN, so the largest finite value is 1.75 * 2^8 = 448 (0x7e).
`decode` builds the 256 values from that rule.  The spacing of the codes at |t| is 2^-3 * 2^floor(log2 |t|), and 2^-9
below 2^-6 (`spacing`).  `rne` rounds a float64 to the nearest code, ties to the code with an even mantissa,
saturating at +-448: t / spacing is an exact power-of-two scaling in fp64, torch.round rounds halves to even, and the
result times the spacing is a code (or the next power of two, which is one too).  Neither function uses torch's
float8 cast; that cast is only the cross-check of the CPU test.

The row quantiser
-----------------
Spec, as the header of dd_rowquant_fp8 states it, in IEEE fp32 on y (the input, or the LayerNorm output rounded to the
storage type T):

    amax = max_c |y_c|;  sc = max(amax / 448, 2^-126)  (1 for an all-zero row);  inv = 1 / sc;
    t = clamp(y * inv, +-448);  q = rne(t);  scale = sc;  bytes c .. ldq - 1 are zero;
    a row that holds a NaN or an Inf: scale = NaN (its bytes are unspecified but finite).

`fp32_recipe` is that recipe in torch fp32 (`floor=False`: the recipe before the 2^-126 floor, for the tests that show
what the floor is for).  SCALE_FLOOR = 2^-126 is the smallest normal fp32: above it 1 / sc is finite (1 / 2^-126 =
2^126), below it sc is subnormal and 1 / sc overflows from amax < 448 * 2^-128 on.  The floor changes no row with amax
>= 448 * 2^-126 ~ 5.3e-36, and a floored row is quantised exactly (inv = 2^126, a power of two).

Acceptance without LayerNorm (`check_rowquant`): y is known exactly, so
  * scale must EQUAL fp32(max(amax / 448, 2^-126)): one correctly rounded division, nothing to reorder;
  * per element, with t64 = y / (amax / 448) in fp64 (the floored scale in place of amax / 448 where it applies), q
    must be one of rne(t64 (1 - d)), rne(t64 (1 + d)), d = DELTA = 3 * 2^-24: the division, the reciprocal and the
    product each round once, relative 2^-24 (`candidates`).  This holds for y * (1 / sc), y / sc and y * (448 / amax)
    alike.  rne is monotone and d is far below the relative code spacing 2^-4, so the two candidates are equal or
    neighbours.  Where all three operations are exact — amax / 448 is a power of two — d is 0, both candidates are
    rne(t64), and an exact tie must have gone to even: bf16 / fp16 data on such a row hits exact ties about 1/16 of the
    time (t64 has one bit more than a code whenever y has 5 significant bits).
  * +0 and -0 are one value (0x80 is compared as 0x00).
  * every row with a nonzero finite amax holds 0x7e or 0xfe (its largest element maps to +-448 exactly: amax * (1 / sc)
    rounds to within 448 (1 +- 2 * 2^-24), inside the round-to-448 interval (432, 464) and clamped) — except the
    floored rows, amax < 448 * 2^-126, whose largest element maps to amax * 2^126 < 448;
  * a zero row is all zero with scale 1, a non-finite row has scale NaN, the padding bytes are zero.
Separately `bytes_off` counts the bytes that differ from fp32_recipe (the count test_fp8_mfma_gpu.py caps).

Behind the LayerNorm (`check_rowquant_ln`): y64, e = norm_reference.layernorm_reference(...).  The kernel's y is the fp32
LayerNorm value rounded to T, within e + ulp_T(y64) of y64 (gemm_reference.bound).  So
  * amax lies in [max_c(|y64| - e - ulp_T), max_c(|y64| + e + ulp_T)] (the bound taken at the row's largest elements),
    and scale in that interval / 448 * (1 -+ 2^-23): the division's rounding and one unit of slack for the fp64
    evaluation of the interval itself; both ends floored at 2^-126;
  * |decode(q) scale - y64| <= e + ulp_T(y64) + half the e4m3 spacing at |t| times scale, t the kernel's own
    t = y / scale, whose magnitude is at most (|y64| + e + ulp_T) / scale: the spacing is taken there (it is monotone),
    capped at 448.  The three fp32 roundings (3 * 2^-24 |y|) sit inside ulp_T(y64), of which the rounding to T uses half;
  * the two exact invariants above (a +-448 byte per unfloored nonzero finite row, zero padding).

The GEMM
--------
acc64 = (decode(a8) @ decode(w8).T) * sa[:, None] * sw[None, :] (`gemm8_acc`), on the bytes and scales the kernel is
handed.  Products of two e4m3 values have at most 8 significant bits and exponents within 2^-18 .. 2^17.7: exact in
fp32.  The accumulator is an fp32 sum over K of exact products, 128 of them per MFMA and one MFMA per K step chained
through the accumulator operand: depth 128 + K / 128 < 256 for every K here, so, as gemm_reference derives,

    E_acc = TAU * (sa ||a8_i||) * (sw ||w8_j||),  TAU = 2^-16 = 256 u,

assuming the 128-wide block dot product of v_mfma_scale_f32_16x16x128_f8f6f4 is no less accurate than a sequential
fp32 sum of its products.  The two scale multiplications are two more fp32 roundings of the accumulator, inside
gemm_reference.epilogue's EPI_REL * |acc|.  Everything behind the accumulator is gemm_reference's: epilogue (bias,
residual), geglu, head_major, check (|y - ref| <= ulp_out(ref) + E; NaN in y fails).
A row whose a_scale is NaN (the quantiser's mark of a non-finite row) must come back non-finite in every column
(inside `check_gemm8`); the other rows are checked as usual.

Data kinds beyond randn (`operands`)
------------------------------------
rowscale: randn rows times 2^p, p spread evenly over -12 .. 8 across the rows of A and, independently, over the same 20
  octaves across the output channels of W (there shifted down by 2^6, so that the largest outputs, ~4 sigma * 2^8 * 2^2,
  stay inside fp16) — the per-element bound is what makes the small rows count; relative to max|ref| they vanish.
onehot:   a8[r] is one power of two at column (7 r + 3) mod K, W random finite codes, all scales powers of two.  Every
  output is ONE product, (4 significant bits) * 2^e with 2^-19 <= |out| <= 448 * 2^6: representable in fp16 (subnormals
  reach 2^-24) and bf16, every fp32 operation of the kernel exact: the result is compared for EQUALITY (`check_exact`).
  A row, 16-byte k chunk or channel routed wrongly through the swizzle, the tile remap or the GEGLU interleave reads
  another code.
exact-sum: entries of A and W in {-1, 0, 1}, at most 256 nonzeros per row of A, unit scales: every partial sum in any
  order is an integer of magnitude <= 256, exact in fp32, fp16 and bf16 (8 significant bits reach 256): EQUALITY.

No constant above is fitted to a measurement.
"""
import torch

from tests import gemm_reference as G
from tests import norm_reference as N

F64 = torch.float64
FP8_MAX = 448.0
DELTA = 3.0 * 2.0 ** -24
SCALE_FLOOR = 2.0 ** -126
SCALE_REL = 2.0 ** -23
NAN_CODE = 0x7F
TAU = G.TAU
_POW2 = torch.tensor([2.0 ** i for i in range(-16, 17)], dtype=F64)      # exact on every device: no exp2 of a device library


# ---- the format ---------------------------------------------------------------------------------------------------------

def decode(b):
    """uint8 tensor of OCP e4m3fn codes -> float64 values (NaN for 0x7f / 0xff)."""
    b = b.to(torch.int64)
    e, m = (b >> 3) & 15, (b & 7).to(F64)
    mag = torch.where(e == 0, m / 8.0 * 2.0 ** -6, (1.0 + m / 8.0) * _POW2.to(b.device)[e - 7 + 16])
    mag = torch.where((e == 15) & ((b & 7) == 7), torch.full_like(mag, float("nan")), mag)
    return torch.where((b >> 7) == 1, -mag, mag)


def spacing(t):
    """Distance between neighbouring e4m3 codes at |t| (float64): 2^-3 * 2^floor(log2 |t|), 2^-9 below 2^-6."""
    a = t.abs().clamp(max=FP8_MAX)
    _, ex = torch.frexp(a)                                   # a = mant * 2^ex, mant in [0.5, 1): floor(log2 a) = ex - 1
    ex = torch.where(a > 0, ex, torch.full_like(ex, -100))
    return _POW2.to(t.device)[((ex - 1).clamp(min=-6) - 3 + 16).to(torch.int64)]


def _magnitudes(device):
    return decode(torch.arange(127, dtype=torch.uint8, device=device))          # increasing: 0 .. 448


def rne(t):
    """float64 -> the nearest e4m3fn code (uint8), ties to even, saturating at +-448; NaN -> 0x7f."""
    t = t.to(F64)
    a = t.abs().clamp(max=FP8_MAX)
    a = torch.where(torch.isnan(t), torch.zeros_like(a), a)
    sp = spacing(a)
    v = torch.round(a / sp) * sp                              # exact: power-of-two scaling, round-half-even, and back
    code = torch.searchsorted(_magnitudes(t.device), v.contiguous())
    code = (code + torch.where(torch.signbit(t), 128, 0)).to(torch.uint8)
    return torch.where(torch.isnan(t), torch.full_like(code, NAN_CODE), code)


def canon(b):
    """-0 -> +0: the two zero codes are one value."""
    return torch.where(b == 0x80, torch.zeros_like(b), b)


# ---- the row quantiser --------------------------------------------------------------------------------------------------

def fp32_recipe(y, floor=True):
    """The spec in torch fp32.  y (rows, c): values of the storage type (any float dtype) -> (bytes uint8, scale fp32)."""
    y = y.to(torch.float32)
    bad = ~torch.isfinite(y).all(dim=1)
    amax = torch.where(torch.isfinite(y), y.abs(), torch.zeros_like(y)).amax(dim=1)
    sc = amax / 448.0
    if floor:
        sc = sc.clamp(min=SCALE_FLOOR)
    sc = torch.where(amax > 0, sc, torch.ones_like(sc))
    inv = 1.0 / sc
    t = (y * inv[:, None]).clamp(-FP8_MAX, FP8_MAX)
    q = rne(t.to(F64))                                         # NaN (0 * inf on an unfloored tiny row) -> 0x7f
    q = torch.where(bad[:, None], torch.zeros_like(q), q)
    return q, torch.where(bad, torch.full_like(sc, float("nan")), sc)


def scale_spec(y):
    """fp32(max(amax / 448, 2^-126)) per row (1 for a zero row, NaN for a non-finite one), and amax in fp64."""
    Y = y.to(F64)
    bad = ~torch.isfinite(Y).all(dim=1)
    amax = torch.where(torch.isfinite(Y), Y.abs(), torch.zeros_like(Y)).amax(dim=1)
    # the fp64 quotient rounded to fp32 IS the correctly rounded fp32 quotient: N / 7 with N < 2^11 stays 2^-39 (relative)
    # away from every fp32 rounding boundary, the fp64 quotient within 2^-53 of it
    sc = (amax / 448.0).to(torch.float32).clamp(min=SCALE_FLOOR)
    sc = torch.where(amax > 0, sc, torch.ones_like(sc))
    return torch.where(bad, torch.full_like(sc, float("nan")), sc), amax


def candidates(y, sc, amax):
    """The two acceptable codes per element (module docstring): rne(t64 (1 -+ d)), d = 0 on rows whose amax / 448 is a
    power of two (or floored): nothing is rounded there."""
    Y = y.to(F64)
    s64 = torch.maximum(amax / 448.0, torch.full_like(amax, SCALE_FLOOR))
    s64 = torch.where(amax > 0, s64, torch.ones_like(s64))
    mant, _ = torch.frexp(sc.to(F64))
    exact = (mant == 0.5) & (sc.to(F64) == s64)
    d = torch.where(exact, torch.zeros_like(s64), torch.full_like(s64, DELTA))[:, None]
    t = Y / s64[:, None]
    return rne((t * (1.0 - d)).clamp(-FP8_MAX, FP8_MAX)), rne((t * (1.0 + d)).clamp(-FP8_MAX, FP8_MAX)), exact


def _has_max_code(q):
    return ((q == 0x7E) | (q == 0xFE)).any(dim=1)


def check_rowquant(q, scale, y, what):
    """q (rows, ldq) uint8, scale (rows,) fp32 as the kernel wrote them for y (rows, c) WITHOUT LayerNorm.  Asserts the
    acceptance of the module docstring; returns the number of bytes that differ from fp32_recipe (finite rows)."""
    rows, c = y.shape
    q, scale = q.reshape(rows, -1), scale.reshape(rows)
    assert bool((q[:, c:] == 0).all()), "%s: padding bytes are not zero" % what
    sc, amax = scale_spec(y)
    fin = ~torch.isnan(sc)
    assert bool(torch.isnan(scale[~fin]).all()), "%s: a row with a NaN or Inf must get scale = NaN" % what
    assert torch.equal(scale[fin], sc[fin]), "%s: scale differs from fp32(max(amax / 448, 2^-126)): first row %d" % (
        what, int(((scale != sc) & fin).nonzero()[0]))
    lo, hi, _ = candidates(y, sc, amax)
    qc = canon(q[:, :c])
    ok = (qc == canon(lo)) | (qc == canon(hi)) | ~fin[:, None]
    if not bool(ok.all()):
        r, j = (~ok).nonzero()[0].tolist()
        raise AssertionError("%s: %d of %d bytes are neither candidate; first at (%d, %d): y=%r scale=%r got 0x%02x, "
                             "candidates 0x%02x 0x%02x" % (what, int((~ok).sum()), ok.numel(), r, j, float(y[r, j]),
                                                           float(scale[r]), int(q[r, j]), int(lo[r, j]), int(hi[r, j])))
    nz = fin & (amax >= 448.0 * SCALE_FLOOR)
    assert bool(_has_max_code(q[:, :c])[nz].all()), "%s: a nonzero finite row without a +-448 byte" % what
    return bytes_off(q[:, :c], y, fin)


def bytes_off(q, y, rows_mask=None):
    """Number of bytes that differ from fp32_recipe(y) (+-0 alike); the recipe runs on the CPU, in IEEE fp32 whatever the
    device's torch kernels do."""
    qr, _ = fp32_recipe(y.cpu())
    diff = canon(q[:, :y.shape[1]].cpu()) != canon(qr)
    if rows_mask is not None:
        diff = diff & rows_mask.cpu()[:, None]
    return int(diff.sum())


def check_rowquant_ln(q, scale, x, gamma, beta, eps, what):
    """The same behind a LayerNorm: x (rows, c), gamma / beta (c,) in the storage type T.  Returns (max err / bound of
    the dequantised values, max position of the scale inside its interval: <= 1 inside)."""
    rows, c = x.shape
    T = x.dtype
    q, scale = q.reshape(rows, -1), scale.reshape(rows).to(F64)
    assert bool((q[:, c:] == 0).all()), "%s: padding bytes are not zero" % what
    bad = ~torch.isfinite(x.to(F64)).all(dim=1)
    assert bool(torch.isnan(scale[bad]).all()), "%s: a row with a NaN or Inf must get scale = NaN" % what
    fin = ~bad
    xs = torch.where(fin[:, None], x, torch.zeros_like(x))               # the reference asserts on its own statistics
    y64, e = N.layernorm_reference(xs, gamma, beta, eps)
    slack = e + G.ulp(y64, T)
    hi = (y64.abs() + slack).amax(dim=1)
    lo = (y64.abs() - slack).amax(dim=1).clamp(min=0)
    s_hi = (hi / 448.0 * (1.0 + SCALE_REL)).clamp(min=SCALE_FLOOR)
    s_lo = (lo / 448.0 * (1.0 - SCALE_REL)).clamp(min=SCALE_FLOOR)
    mid, half = 0.5 * (s_hi + s_lo), 0.5 * (s_hi - s_lo)
    pos = torch.where(fin, (scale - mid).abs() / half.clamp(min=1e-300), torch.zeros_like(mid))
    inside = ((scale >= s_lo) & (scale <= s_hi)) | bad | ((lo == 0) & (scale == 1.0) & (q[:, :c] == 0).all(dim=1))
    if not bool(inside.all()):
        r = int((~inside).nonzero()[0])
        raise AssertionError("%s: scale of row %d is %r, outside [%r, %r]" % (what, r, float(scale[r]), float(s_lo[r]), float(s_hi[r])))
    s = torch.where(fin, scale, torch.ones_like(scale))[:, None]
    tmax = ((y64.abs() + slack) / s).clamp(max=FP8_MAX)
    b = slack + 0.5 * spacing(tmax) * s
    err = (decode(q[:, :c]) * s - y64).abs()
    okm = (err <= b) | bad[:, None]
    if not bool(okm.all()):
        r, j = (~okm).nonzero()[0].tolist()
        raise AssertionError("%s: %d of %d dequantised values outside the bound; first at (%d, %d): got %r ref %r bound %r"
                             % (what, int((~okm).sum()), okm.numel(), r, j, float(decode(q[r, j]) * s[r, 0]),
                                float(y64[r, j]), float(b[r, j])))
    nz = fin & (lo >= 448.0 * SCALE_FLOOR)
    assert bool(_has_max_code(q[:, :c])[nz].all()), "%s: a nonzero finite row without a +-448 byte" % what
    ratio = torch.where(bad[:, None], torch.zeros_like(err), err / b)
    return float(ratio.max()), float(pos.max())


def check_quantize_torch(q, scale, w, what):
    """ops.quantize_fp8[_padded] (plain torch): per element within half an e4m3 step times the scale (plus the fp32
    roundings of the scale and the quotient, DELTA |w|), every nonzero row reaches |q| = 448, padding bytes zero, a zero
    row gives zeros and a finite scale."""
    n, k = w.shape
    W = w.to(F64)
    s = scale.to(F64)[:, None]
    assert bool(torch.isfinite(scale).all()) and bool((scale > 0).all()), "%s: scale not finite and positive" % what
    assert bool((q[:, k:] == 0).all()), "%s: padding bytes are not zero" % what
    d = decode(q[:, :k])
    b = 0.5 * spacing(W.abs() / s + 0.5 * spacing(W / s)) * s + DELTA * W.abs()
    err = (d * s - W).abs()
    assert bool((err <= b).all()), "%s: max err/bound %.3g" % (what, float((err / b.clamp(min=1e-300)).max()))
    nz = W.abs().amax(dim=1) > 0
    assert bool(_has_max_code(q[:, :k])[nz].all()), "%s: a nonzero row without a +-448 byte" % what
    assert bool((canon(q[:, :k])[~nz] == 0).all()), "%s: a zero row must quantise to zeros" % what
    return float((err / b.clamp(min=1e-300)).max())


# ---- the GEMM -----------------------------------------------------------------------------------------------------------

def gemm8_acc(a8, sa, w8, sw):
    """a8 (rows, K) / w8 (n, K) uint8 codes, sa (rows,) / sw (n,) fp32 -> (acc64, E_acc).  Rows whose scale is not
    finite are computed with scale 0 (they are checked by check_nonfinite_rows, and must not poison the bound)."""
    A, W = decode(a8), decode(w8)
    sa64 = torch.where(torch.isfinite(sa), sa, torch.zeros_like(sa)).to(F64)
    sw64 = sw.to(F64)
    acc = (A @ W.t()) * sa64[:, None] * sw64[None, :]
    return acc, TAU * torch.outer(sa64.abs() * A.norm(dim=1), sw64.abs() * W.norm(dim=1))


def gemm8_reference(a8, sa, w8, sw, *, bias=None, res=None, head_major=None, geglu=False):
    """(ref, E) before the output rounding, in the layout the kernel stores: (rows, n), (rows, n / 2) with geglu (w8 has
    the h | g rows), or (n / D, rows, D) planes with head_major = (D, planes, scale)."""
    acc, e_acc = gemm8_acc(a8, sa, w8, sw)
    if geglu:
        return G.geglu(acc, e_acc, bias)
    ref, e = G.epilogue(acc, e_acc, bias=bias, res=res)
    if head_major is not None:
        ref, e = G.head_major(ref, e, *head_major)
    return ref, e


def keep_rows(t, mask, head_major):
    """The rows `mask` selects, of a (rows, n) result or of (planes, rows, D) head-major planes."""
    return t[:, mask] if head_major else t[mask]


def check_gemm8(y, a8, sa, w8, sw, what, **epi):
    """gemm_reference.check on the rows with a finite a_scale; the others must be non-finite in every column.  Returns
    max err / bound."""
    ref, e = gemm8_reference(a8, sa, w8, sw, **epi)
    assert tuple(y.shape) == tuple(ref.shape), (what, tuple(y.shape), tuple(ref.shape))
    fin = torch.isfinite(sa)
    hm = epi.get("head_major") is not None
    if not bool(fin.all()):
        assert not bool(torch.isfinite(keep_rows(y, ~fin, hm)).any()), \
            "%s: a row with a non-finite a_scale came back with finite values" % what
    return G.check(keep_rows(y, fin, hm), keep_rows(ref, fin, hm), keep_rows(e, fin, hm), what, y.dtype)


def check_exact(y, a8, sa, w8, sw, what, **epi):
    """EQUALITY with the fp64 reference (onehot / exact-sum data without bias, residual or GEGLU: the reference is
    representable in the output type and every operation of the kernel is exact).  +0 == -0."""
    ref, _ = gemm8_reference(a8, sa, w8, sw, **epi)
    assert tuple(y.shape) == tuple(ref.shape), (what, tuple(y.shape), tuple(ref.shape))
    assert torch.equal(ref.to(y.dtype).to(F64), ref), "%s: the reference is not representable in %s" % (what, y.dtype)
    ne = ~(y.to(F64) == ref)
    if bool(ne.any()):
        i = tuple(ne.nonzero()[0].tolist())
        raise AssertionError("%s: %d of %d elements differ from the exact result; first at %s: y=%r ref=%r"
                             % (what, int(ne.sum()), ne.numel(), i, float(y[i]), float(ref[i])))
    return 0.0


def old_criterion(y, ref, dtype):
    """What test_fp8_mfma_gpu.py asserts: max |y - ref| / max |ref| <= 1.5 * (2^-10 fp16, 2^-7 bf16)."""
    tol = (2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7) * 1.5
    return float((y.to(F64) - ref).abs().max() / (ref.abs().max() + 1e-12)) <= tol


# ---- data ---------------------------------------------------------------------------------------------------------------

KINDS = ("randn", "rowscale", "onehot", "exact-sum")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def quantize_rows(x):
    """fp32_recipe on the first dims -> (codes uint8 padded with zeros to K % 128 == 0, scale fp32): the A8 / W8 operands
    of the GEMM tests that do not go through the kernels' own quantisers."""
    q, s = fp32_recipe(x)
    kp = (x.shape[1] + 127) // 128 * 128
    out = torch.zeros((x.shape[0], kp), dtype=torch.uint8)
    out[:, :x.shape[1]] = q
    return out, s


def operands(kind, rows, n, kp, seed, k=None, sw_exp=0):
    """-> a8 (rows, kp) uint8, sa (rows,) fp32, w8 (n, kp) uint8, sw (n,) fp32 on the CPU; k <= kp columns carry data (the
    rest is the zero padding the ABI asks for).  Kinds: module docstring.  sw_exp: onehot and rowscale, added to the exponents
    of W's channel scales (GEGLU multiplies two outputs: sw_exp = -7 keeps |h gelu(g)| <= 224^2 inside fp16)."""
    g = _gen(seed)
    k = kp if k is None else k
    a8 = torch.zeros((rows, kp), dtype=torch.uint8)
    w8 = torch.zeros((n, kp), dtype=torch.uint8)
    if kind in ("randn", "rowscale"):
        a = torch.randn((rows, k), generator=g)
        w = torch.randn((n, k), generator=g) * k ** -0.5
        if kind == "rowscale":
            a = a * torch.exp2(torch.round(torch.linspace(-12, 8, rows)))[torch.randperm(rows, generator=g)][:, None]
            w = w * torch.exp2(torch.round(torch.linspace(-18, 2, n)) + sw_exp)[torch.randperm(n, generator=g)][:, None]
        (qa, sa), (qw, sw) = fp32_recipe(a), fp32_recipe(w)
        a8[:, :k], w8[:, :k] = qa, qw
        return a8, sa, w8, sw
    if kind == "onehot":
        r = torch.arange(rows)
        p = torch.randint(-2, 3, (rows,), generator=g)
        a8[r, (7 * r + 3) % k] = rne(torch.exp2(p.to(F64)))
        codes = torch.randint(0, 127, (n, k), generator=g) + 128 * torch.randint(0, 2, (n, k), generator=g)   # no NaN code
        w8[:, :k] = codes.to(torch.uint8)
        sa = torch.exp2(torch.randint(-2, 3, (rows,), generator=g).float())
        sw = torch.exp2(torch.randint(-2, 3, (n,), generator=g).float() + sw_exp)
        return a8, sa, w8, sw
    if kind == "exact-sum":
        lut = rne(torch.tensor([-1.0, 0.0, 1.0], dtype=F64))
        a = torch.randint(0, 3, (rows, k), generator=g)
        if k > 256:                                            # at most 256 nonzeros per row of A
            keep = torch.rand((rows, k), generator=g).argsort(dim=1) < 256
            a = torch.where(keep, a, torch.ones_like(a))
        a8[:, :k] = lut[a]
        w8[:, :k] = lut[torch.randint(0, 3, (n, k), generator=g)]
        return a8, torch.ones(rows), w8, torch.ones(n)
    raise ValueError(kind)


ROWQUANT_KINDS = N.KINDS + ("pow2", "edge")


def rowquant_data(kind, rows, c, dtype, seed, device="cpu"):
    """(rows, c) in the storage type.  norm_reference.layernorm_data's kinds; pow2: 5-significant-bit values on rows whose
    largest magnitude is 448 * 2^p (amax / 448 a power of two: every fp32 operation exact, ties must go to even); edge:
    randn with row 0 all zero, row 1 at the subnormal floor of the type (for bf16: below 448 * 2^-126, the floored
    scale; [1e-37, 0, -5e-38, ...]), row 2 tiny normals, where there are that many rows."""
    if kind in N.KINDS:
        return N.layernorm_data(kind, rows, c, dtype, seed, device)
    g = _gen(seed)
    if kind == "pow2":
        # y = m * 2^p with |m| <= 28 (5 bits, exact in fp16 and bf16) and one element 28 * 2^p = 448 * 2^(p - 4) per row:
        # scale = 2^(p - 4), t = 16 m: multiples of 16 up to 448, a tie wherever |m| is odd and above 16 (code spacing 32)
        m = torch.randint(-28, 29, (rows, c), generator=g).float()
        m[torch.arange(rows), torch.randint(0, c, (rows,), generator=g)] = 28.0
        p = torch.randint(-6, 7, (rows, 1), generator=g).float()
        return (m * torch.exp2(p)).to(dtype).to(device)
    if kind == "edge":
        x = torch.randn((rows, c), generator=g)
        tiny = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -133           # smallest subnormal of the type
        x[0] = 0
        if rows > 1:
            x[1] = torch.randint(-40, 41, (c,), generator=g).float() * tiny
            if dtype == torch.bfloat16:
                x[1, :3] = torch.tensor([1e-37, 0.0, -5e-38])
        if rows > 2:
            x[2] = torch.randn((c,), generator=g) * (2.0 ** -14 if dtype == torch.float16 else 2.0 ** -120)
        return x.to(dtype).to(device)
    raise ValueError(kind)


def report(family, dtype, ratios, extra=""):
    name = {torch.float16: "f16", torch.bfloat16: "bf16"}.get(dtype, dtype)
    print("[fp8 fp64] %-28s %-5s launches %4d   max err/bound %.3f%s" % (family, name, len(ratios), max(ratios), extra))
    assert max(ratios) <= 1.0
