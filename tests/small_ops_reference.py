"""fp64 references and per-element bounds for the small HIP kernels of csrc/elementwise.hip, csrc/vae.hip and the layout
kernel of csrc/tokens.hip, shared by test_small_ops_reference_cpu.py and test_small_ops_fp64_gpu.py.  `ulp`, `conv_acc`,
`epilogue`, `bound`, `check`, TAU and EPI_REL are gemm_reference's, ARG_REL and EXP_REL attention_reference's; u = 2^-24
(U), T is the storage type.  Every reference is computed in float64 from the SAME values the kernel reads (storage-type
operands, fp32 coefficients cast up) on the device that holds them.

The two criteria
----------------
* `closest` — "as close as the correct rounding", for kernels that round an almost exact fp32 value v once to T.  With
  r = ref.to(T) (torch's round-to-nearest-even) an element passes when y == r or |y - ref| <= |r - ref| + E.  y = RN_T(v)
  differs from r only where a rounding boundary of T lies between v and ref, and then |y - ref| - |r - ref| is twice the
  distance from ref to that boundary, which is at most 2 |v - ref|.  A conversion that truncates misses it on about
  half of the elements (|y - ref| up to a whole unit of T against half a unit).  Where r is infinite y must be r, unless
  |ref| is within E of the overflow threshold max_T + ulp_T(max_T) / 2: there the largest finite value is as good.
  NaN in y never passes (a missed write of a NaN-filled output).
* gemm_reference.check — |y - ref| <= ulp_T(ref) + E, for the kernels whose fp32 value carries an accumulation error
  (the two convolutions).  `conv_check` adds `closest` with 2 E (the worst case above), so that a truncating store is
  caught there too.

E per kernel (the fp32 value before the store against the fp64 reference)
--------------------------------------------------------------------------
dd_add, two operands: one fp32 add, u |ref|.  Three operands, (a + b) + c: u |a + b| + u |ref| <= 2u (|a| + |b| + |c|).
dd_scale: the reference multiplies by float32(s), what the launcher is handed; one fp32 product, u |ref|.
dd_silu, x * rcp(1 + exp2(-log2e x)) (dd_silu_f): the product -log2e x rounds relative 1.5u (the constant and the
  product), which is |x| 1.5u relative on e^-x; v_exp_f32 and v_rcp_f32 are good to one unit, then an add and a product:
  EPI_REL = 16u covers those as in gemm_reference, so EPI_REL (1 + |x|) |ref|.  Neither instruction returns a subnormal:
  an intermediate below 2^-126 becomes zero, |x| 2^-126 on the result.
dd_cfg_ddim_step, sa_p (x - s1a_t e) / sa_t + s1a_p e: at most six fp32 roundings (product, difference, quotient, two
  products, sum), each relative to a partial result no larger than the sum of the absolute terms:
  6u (sa_p (|x| + s1a_t |e|) / sa_t + s1a_p |e|).
dd_cfg_unipc_step (dd_unipc_coef::step): x0 = a_x x + a_e e;  xc = c_l last + c_1 m1 + c_2 m2 + c_0 x0 (or x itself,
  exactly, on the first step);  r = p_x xc + p_0 x0 + p_1 m1.  No product of the chain is deeper than 8 roundings under
  the fma contraction the compiler applies, so 8u times the sum of the absolute LEAF terms of each expression (x0 and
  xc expanded, as the DDIM row expands x0: their own rounding errors reach r through p_x and p_0, and |xc| may be far
  smaller than its terms): A_0 = |a_x x| + |a_e e|, A_c = |c_l last| + |c_1 m1| + |c_2 m2| + |c_0| A_0,
  A_r = |p_x| A_c + |p_0| A_0 + |p_1 m1|.  The history outputs are fp32: last = xc (E = 8u A_c, or exact), m1 = x0
  (8u A_0), m2 = the old m1 (exact).
Guided noise of both steps, (T)(eu + g (ec - eu)): with d = fl32(ec - eu) the fp32 value is v1 = fl32(eu + fl32(g d)) or
  v2 = fl32(fma(g, d, eu)), and the kernel stores T(v1) or T(v2).  Where these differ the element is ambiguous, and
  MAX_AMBIGUOUS bounds the share of such elements.  There is a third legal evaluation: the compiler may fold the
  conversion to T into the fma (gfx950's v_fma_mixlo_f16 does: the fp16 kernels are compiled to it), and that
  instruction rounds the unrounded fma ONCE, to T.  It differs from T(v2) where v2 is a rounding boundary of T that the
  exact value is not, which is rare on random data but not with g = 3.3 on fp16 operands: 3.3 d sits at such boundaries
  for whole classes of d, and float32(3.3) is just off them.  `guided` returns v1 and v2 for both types and this
  third form for fp16 only (there is no such bf16 instruction, and the bf16 kernels were seen to store T(v2)).  Which
  form a kernel takes is decided when it is compiled, not per element: `closest_either` wants EVERY element and every
  output of a launch to meet the bound under ONE of the candidates, so no element is free to take another's value.
dd_vae_posterior: p_o = bq_o + sum_c wq_oc x_c as a chain of 8 fmas over 9 terms, 9u (|bq_o| + sum_c |wq_oc x_c|) =: e_o.
  The clamp is 1-Lipschitz; sd = expf(lv / 2) is off by expm1(e_lv / 2) + EXP_REL relative (the halving is exact);
  v = fma(sd, noise, mean) and scale * v round once each (u each, relative to |mean| + sd |noise|):
  E = |scale| (e_mean + sd |noise| (expm1(e_lv / 2) + EXP_REL) + 2u (|mean| + sd |noise|)).  mode(): |scale| e_mean + u |ref|.
dd_softmax_rows (`__expf`, i.e. v_exp_f32 of the argument in log2 units): p_j = exp(s_j - max) / sum.  As attention_reference._one builds it for P: the argument s_j - max and
  its scaling to log2 units round ARG_REL |s_j - max| relative on the exponential, v_exp_f32 EXP_REL:
  d_j = ARG_REL |s_j - max| + EXP_REL; the denominator carries sum_k p_k d_k of it and cols u of its own fp32 sum; the
  reciprocal and the product 2u (one unit of v_rcp_f32).  v_exp_f32 returns no subnormal: 2^-126 absolute (sum >= 1).
  E_j = p_j (d_j + sum_k p_k d_k + (cols + 2) u) + 2^-126, then `closest`.
dd_timestep_embedding: arg = t exp(c j / (half - shift)) with c = float32(-ln 10000) as the kernel holds it.  The
  exponent is at most 9.21 in magnitude and takes three fp32 roundings (27.7u absolute, so relative on the frequency),
  expf one unit (2u), the product with t u: |arg| 2^-19.  sin and cos are 1-Lipschitz; sinf / cosf add 2^-22.
dd_fourier_embed: a = x f is exact for a power-of-two f, else u |a|; sinf / cosf 2^-22; the copied input is exact.
  Both embeddings then round once to T (not at all for fp32): `closest` with that error as E.
Layout converts: exact copies, torch.equal against permute / reshape and zero padding.

No constant above is fitted to a measurement.
"""
import math

import torch

from tests.attention_reference import ARG_REL, EXP_REL
from tests.gemm_reference import EPI_REL, TAU, bound, check, conv_acc, epilogue, rand, ulp  # noqa: F401  (re-exported)

U = 2.0 ** -24
FLUSH = 2.0 ** -126                      # below it v_exp_f32 / v_rcp_f32 return zero
MAX_AMBIGUOUS = 0.005                    # share of guided-noise elements whose two fp32 evaluations round apart
F64 = torch.float64


def _d(t):
    return t.to(F64)


# ---- "as close as the correct rounding" -----------------------------------------------------------------------------

def closest_ok(y, ref, e, dtype=None):
    """-> (ok, ratio): per element, whether y passes against (ref, e) in `dtype` (default y's), and the part of e it
    uses: (|y - ref| - |r - ref|) / e, 0 where y == r or y is closer than r, inf where y is wrong and e is 0.  (|y - ref|
    over |r - ref| + e would sit at 0.99 for every harmless flip next to a tie and say nothing.)"""
    dtype = dtype or y.dtype
    fi = torch.finfo(dtype)
    r = ref.to(dtype).to(F64)
    yd = y.to(F64)
    e = torch.as_tensor(e, dtype=F64, device=ref.device).expand_as(ref)
    same = yd == r
    fin = torch.isfinite(r) & torch.isfinite(yd)
    err = (yd - ref).abs()
    allow = (r - ref).abs() + e
    ok = same | (fin & (err <= allow))
    thr = fi.max + 0.5 * float(ulp(torch.tensor(fi.max, dtype=F64), dtype))
    edge = (ref.abs() - thr).abs() <= e
    top = torch.copysign(torch.full_like(ref, fi.max), ref)
    ok = ok | (edge & ((yd == top) | (yd == torch.copysign(torch.full_like(ref, float("inf")), ref))))
    over = (err - (r - ref).abs()).clamp(min=0)
    ratio = torch.where(fin & (e > 0), over / torch.where(e > 0, e, torch.ones_like(e)), torch.full_like(ref, float("inf")))
    ratio = torch.where(same | (ok & ~fin) | (fin & (over == 0)), torch.zeros_like(ratio), ratio)
    return ok, ratio


def _raise(what, ok, ratio, y, ref):
    bad = ~ok
    i = tuple(bad.nonzero()[0].tolist())
    raise AssertionError("%s: %d of %d elements are not as close as the correct rounding; first at %s: y=%r ref=%r "
                         "(max err/bound %.3g)" % (what, int(bad.sum()), bad.numel(), i, float(y[i]), float(ref[i]),
                                                   float(ratio.max())))


def closest(y, ref, e, what, dtype=None):
    """Assert the criterion everywhere; returns the largest part of e used, for the report."""
    assert y.shape == ref.shape, (what, tuple(y.shape), tuple(ref.shape))
    ok, ratio = closest_ok(y, ref, e, dtype)
    if not bool(ok.all()):
        _raise(what, ok, ratio, y, ref)
    return float(ratio.max()) if ratio.numel() else 0.0


def closest_either(ys, cands, what, dtypes=None):
    """ys: the outputs of ONE launch; cands: candidate lists [(ref, e) per output], one per evaluation of the guided noise
    (equal wherever the evaluations agree).  Passes when every element of every output passes against the SAME candidate:
    a kernel is compiled to one evaluation.  The failure reported is that of the candidate with the fewest bad elements."""
    dtypes = dtypes or [None] * len(ys)
    best = None
    for k, cand in enumerate(cands):
        pair = [closest_ok(y, ref, e, dt) for y, (ref, e), dt in zip(ys, cand, dtypes)]
        ok = torch.stack([p[0] for p in pair]).all(dim=0)
        ratio = torch.stack([p[1] for p in pair]).amax(dim=0)
        if bool(ok.all()):
            return float(ratio.max()) if ratio.numel() else 0.0
        if best is None or int((~ok).sum()) < int((~best[0]).sum()):
            best = (ok, ratio, k)
    _raise("%s (closest candidate: %d of %d)" % (what, best[2] + 1, len(cands)), best[0], best[1], ys[0], cands[best[2]][0][0])


def conv_check(y, ref, e, what):
    """gemm_reference.check, and `closest` with its worst case 2 e: a truncating store fails the second."""
    r1 = check(y, ref, e, what)
    closest(y, ref, 2 * e, what)
    return r1


# ---- add, scale, silu ---------------------------------------------------------------------------------------------------

def add_ref(a, b, c=None):
    A, B = _d(a), _d(b)
    if c is None:
        ref = A + B
        return ref, U * ref.abs()
    C = _d(c)
    return A + B + C, 2 * U * (A.abs() + B.abs() + C.abs())


def scale_ref(x, s):
    ref = _d(x) * float(torch.tensor(float(s), dtype=torch.float32))
    return ref, U * ref.abs()


def silu_ref(x):
    X = _d(x)
    ref = X * torch.sigmoid(X)
    return ref, EPI_REL * (1 + X.abs()) * ref.abs() + X.abs() * FLUSH


# randn x 1, x 100, + 1000 (large sums, exact in fp32), and a cancelling triple: a = randn + 1000, b = randn, c = -(randn
# + 1000), where a + b rounds in fp32 (b's low bits lie below a's fp32 unit) and c then takes the 1000 away, so that the
# rounding error is no longer small next to the result: the case add3's 2u (|a| + |b| + |c|) is there for
ADD_KINDS = [(1.0, 0.0), (100.0, 0.0), (1.0, 1000.0), "cancel"]


def add_operands(kind, k, n, dtype, make):
    """a, b, c of data kind number k; make(shape, dtype, seed, scale) draws fp32 randn."""
    if kind == "cancel":
        r = [make((n,), torch.float32, 10 * k + i, 1.0) for i in range(3)]
        return (r[0] + 1000.0).to(dtype), r[1].to(dtype), (-(r[2] + 1000.0)).to(dtype)
    mul, off = kind
    return tuple((make((n,), torch.float32, 10 * k + i, mul) + off).to(dtype) for i in range(3))


def finite_patterns(dtype, device="cpu"):
    """Every finite value of the 16-bit type, in bit-pattern order."""
    bits = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)
    x = bits.view(dtype)
    return x[torch.isfinite(x.float())].contiguous().to(device)


# ---- sampler steps --------------------------------------------------------------------------------------------------------

def round_once(z, dtype):
    """Round-to-nearest-even of the float64 z to the 16-bit `dtype` in ONE rounding (torch's .to() goes through fp32)."""
    fi = torch.finfo(dtype)
    over = fi.max + float(ulp(torch.tensor(fi.max, dtype=F64), dtype))      # what the step past max would be
    value = lambda t: torch.where(torch.isinf(t.to(F64)), torch.copysign(torch.full_like(z, over), z), t.to(F64))
    h = z.to(dtype)
    bits = h.view(torch.int16).to(torch.int32) & 0xFFFF
    mag = bits & 0x7FFF
    sign = torch.where(mag == 0, (z < 0).to(torch.int32) * 0x8000, bits & 0x8000)
    hd = value(h)
    mag2 = torch.where(z.abs() > hd.abs(), mag + 1, (mag - 1).clamp(min=0))  # h's neighbour on z's side
    nb = sign | mag2
    nb = torch.where(nb >= 0x8000, nb - 0x10000, nb).to(torch.int16).view(dtype)
    dh, dn = (z - hd).abs(), (z - value(nb)).abs()
    take = torch.isfinite(z) & ~torch.isnan(hd) & ((dn < dh) | ((dn == dh) & ((mag2 & 1) == 0) & ((mag & 1) == 1)))
    return torch.where(take, nb, h)


def guided(eps, g):
    """eps (2, n...) in T, uncond first -> ([e1, e2] or, for fp16, [e1, e2, e3], amb, fused): the guided noise in T from
    v1 = fl32(eu + fl32(g d)), from v2 = fl32(fma(g, d, eu)) and from the fma rounded once to T, d = fl32(ec - eu);
    amb = e1 != e2 (the elements MAX_AMBIGUOUS counts) and fused = e3 != e2 (all False for bf16).  Evaluated on the CPU
    (torch's fp32 ops there are single IEEE operations; the product of two fp32 values is exact in fp64), returned on
    eps's device."""
    e = eps.detach().cpu()
    eu, ec = e[0].float(), e[1].float()
    g32 = torch.tensor(float(g), dtype=torch.float32)
    d = ec - eu
    v1 = eu + g32 * d
    z = g32.double() * d.double() + eu.double()
    es = [v1.to(eps.dtype), z.float().to(eps.dtype)]
    if eps.dtype == torch.float16:
        es.append(round_once(z, eps.dtype))
    return [t.to(eps.device) for t in es], (es[0] != es[1]).to(eps.device), (es[-1] != es[1]).to(eps.device)


def ddim_ref(x, e, coef):
    """x, e (the guided noise) in T, coef the fp32 [sa_t, s1a_t, sa_p, s1a_p] row -> (ref, E)."""
    sa_t, s1a_t, sa_p, s1a_p = coef.detach().double().cpu().tolist()
    X, N = _d(x), _d(e)
    ref = sa_p * ((X - s1a_t * N) / sa_t) + s1a_p * N
    return ref, 6 * U * (abs(sa_p) * (X.abs() + abs(s1a_t) * N.abs()) / abs(sa_t) + abs(s1a_p) * N.abs())


def unipc_ref(x, e, hist, coef):
    """x, e in T, hist fp32 (3, n...) = [last, m1, m2] BEFORE the step, coef the fp32 row of unipc_schedule ->
    [(ref, E)] for the outputs [x_out (T), last, m1, m2 (fp32)]."""
    a_x, a_e, use_c, c_l, c_1, c_2, c_0, p_x, p_0, p_1 = coef.detach().double().cpu().tolist()
    X, N = _d(x), _d(e)
    last, m1, m2 = _d(hist[0]).reshape(X.shape), _d(hist[1]).reshape(X.shape), _d(hist[2]).reshape(X.shape)
    x0 = a_x * X + a_e * N
    a0 = (a_x * X).abs() + (a_e * N).abs()
    if use_c != 0.0:
        xc = c_l * last + c_1 * m1 + c_2 * m2 + c_0 * x0
        ac = (c_l * last).abs() + (c_1 * m1).abs() + (c_2 * m2).abs() + abs(c_0) * a0
        ec = 8 * U * ac
    else:
        xc, ac, ec = X, X.abs(), torch.zeros_like(X)
    r = p_x * xc + p_0 * x0 + p_1 * m1
    ar = abs(p_x) * ac + abs(p_0) * a0 + (p_1 * m1).abs()
    return [(r, 8 * U * ar), (xc, ec), (x0, 8 * U * a0), (m1, torch.zeros_like(X))]


# ---- VAE posterior --------------------------------------------------------------------------------------------------------

def posterior_ref(moments, wq, bq, m, h, w, noise=None, scale=1.0):
    """moments (m*h*w, 8) in T, wq (8, 8) / bq (8,) fp32, noise (m, 4, h, w) in T or None -> (ref, E), (m, 4, h, w)."""
    X, W, B = _d(moments), _d(wq).reshape(8, 8), _d(bq).reshape(8)
    p = X @ W.t() + B
    ep = 9 * U * (X.abs() @ W.abs().t() + B.abs())
    nchw = lambda t: t.reshape(m, h, w, -1).permute(0, 3, 1, 2)
    mean, e_mean = nchw(p[:, :4]), nchw(ep[:, :4])
    s = float(torch.tensor(float(scale), dtype=torch.float32))
    if noise is None:
        ref = s * mean
        return ref, abs(s) * e_mean + U * ref.abs()
    lv, e_lv = nchw(p[:, 4:]).clamp(-30.0, 20.0), nchw(ep[:, 4:])
    sd = torch.exp(0.5 * lv)
    sn = sd * _d(noise).abs()
    ref = s * (mean + sd * _d(noise))
    return ref, abs(s) * (e_mean + sn * (torch.expm1(0.5 * e_lv) + EXP_REL) + 2 * U * (mean.abs() + sn))


# ---- convolutions ---------------------------------------------------------------------------------------------------------

def conv_ref(x, w, bias, m, hin, win, stride=1, silu=False):
    """3x3 / pad 1 conv of the NHWC rows x (m*hin*win, cin) with the packed weight w (cout, 9*cin) -> (ref, E), NHWC rows
    (m*hout*wout, cout), before the output rounding."""
    acc, e_acc = conv_acc(x, w, m, hin, win, stride=stride)
    return epilogue(acc, e_acc, bias=bias, silu=silu)


def to_nchw(t, m, h, w):
    return t.reshape(m, h, w, -1).permute(0, 3, 1, 2).contiguous()


# ---- softmax rows ---------------------------------------------------------------------------------------------------------

def softmax_ref(s):
    """fp32 logits (rows, cols), -inf allowed next to at least one finite entry per row -> (p, E)."""
    S = _d(s)
    cols = S.shape[1]
    x = S - S.amax(dim=1, keepdim=True)
    p = torch.exp(x)
    p = p / p.sum(dim=1, keepdim=True)
    d = ARG_REL * torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x)) + EXP_REL
    den = (p * d).sum(dim=1, keepdim=True)
    return p, p * (d + den + (cols + 2) * U) + FLUSH


# ---- embeddings -----------------------------------------------------------------------------------------------------------

LN_PERIOD32 = float(torch.tensor(-9.210340371976184, dtype=torch.float32))


def timestep_ref(t, dim, flip=True, shift=0.0):
    """t fp32 [n] -> (ref, e) (n, dim): [cos | sin] when flip else [sin | cos]; e is the error of the fp32 value."""
    half = dim // 2
    j = torch.arange(half, dtype=F64, device=t.device)
    s32 = float(torch.tensor(float(shift), dtype=torch.float32))
    arg = _d(t)[:, None] * torch.exp(LN_PERIOD32 * j / (half - s32))[None, :]
    e = arg.abs() * 2.0 ** -19 + 2.0 ** -22
    sv, cv = torch.sin(arg), torch.cos(arg)
    return (torch.cat([cv, sv], dim=1) if flip else torch.cat([sv, cv], dim=1)), torch.cat([e, e], dim=1)


def fourier_ref(x, freqs, include_input=True):
    """x (..., dims) -> (ref, e) (..., dims * (inc + 2 F)): [x | sin f0 x | cos f0 x | ...]."""
    X = _d(x)
    refs = [X] if include_input else []
    errs = [torch.zeros_like(X)] if include_input else []
    for f in freqs:
        f32 = float(torch.tensor(float(f), dtype=torch.float32))
        a = X * f32
        exact = f32 != 0 and math.frexp(f32)[0] == 0.5
        e = (0.0 if exact else U) * a.abs() + 2.0 ** -22
        refs += [torch.sin(a), torch.cos(a)]
        errs += [e, e]
    return torch.cat(refs, dim=-1), torch.cat(errs, dim=-1)


# ---- layout ---------------------------------------------------------------------------------------------------------------

def nhwc_ref(x, c_pad=None, views=1):
    """(m, c, h, views * w) -> (m * views * h * w, c_pad) rows with zero channel padding, the views as instances."""
    m, c, h, wt = x.shape
    w = wt // views
    c_pad = c if c_pad is None else c_pad
    rows = x.reshape(m, c, h, views, w).permute(0, 3, 2, 4, 1).reshape(-1, c)
    out = torch.zeros((rows.shape[0], c_pad), dtype=x.dtype, device=x.device)
    out[:, :c] = rows
    return out


def nchw_ref(x, m, c, h, w):
    """(m*h*w, ld >= c) rows -> (m, c, h, w)."""
    return x[:, :c].reshape(m, h, w, c).permute(0, 3, 1, 2).contiguous()


# ---- the inputs of the sampler-step cases (the CPU test holds the ambiguity condition on the same data) -------------------

STEP_N = (1, 257, 2048 * 256 + 37)
STEP_G = (0.0, 1.0, 2.0, 7.5, 3.3)


def step_eps(n, dtype, g, step=0, device="cpu"):
    """The model output (2, n) of sampler-step case (n, g), step `step` of a run."""
    return rand((2, n), dtype, 1000 + 16 * STEP_G.index(g) + step, device=device)


def step_x(n, dtype, device="cpu"):
    return rand((n,), dtype, 7, device=device)
