"""fp64 reference and per-element error bound for dd_gemm (dense GEMM and 3x3 conv), shared by the GEMM/conv tests.

Reference
---------
Computed in float64 from the SAME fp16 / bf16 operands the kernel reads (no re-rounding of anything): dense
`A @ W.T` with A = cat(a, a2) on K; conv as nine tap matmuls over a zero-padded NHWC tensor (after the nearest upsample
of oracle/leaf_ops.conv3x3_ref, F.interpolate's rule), with the stride taken by slicing — no F.conv2d, so no MIOpen in
the reference.  The epilogue then follows dd_gemm's documented order (include/dualdiff_hip.h):

    v = alpha * (acc + bias + rowvec[row // rows_per_inst]) + res;   v = silu(v);   v += out   (accumulate)

GEGLU is `h * gelu_erf(g)` with h / g the first / second N columns; head-major planes are `v * scale` on the first
`planes` heads; the LayerNorm fold is computed as what it stands for: LayerNorm(x) (no affine, biased variance) times
the gamma-scaled weight, plus the folded bias.

Bound
-----
Per element, |y - ref| <= B with

    B = ulp_out(ref) + E

* ulp_out(ref): one unit of the output type at |ref|.  Round-to-nearest of the exact fp32 result costs half a unit of
  ITS binade; when that value lies just above a power of two whose lower neighbour ref sits under, that is one unit at
  |ref|.  (fp32 output: one fp32 unit.)
* E, the error of the fp32 value before the final rounding:
  - accumulator: the products of fp16 / bf16 operands are exact in fp32; their fp32 sum over K is off by at most
    (summation depth) * u * sum_k |a_ik w_jk| (u = 2^-24), and sum_k |a_ik w_jk| <= ||a_i||_2 ||w_j||_2 (Cauchy-Schwarz).
    The depth of MFMA blocks + K steps + split-K slabs stays below 256 for every K here, so
        E_acc = TAU * ||a_i|| * ||w_j||,   TAU = 2^-16 = 256 u.
    The row and column norms cost O((rows + n) K) and do not shrink under cancellation, unlike sum |a w|.
  - epilogue arithmetic: at most ~6 fp32 roundings and SiLU's exp / reciprocal approximations, each relative to a
    magnitude no larger than those of its operands:  E_epi = EPI_REL * (|alpha| (|acc| + |bias| + |rowvec|) + |res|
    + |out_old|),  EPI_REL = 2^-20 = 16 u.
  - propagation:  E_v = |alpha| E_acc + E_epi;  SiLU is Lipschitz with constant max |silu'| = 1.0998 < SILU_LIP = 1.1.
  - GEGLU:  |h gelu(g) - h' gelu(g')| <= |gelu(g)| E_h + GELU_LIP |h| E_g  (max |gelu'| = 1.1289 < 1.13), plus the
    kernel's erf (Abramowitz-Stegun 7.1.26, |error| <= 1.5e-7, halved by x Phi(x)) and its few fp32 operations:
    GELU_APPROX |h| |g| with GELU_APPROX = 4e-7.
  - head-major: scaled planes scale E by |scale| (the multiply itself is one more fp32 rounding, inside EPI_REL).
  - LayerNorm fold, y = rstd (x W'^T - mean colsum) + b': the accumulator term becomes rstd E_acc; the fp32 products
    mean * colsum (colsum handed in as fp32) and the fp32 row statistics add
    rstd TAU |mean| sqrt(K) ||w'_j||  (|colsum_j| <= sqrt(K) ||w'_j||)  and  TAU |y - b'|  (relative error of rstd).
    With `ln_stats_in` the statistics are those the producing GEMM summed from its fp32 values BEFORE rounding them
    into A (not those of the stored A: for bf16 the two differ by up to ~4x the bound above), so the reference takes
    mean / rstd from the producer's fp64 reference v and normalises the stored A with them; the producer's own error
    E_v adds rstd sqrt(K) ||w'_j|| mean(E_v) (mean) and |y| mean(|v - mean| E_v) / var (rstd).

No constant above is fitted to a measurement: each follows from the arithmetic named next to it.
"""
import math

import torch
import torch.nn.functional as F

TAU = 2.0 ** -16
EPI_REL = 2.0 ** -20
SILU_LIP = 1.1
GELU_LIP = 1.13
GELU_APPROX = 4e-7

_MANT = {torch.float16: 10, torch.bfloat16: 7, torch.float32: 23}
_EMIN = {torch.float16: -14, torch.bfloat16: -126, torch.float32: -126}


def ulp(x, dtype):
    """One unit in the last place of `dtype` at |x| (x: float64 tensor); subnormal spacing below the normal range."""
    ax = x.abs()
    e = torch.floor(torch.log2(torch.where(ax > 0, ax, torch.ones_like(ax))))
    e = torch.where(ax > 0, e, torch.full_like(ax, _EMIN[dtype])).clamp(min=_EMIN[dtype])
    return torch.exp2(e - _MANT[dtype])


def _f64(t):
    return None if t is None else t.to(torch.float64)


# ---- accumulators: (acc, E_acc) ------------------------------------------------------------------------------------------

def dense_acc(a, w, a2=None, rows=None):
    """acc = cat(a, a2) @ w.T in fp64 and its bound TAU ||a_i|| ||w_j||.  rows: optional index tensor — only those rows
    (huge launches are compared on a sample)."""
    A = _f64(a if a2 is None else torch.cat([a, a2], dim=1))
    if rows is not None:
        A = A[rows]
    W = _f64(w)
    return A @ W.t(), TAU * torch.outer(A.norm(dim=1), W.norm(dim=1))


def _upsample_pad(x, m, hin, win, up_size):
    X = _f64(x).reshape(m, hin, win, -1)
    if up_size is not None and tuple(up_size) != (hin, win):
        X = F.interpolate(X.permute(0, 3, 1, 2), size=tuple(up_size), mode="nearest").permute(0, 2, 3, 1)
    return F.pad(X, (0, 0, 1, 1, 1, 1))          # zero border on W and H


def conv_acc(x, w, m, hin, win, stride=1, up_size=None):
    """3x3 / pad 1 conv of the NHWC batch x (m*hin*win, cin) with w packed [cout][ky][kx][cin]: nine fp64 tap matmuls.
    Returns (acc (m*hout*wout, cout), E_acc) with ||a_i|| the norm of output pixel i's 3x3xcin input patch."""
    cin, cout = x.shape[1], w.shape[0]
    hv, wv = (hin, win) if up_size is None else (int(up_size[0]), int(up_size[1]))
    hout, wout = (hv - 1) // stride + 1, (wv - 1) // stride + 1
    xp = _upsample_pad(x, m, hin, win, up_size)
    W = _f64(w).reshape(cout, 3, 3, cin)
    acc = torch.zeros((m * hout * wout, cout), dtype=torch.float64, device=x.device)
    n2 = torch.zeros((m * hout * wout,), dtype=torch.float64, device=x.device)
    for ky in range(3):
        for kx in range(3):
            tap = xp[:, ky:ky + stride * (hout - 1) + 1:stride, kx:kx + stride * (wout - 1) + 1:stride, :]
            tap = tap.reshape(-1, cin)
            acc += tap @ W[:, ky, kx, :].t()
            n2 += (tap * tap).sum(dim=1)
    return acc, TAU * torch.outer(n2.sqrt(), _f64(w).norm(dim=1))


def ln_fold_acc(x, wp, lnb, eps, rows=None, stats_of=None):
    """LayerNorm fold as LayerNorm-then-GEMM: ((x - mean) rstd) @ wp.T + lnb (wp = gamma-scaled weight, lnb = W beta + b).
    stats_of = (v, E_v): the statistics come from the producer's values v (fp64 reference of the fp32 result the
    producing GEMM summed before rounding x, bound E_v) — the ln_stats_in form; else from x itself.
    Returns (acc, E) with E the fold's accumulator-side bound (module docstring)."""
    X = _f64(x) if rows is None else _f64(x[rows])
    W = _f64(wp)
    S = X if stats_of is None else stats_of[0]
    mean = S.mean(dim=1)
    var = ((S - mean[:, None]) ** 2).mean(dim=1)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = ((X - mean[:, None]) * rstd[:, None]) @ W.t()
    wn = W.norm(dim=1)
    sk = math.sqrt(X.shape[1])
    e = TAU * rstd[:, None] * (torch.outer(X.norm(dim=1), wn) + sk * torch.outer(mean.abs(), wn))
    rel = torch.full_like(rstd, TAU)
    if stats_of is not None:
        # the producer's fp32 values are off by E_v: the mean by <= mean(E_v), the variance by <= 2 mean(|v - mean| E_v)
        ev = stats_of[1]
        e = e + rstd[:, None] * sk * torch.outer(ev.mean(dim=1), wn)
        rel = rel + ((S - mean[:, None]).abs() * ev).mean(dim=1) / (var + eps)
    e = e + rel[:, None] * y.abs()
    return y + _f64(lnb)[None, :], e


# ---- epilogue: (ref, E) ---------------------------------------------------------------------------------------------------

def epilogue(acc, e_acc, *, bias=None, rowvec=None, rows_per_inst=1, alpha=1.0, res=None, silu=False, old=None,
             rows=None):
    """dd_gemm's epilogue in its documented order on the fp64 accumulator; returns (ref, E) before the output rounding.
    rows: the row indices acc holds (sampled comparison), for rowvec / res / old lookups."""
    v = acc.clone()
    mag = acc.abs()
    if bias is not None:
        b = _f64(bias)[None, :]
        v += b
        mag = mag + b.abs()
    if rowvec is not None:
        idx = torch.arange(acc.shape[0], device=acc.device) if rows is None else rows
        rv = _f64(rowvec)[idx // rows_per_inst]
        v += rv
        mag = mag + rv.abs()
    v *= alpha
    mag = abs(alpha) * mag
    e = abs(alpha) * e_acc
    if res is not None:
        r = _f64(res if rows is None else res[rows])
        v += r
        mag = mag + r.abs()
    if silu:
        e = SILU_LIP * e
        v = v * torch.sigmoid(v)
    if old is not None:
        o = _f64(old if rows is None else old[rows])
        v += o
        mag = mag + o.abs()
    return v, e + EPI_REL * mag


def geglu(acc, e_acc, bias=None):
    """h * gelu_erf(g) of the (rows, 2n) accumulator (+ bias) -> (ref, E) before the output rounding."""
    n = acc.shape[1] // 2
    v = acc if bias is None else acc + _f64(bias)[None, :]
    e = e_acc + EPI_REL * v.abs()
    h, g = v[:, :n], v[:, n:]
    gg = F.gelu(g)
    ref = h * gg
    return ref, gg.abs() * e[:, :n] + GELU_LIP * h.abs() * e[:, n:] + GELU_APPROX * h.abs() * g.abs() + EPI_REL * ref.abs()


def head_major(ref, e, d, planes, scale):
    """(rows, n) -> the kernel's (n / d, rows, d) plane layout, the first `planes` planes times `scale`."""
    rows, n = ref.shape
    s = torch.ones(n // d, dtype=torch.float64, device=ref.device)
    s[:planes] = scale
    ref = ref.reshape(rows, n // d, d).permute(1, 0, 2) * s[:, None, None]
    e = e.reshape(rows, n // d, d).permute(1, 0, 2) * s.abs()[:, None, None]
    return ref.contiguous(), e.contiguous()


# ---- the comparison -------------------------------------------------------------------------------------------------------

def bound(ref, e, out_dtype):
    return ulp(ref, out_dtype) + e


def check(y, ref, e, what, out_dtype=None):
    """Assert |y - ref| <= ulp_out(ref) + e everywhere (NaN in y fails: a missed write of a NaN-filled output).
    Returns max(|y - ref| / bound) for the report."""
    out_dtype = out_dtype or y.dtype
    b = bound(ref, e, out_dtype)
    err = (y.to(torch.float64) - ref).abs()
    bad = ~(err <= b)
    if bool(bad.any()):
        idx = bad.nonzero()[0].tolist()
        i = tuple(idx)
        raise AssertionError("%s: %d of %d elements outside the bound; first at %s: y=%r ref=%r bound=%r (max err/bound %.3g)"
                             % (what, int(bad.sum()), bad.numel(), i, float(y[i]), float(ref[i]), float(b[i]),
                                float(torch.nan_to_num(err / b, nan=float("inf")).max())))
    return float((err / b).max()) if err.numel() else 0.0


def check_stats(stats, ref, e, what):
    """ln_stats output (rows, n / 32, 2): per 32-column group, sum and sum of squares of the fp32 values the epilogue
    rounded for the store (so no output-rounding term).  Bounds: sum_g E and sum_g (2 |ref| E + E^2), plus the sums'
    own fp32 reductions."""
    rows, n = ref.shape
    r = ref.reshape(rows, n // 32, 32)
    ee = e.reshape(rows, n // 32, 32)
    s = stats.to(torch.float64)
    # the fp32 sums over 32 columns (adds, squares, lane shuffles) are fp32 reductions like the statistics: TAU
    r1 = check(s[..., 0], r.sum(-1), ee.sum(-1) + TAU * r.abs().sum(-1), what + " ln_stats sum", torch.float32)
    r2 = check(s[..., 1], (r * r).sum(-1), (2 * r.abs() * ee + ee * ee).sum(-1) + TAU * (r * r).sum(-1),
               what + " ln_stats sumsq", torch.float32)
    return max(r1, r2)


def nan_like(shape, dtype, device):
    return torch.full(shape, float("nan"), dtype=dtype, device=device)


def strided(rows, cols, dtype, device, fill, pad=64):
    """A (rows, cols) view of a (rows, cols + pad) buffer whose pad columns hold `fill`: the pad of an input must not
    reach the result (K over-read), the pad of an output must come back untouched (column over-write)."""
    buf = torch.full((rows, cols + pad), fill, dtype=dtype, device=device)
    return buf, buf[:, :cols]


def pad_untouched(buf, cols, fill):
    p = buf[:, cols:]
    return bool((p == fill).all()) if fill == fill else bool(torch.isnan(p).all())


def rand(shape, dtype, seed, scale=1.0, device="cuda"):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(device)


def rand_dev(shape, dtype, seed, scale=1.0, device="cuda"):
    """Same distribution drawn on the device (the large operands of the byte-extent cases)."""
    g = torch.Generator(device=device).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=device, dtype=torch.float32) * scale).to(dtype)
