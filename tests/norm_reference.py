"""fp64 reference and per-element error bound for dd_groupnorm_nhwc (dd_gn_stats_kernel + dd_gn_apply_kernel and
dd_gn_fused_kernel) and dd_layernorm (dd_layernorm_kernel, dd_layernorm_sub_kernel), shared by the norm tests.  `ulp`,
`check`, `nan_like`, `rand`, `EPI_REL`, `SILU_LIP` and `TAU` are gemm_reference's.

Reference
---------
Computed in float64 from the SAME fp16 / bf16 operands the kernel reads, on the device that holds them.  GroupNorm:
x = cat(x1, x2) on C before anything else, then per (instance, group) over hw pixels x (C / groups) channels

    mu = mean(x),  var = mean((x - mu)^2)  (biased),  r = 1 / sqrt(var + eps),  y = act((x - mu) r gamma + beta)

with act = SiLU or nothing.  LayerNorm: the same per row over its C channels, no activation.

Bound
-----
Per element, |y - ref| <= ulp_out(ref) + E (gemm_reference.check).  E follows the kernels' fp32 arithmetic; u = 2^-24.

Statistics.  GroupNorm sums d = x - p and d^2 in ONE pass around a pivot p = the group's element at pixel 0, first
channel (csrc/norm.hip: gn_pivot), so mean = p + sum(d) / n and var = sum(d^2) / n - (sum(d) / n)^2; d itself is exact in
fp32 for data within 2^13 of the pivot's binade.  LayerNorm is two-pass around p = 0: mean = sum(x) / c, then
var = sum((x - mean)^2) / c.  With A1 = mean|x - p|, dm = |mu - p|, M2 = var + dm^2 = mean((x - p)^2):

  * mean: an fp32 sum whose longest serial add chain is L is off by at most L u sum|d|, so  d_mu = T A1.
    GroupNorm: T = TAU = 2^-16 = 256 u, the project's constant for chains below 256.  The deepest chain among the
    workload's shapes is the 89600 x 128 image of the VAE decoder on the two-launch path: 88 pixels per lane, 4 channels of
    the vector, 16 pixel lanes per group, 8 splits per chunk and 8 chunks: 124 adds.  The fused form stays below 90
    (8 vectors x 8 channels per thread, 16 strided shares per lane, 6 shuffle steps).  ONE case of the GPU test goes
    past 256: groups = 1 at c = 4096 lets the owner thread of dd_gn_stats_kernel add the 256 vector shares of each of the
    two channel passes in sequence, 512 + 4 + 8 + 3 = 527 adds, for which the worst case would be 2.06 TAU.  T stays TAU
    there as well: roundings of either sign do not line up over 527 adds, a smaller T only makes the check stricter, and
    no model of this project has fewer than 32 groups.
    LayerNorm: T = 2^-18 = 64 u: at most 4 vectors x 8 channels = 32 serial adds per lane and 6 shuffle steps.
  * variance: the sum of squares is off by T M2 (every d^2 is rounded once: inside T), and dm^2 inherits the mean's
    error:  e_var = T M2 + 2 dm d_mu + d_mu^2.  LayerNorm squares CENTRED values, (x - mean')^2 with mean' off by d_mu:
    e_var = T var + d_mu^2 (the cross term sums to zero to first order; the centring error enters squared).
  * rstd: r'/r = sqrt((var + eps) / (var' + eps)), so with rel = e_var / (2 (var + eps)) the relative error of rstd is
    d_r = rel (1 + 4 rel) + 2^-22; the second-order factor holds for rel < 2^-6, which the reference ASSERTS; 2^-22 covers
    rsqrtf (one fp32 unit) and the division by n.

Apply.  GroupNorm folds the statistics into sc = r gamma, sh = beta - mean sc and stores x sc + sh:

    E = |gamma| r (d_mu + |x - mu| d_r) + EPI_REL (|gamma| r (|x| + |mu|) + |beta|).

The first term is the error of the statistics carried to the output.  The second, EPI_REL = 16 u as for dd_gemm's
epilogue, covers the few fp32 roundings of sc, sh and x sc + sh, each relative to the magnitude of ITS operands: x sc and
mean sc cancel when |mu| >> sigma, so the term does not shrink with |x - mu|.  LayerNorm stores
(x - mean) rstd gamma + beta, where nothing cancels:  EPI_REL (|ref - beta| + |beta|).
With SiLU (Lipschitz constant max |silu'| = 1.0998 < SILU_LIP):  E <- SILU_LIP E + EPI_REL |silu(ref)|.

No constant above is fitted to a measurement: each is one the project already uses, or follows from the arithmetic
named next to it.  On an fp32 emulation of the kernels' arithmetic (tests/test_norm_reference_cpu.py) the largest
err / bound is 0.5, pure output rounding; E is 0 - 25 % of the bound without SiLU and up to about half of it on data with
a large common offset.

What this bound CANNOT see: an error of the statistics below one output unit — a pixel missing from a group of more
than about 2^11 (fp16) / 2^8 (bf16) elements moves nothing by a whole unit unless the pixel is an outlier, hence the
`spike` data; the pivot: statistics without it pass whenever |mean| is within a few sigma (randn, spike), and on
`offset` data bf16 sees their loss only just (2 to 8 times the bound on about 1 % of the elements of a small group,
against 7 to 34 times on 10 - 25 % in fp16), because its output unit is eight times wider; on
`offset` data E itself grows with |mu| r (the x sc + sh cancellation is real), so faults there are seen less sharply
than on zero-mean data; and which of the kernels produced a result — the tests' case table asserts the form each shape
takes.
"""
import torch
import torch.nn.functional as F

from tests.gemm_reference import EPI_REL, SILU_LIP, TAU, check, nan_like, rand, ulp  # noqa: F401  (re-exported for the tests)

TAU_LN = 2.0 ** -18
RSQRT_REL = 2.0 ** -22
REL_MAX = 2.0 ** -6


def _rstd_error(e_var, var, eps, what):
    rel = e_var / (2.0 * (var + eps))
    if not bool((rel < REL_MAX).all()):
        raise AssertionError("%s: relative variance error %.3g is not small: the first-order bound does not apply"
                             % (what, float(rel.max())))
    return rel * (1.0 + 4.0 * rel) + RSQRT_REL


def groupnorm_reference(x1, gamma, beta, m, hw, groups, eps, silu, x2=None):
    """x1 (m * hw, c1), x2 (m * hw, c2) or None, gamma / beta (c,) in the storage type -> (ref, E), each (m * hw, c)
    float64, E the bound on the fp32 value before the output rounding."""
    x = x1 if x2 is None else torch.cat([x1, x2], dim=1)
    c = x.shape[1]
    cpg = c // groups
    X = x.to(torch.float64).reshape(m, hw, groups, cpg)
    G = gamma.to(torch.float64).reshape(1, 1, groups, cpg)
    B = beta.to(torch.float64).reshape(1, 1, groups, cpg)
    p = X[:, 0:1, :, 0:1]
    mu = X.mean(dim=(1, 3), keepdim=True)
    var = ((X - mu) ** 2).mean(dim=(1, 3), keepdim=True)
    a1 = (X - p).abs().mean(dim=(1, 3), keepdim=True)
    dm = (mu - p).abs()
    r = 1.0 / torch.sqrt(var + eps)
    d_mu = TAU * a1
    e_var = TAU * (var + dm * dm) + 2.0 * dm * d_mu + d_mu * d_mu
    d_r = _rstd_error(e_var, var, eps, "groupnorm")
    ref = (X - mu) * r * G + B
    e = G.abs() * r * (d_mu + (X - mu).abs() * d_r) + EPI_REL * (G.abs() * r * (X.abs() + mu.abs()) + B.abs())
    if silu:
        ref = F.silu(ref)
        e = SILU_LIP * e + EPI_REL * ref.abs()
    return ref.reshape(m * hw, c), e.reshape(m * hw, c)


def layernorm_reference(x, gamma, beta, eps):
    """x (rows, c), gamma / beta (c,) in the storage type -> (ref, E), each (rows, c) float64."""
    X = x.to(torch.float64)
    G = gamma.to(torch.float64)[None, :]
    B = beta.to(torch.float64)[None, :]
    mu = X.mean(dim=1, keepdim=True)
    var = ((X - mu) ** 2).mean(dim=1, keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    d_mu = TAU_LN * X.abs().mean(dim=1, keepdim=True)
    d_r = _rstd_error(TAU_LN * var + d_mu * d_mu, var, eps, "layernorm")
    ref = (X - mu) * r * G + B
    e = G.abs() * r * (d_mu + (X - mu).abs() * d_r) + EPI_REL * ((ref - B).abs() + B.abs())
    return ref, e


def settled(ref, e, dtype):
    """(mask, value): the elements whose correctly rounded output does not depend on where inside [ref - e, ref + e] the
    fp32 value fell, and that output.  There the kernel has ONE right answer; `const` data (var = 0, ref = act(beta)) is
    compared bit for bit on them."""
    lo, hi = (ref - e).to(dtype), (ref + e).to(dtype)
    return lo == hi, lo


# ---- data ------------------------------------------------------------------------------------------------------------

KINDS = ("randn", "offset", "spike", "const")


def _gen(seed, device):
    return torch.Generator(device=device).manual_seed(seed)


def affine(c, dtype, seed, device):
    """gamma = 1 + randn, beta = randn, in the storage type."""
    g = _gen(seed, device)
    gamma = 1.0 + torch.randn((c,), generator=g, device=device, dtype=torch.float32)
    beta = torch.randn((c,), generator=g, device=device, dtype=torch.float32)
    return gamma.to(dtype), beta.to(dtype)


def groupnorm_data(kind, m, hw, c, groups, dtype, seed, device):
    """(m * hw, c) in the storage type.  randn: N(0.5, 1).  offset: a per-(instance, group) level 100 + 60 randn plus unit
    noise (|mean| ~ 100 sigma, as real SD checkpoints have).  spike: N(0, 1) with the last pixel and pixel hw // 2 times
    32 (a pixel left out of, or counted twice in, the statistics moves them by far more than rounding).  const: one
    value 2^-12 randn per (instance, group): var = 0 exactly, and |x| r stays below one so that act(beta) is the ONE
    right answer almost everywhere (settled())."""
    g = _gen(seed, device)
    cpg = c // groups
    rn = lambda *shape: torch.randn(shape, generator=g, device=device, dtype=torch.float32)
    if kind == "randn":
        x = rn(m, hw, groups, cpg) + 0.5
    elif kind == "offset":
        x = rn(m, 1, groups, 1) * 60.0 + 100.0 + rn(m, hw, groups, cpg)
    elif kind == "spike":
        x = rn(m, hw, groups, cpg)
        x[:, hw - 1] *= 32.0
        x[:, hw // 2] *= 32.0
    elif kind == "const":
        x = (rn(m, 1, groups, 1) * 2.0 ** -12).expand(m, hw, groups, cpg)
    else:
        raise ValueError(kind)
    return x.reshape(m * hw, c).to(dtype).contiguous()


def layernorm_data(kind, rows, c, dtype, seed, device):
    """As groupnorm_data with a row in place of a group; spike: the last channel times 32."""
    g = _gen(seed, device)
    rn = lambda *shape: torch.randn(shape, generator=g, device=device, dtype=torch.float32)
    if kind == "randn":
        x = rn(rows, c) + 0.5
    elif kind == "offset":
        x = rn(rows, 1) * 60.0 + 100.0 + rn(rows, c)
    elif kind == "spike":
        x = rn(rows, c)
        x[:, c - 1] *= 32.0
    elif kind == "const":
        x = (rn(rows, 1) * 2.0 ** -12).expand(rows, c)
    else:
        raise ValueError(kind)
    return x.to(dtype).contiguous()


# ---- reporting -------------------------------------------------------------------------------------------------------

def report_line(name, ratios, means):
    return "%-34s launches %3d   max err/bound %.3f   mean err/bound %.4f" % (
        name, len(ratios), max(ratios) if ratios else 0.0, (sum(means) / len(means)) if means else 0.0)


def mean_ratio(y, ref, e, out_dtype=None):
    b = ulp(ref, out_dtype or y.dtype) + e
    return float(((y.to(torch.float64) - ref).abs() / b).mean())
