"""fp64 reference and per-element error bound for dd_attention (dd_attn5_kernel) and the attention core of dd_xattn320,
shared by the attention tests.  `ulp`, `check`, `nan_like`, `rand` are gemm_reference's.

Reference
---------
Computed in float64 from the SAME fp16 / bf16 operands the kernel reads, on the device that holds them, one group of
(batch, head) planes at a time (a group is as many planes as keep the score matrices under PLANE_ELEMS elements; every
plane is computed on its own, the group only saves Python round trips):

    t = c q k^T  (log2 units, c = scale log2 e),   w = softmax_j(t ln 2),   o = w v

over the first `n_keys` keys.  Operands are canonical 4-D VIEWS [batches, heads, rows, d] of whatever layout the kernel
was handed (rows_view / head_major_view / seq_view below; a batch-major operand is already one), so the reference reads
the bytes the kernel reads.  kv_map redirects batch b to the K / V of batch kv_map[b]; with kv_map2 the result is the
fp64 SUM of the two independent softmaxes; `old` (accumulate) is added in fp64.  q_prescaled: the operand is the STORED
prescaled q and scale = ln 2, i.e. c = 1 exactly, which is also what the kernel multiplies by.

Bound
-----
Per element, |y - ref| <= ulp_out(ref) + E (gemm_reference.check).  E follows the kernel's arithmetic; u = 2^-24.

Scores.  The products of fp16 / bf16 operands are exact in fp32 and their fp32 sum over d <= 160 (+ the C operand) is off
by at most (depth) u sum|q k| <= TAU ||q_i|| ||k_j|| (Cauchy-Schwarz, TAU = 256 u as for dd_gemm), in log2 units
        eps_s = TAU (c ||q_i|| ||k_j|| + [prescaled] A_i).
The prescaled form starts the MFMA chain from -m_run, so the partial sums also carry |m_run| <= A_i = max_j |t_ij| + THR
(THR = 5: the lazy rescale lets the running max trail the true one by that much).
The argument of v_exp_f32 is x = fma(s, c, -m_run).  c is an fp32 product of two rounded fp32 values (<= 3 u relative) and
is the SAME for every key of the row, so it stretches (t_j - M_i), not t_j; the fma rounds relative to |x| <= |t_j - M_i|
+ THR; every rescale multiplies what is already summed by exp2(m_old - m_new), whose subtractions telescope to at most
|t_j - M_i| + THR: together fewer than ARG_REL = 16 u roundings relative to (|t_ij - M_i| + THR).  v_exp_f32 is accurate
to one fp32 unit (EXP_REL = 2^-22 covers it and the product with alpha), once for p and once per rescale; the number of
rescales is at most the number of 32-key chunks nch (any row of a 16-row block triggers the block).  In the prescaled
form m_run += mx rounds at |m_run| <= A_i per rescale, which shifts later scores against earlier ones: nch u A_i.  So the
unnormalised probability of key j carries the relative error
        delta_ij = ln2 (eps_s + ARG_REL (|t_ij - M_i| + THR) + [prescaled] nch u A_i) + (1 + nch) EXP_REL + u_P,
u_P = 2^-11 (fp16) / 2^-8 (bf16): P is rounded to the storage type before the PV product.
fp16 only: p < 2^-14 is subnormal in the storage type and rounds with an ABSOLUTE error of 2^-25.  The denominator is
>= 1: the key that last set the running max has x = 0, p = 1, and later rescales have alpha <= 1 only when another key
takes that role.  p is taken against a running max <= M_i, so only keys with t_ij - M_i < -13.9 can be subnormal: they
get a_ij = w_ij delta_ij + 2^-25.  (bf16 and fp32 flush below 2^-126: nothing next to one output unit.)

Weights -> output.  With a_ij the absolute error of the normalised weight and abar_i = sum_j a_ij:
  * d = 80 / 160 round P for the numerator and sum the UNROUNDED p in l_run for the denominator:
        E_P = sum_j a_ij (|v_jd| + |o_id|) / (1 - abar_i);
  * d = 40 takes the denominator from the same rounded P (a ones column of V), so the output is an exact weighted mean
    under perturbed weights, o' - o = sum_j dP_j (v_j - o) / sum P':
        E_P = sum_j a_ij |v_jd - o_id| / (1 - abar_i) <= sqrt(abar_i sum_j a_ij (v_jd - o_id)^2) / (1 - abar_i)
    (Cauchy-Schwarz, so that it stays three matrix products); the smaller of this and the general form is used.
PV accumulation in fp32 over lk keys, nch rescales (and l_run / the ones column likewise):
        E_acc = (lk + nch + 8) u (sum_j w_ij |v_jd| + |o_id|);
the reciprocal, the normalising multiply, and for the pair / accumulate the fp32 adds (the old output converted exactly):
EPI_REL = 16 u times |o| (+ |o_1| + |o_2|, + |old|).  The pair's E is E_1 + E_2.

No constant above is fitted to a measurement.  What this bound CANNOT see: any fault that changes a weight by less than
delta (2^-8 in bf16: a 2 % mis-scaled 32-key chunk stays inside it, in fp16 it does not), and on zero-mean V the worst
case sum_j a_ij |v_jd - o_id| is 10 to 50 output units wide because the roundings it allows for never line up; on V with
a common offset (d = 40) it is a few units.  Hence the test data include offset V and peaked softmaxes.
"""
import math

import torch

from tests.gemm_reference import EPI_REL, TAU, check, nan_like, rand, ulp  # noqa: F401  (re-exported for the tests)

U32 = 2.0 ** -24
ARG_REL = 2.0 ** -20
EXP_REL = 2.0 ** -22
THR = 5.0
U_P = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
SUBN = 2.0 ** -25
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
PLANE_ELEMS = 1 << 22


# ---- canonical [batches, heads, rows, d] views of the kernel's operand layouts -------------------------------------------

def rows_view(t, batch, l, heads, d):
    """(batch*l, >= heads*d) row-strided 2-D operand (a column slice of a wider buffer)."""
    return t[:, :heads * d].unflatten(0, (batch, l)).unflatten(2, (heads, d)).permute(0, 2, 1, 3)


def head_major_view(t, batch, l, heads, d):
    """(heads, batch*l, d) planes."""
    return t.unflatten(1, (batch, l)).permute(1, 0, 2, 3)


def seq_view(t, batch, l, heads, d, row_stride, batch_stride):
    """2-D operand walked with seq_strides = (row_stride, batch_stride): element (b, h, i, e) at b*bs + i*rs + h*d + e."""
    return torch.as_strided(t, (batch, heads, l, d), (batch_stride, d, row_stride, 1), t.storage_offset())


# ---- reference + bound -----------------------------------------------------------------------------------------------

def _one(q, k, v, c, dtype, pre, ones, dscore=None):
    """q (G, lq, d), k / v (G, lk, d) float64 -> (o, E) without the pair / accumulate terms.  dscore (G, lq, lk): an extra
    absolute error of the scores in log2 units (dd_xattn320: q itself is a rounded intermediate)."""
    lk = k.shape[1]
    nch = (lk + 31) // 32
    t = c * (q @ k.transpose(1, 2))
    big = t.abs().amax(dim=2, keepdim=True) + THR
    x = t - t.amax(dim=2, keepdim=True)
    p = torch.exp2(x)
    w = p / p.sum(dim=2, keepdim=True)
    o = w @ v
    eps = TAU * c * q.norm(dim=2)[:, :, None] * k.norm(dim=2)[:, None, :]
    arg = eps + ARG_REL * (THR - x)
    sub_below = -13.9
    if dscore is not None:
        arg = arg + dscore
        sub_below = sub_below + 2 * dscore.amax(dim=2, keepdim=True)
    if pre:
        arg = arg + (TAU + nch * U32) * big
    a = w * (LN2 * arg + (1 + nch) * EXP_REL + U_P[dtype])
    if dtype == torch.float16:
        a = a + SUBN * (x < sub_below)
    del t, x, p, arg, eps
    abar = a.sum(dim=2, keepdim=True)
    if not bool((abar < 0.5).all()):
        raise AssertionError("weight error bound %.3g is not small: the first-order bound does not apply" % float(abar.max()))
    av = a @ v.abs()
    e_p = av + abar * o.abs()
    if ones:
        mid = v.mean(dim=1, keepdim=True)                 # (v - o) = (v - mid) - (o - mid): no cancellation on offset V
        vc, oc = v - mid, o - mid
        var = (a @ (vc * vc) - 2 * oc * (a @ vc) + oc * oc * abar).clamp(min=0)
        e_p = torch.minimum(e_p, torch.sqrt(abar * var))
    e_p = e_p / (1 - abar)
    e_acc = (lk + nch + 8) * U32 * (w @ v.abs() + o.abs())
    return o, e_p + e_acc + EPI_REL * o.abs()


def reference(q4, k4, v4, scale, *, kv_map=None, kv_map2=None, old4=None, n_keys=None, prescaled=False, planes=None):
    """q4 [B, H, lq, d], k4 / v4 [Bk, H, lk, d] storage-type views; old4 [B, H, lq, d] (accumulate) or None; planes: list of
    flat plane indices b * H + h to compute (None = all).  -> (ref, E), each [len(planes), lq, d] float64."""
    dtype = q4.dtype
    B, H, lq, d = q4.shape
    lk = k4.shape[2] if n_keys is None else int(n_keys)
    c = 1.0 if prescaled else float(scale) * LOG2E
    ones = d % 16 != 0
    planes = list(range(B * H)) if planes is None else list(planes)
    dev = q4.device
    maps = [None if m is None else m.to("cpu").tolist() for m in (kv_map, kv_map2)]
    group = max(1, PLANE_ELEMS // (lq * lk))
    refs, errs = [], []
    for g0 in range(0, len(planes), group):
        pl = planes[g0:g0 + group]
        bi = torch.tensor([p // H for p in pl], device=dev)
        hi = torch.tensor([p % H for p in pl], device=dev)
        q = q4[bi, hi].to(torch.float64)
        ref = e = None
        for m in (maps if maps[1] is not None else maps[:1]):
            kb = bi if m is None else torch.tensor([m[p // H] for p in pl], device=dev)
            k = k4[kb, hi, :lk].to(torch.float64)
            v = v4[kb, hi, :lk].to(torch.float64)
            o, eo = _one(q, k, v, c, dtype, prescaled, ones)
            if ref is None:
                ref, e = o, eo
            else:
                e = e + eo + EPI_REL * (ref.abs() + o.abs())
                ref = ref + o
        if old4 is not None:
            od = old4[bi, hi].to(torch.float64)
            e = e + EPI_REL * (ref.abs() + od.abs())
            ref = ref + od
        refs.append(ref)
        errs.append(e)
    return torch.cat(refs), torch.cat(errs)


def xattn_reference(x, wq, wo, bo, k4, v4, scale, res=None, n_keys=None):
    """dd_xattn320 without ln_out: out = (softmax(scale (x Wq^T)_h K_h^T) V_h)_h Wo^T + bo + res in float64 and its bound.
    x (inst * n, 320), wq / wo the RAW (320, 320) weights, k4 / v4 [inst, 8, lk, 40] views.  The kernel's chain, csrc/xattn.hip:
      * q = (x Wq^T) scale log2 e from an fp32 accumulator, ROUNDED to the storage type: the stored q is within
        e_q = ulp(q) + c TAU ||x_i|| ||wq_n|| + EPI_REL |q| of the fp64 q, so every score is off by up to
        sum_e e_q[i, e] |k[j, e]| (log2 units) on top of its own fp32 accumulation — `dscore` of _one;
      * one-pass softmax (all <= 128 keys resident), the row sum taken from the ROUNDED probabilities: the d = 40 form of
        the module docstring (an exact weighted mean under perturbed weights); a shift common to a row's scores cancels;
      * the attention output is rounded to the storage type before the out projection: E_O = E_attention + ulp(o);
      * out projection from an fp32 accumulator: E_O |Wo|^T (worst case over the 320 channels: this is what makes the
        bound wide, some tens of output units) + TAU ||o_i|| ||wo_m||, then bias and residual in fp32 (EPI_REL)."""
    dtype = x.dtype
    inst, heads, lk_cap, d = k4.shape
    lk = lk_cap if n_keys is None else int(n_keys)
    n = x.shape[0] // inst
    c = float(scale) * LOG2E
    X, Wq, Wo = x.to(torch.float64), wq.to(torch.float64), wo.to(torch.float64)
    q = (X @ Wq.t()) * c
    e_q = ulp(q, dtype) + c * TAU * torch.outer(X.norm(dim=1), Wq.norm(dim=1)) + EPI_REL * q.abs()
    planes = lambda t: t.view(inst, n, heads, d).permute(0, 2, 1, 3).reshape(inst * heads, n, d)
    K = k4[:, :, :lk].to(torch.float64).reshape(inst * heads, lk, d)
    V = v4[:, :, :lk].to(torch.float64).reshape(inst * heads, lk, d)
    o, e_o = _one(planes(q), K, V, 1.0, dtype, False, True, dscore=planes(e_q) @ K.abs().transpose(1, 2))
    e_o = e_o + ulp(o, dtype)
    rows = lambda t: t.view(inst, heads, n, d).permute(0, 2, 1, 3).reshape(inst * n, heads * d)
    o, e_o = rows(o), rows(e_o)
    acc = o @ Wo.t()
    e = e_o @ Wo.abs().t() + TAU * torch.outer(o.norm(dim=1) + e_o.norm(dim=1), Wo.norm(dim=1))
    mag = acc.abs()
    ref = acc
    for t in (bo, res):
        if t is not None:
            ref = ref + t.to(torch.float64)
            mag = mag + t.to(torch.float64).abs()
    return ref, e + EPI_REL * mag


def take_planes(y4, planes=None):
    """[B, H, lq, d] view of an output -> [len(planes), lq, d] in reference()'s order."""
    B, H = y4.shape[:2]
    if planes is None:
        return y4.reshape(B * H, y4.shape[2], y4.shape[3])
    idx = torch.tensor(list(planes), device=y4.device)
    return y4[idx // H, idx % H]


def xcd_sample(batch, heads, lq, rows_per_wg):
    """Planes to compare when a case has more than 96 of them: every even plane, the first and the last, and the planes on
    both sides of each boundary of the kernel's workgroup -> item mapping (blockIdx.x & 7 selects one of eight contiguous
    item ranges: attention.hip)."""
    nqb = -(-lq // rows_per_wg)
    nwg = nqb * batch * heads
    xq, xr = nwg >> 3, nwg & 7
    keep = set(range(0, batch * heads, 2)) | {0, batch * heads - 1}
    for xcd in range(1, 9):
        start = xcd * (xq + 1) if xcd < xr else xr * (xq + 1) + (xcd - xr) * xq
        for item in (start - 1, start):
            if 0 <= item < nwg:
                keep.add(item // nqb)
    return sorted(keep)


def report_line(name, ratios, means):
    return "%-28s launches %3d   max err/bound %.3f   mean err/bound %.4f" % (
        name, len(ratios), max(ratios) if ratios else 0.0, (sum(means) / len(means)) if means else 0.0)


def mean_ratio(y, ref, e, out_dtype=None):
    b = ulp(ref, out_dtype or y.dtype) + e
    return float(((y.to(torch.float64) - ref).abs() / b).mean())


def softmax_scale(d):
    return 1.0 / math.sqrt(d)
