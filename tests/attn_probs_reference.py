"""fp64 reference and per-element error bound for dd_attn_probs (csrc/attn_probs.hip), shared by the attention-probability
and attention-map tests.  Pattern and constants (`TAU`, `ARG_REL`, `EXP_REL`, `ulp`, `check`) are attention_reference's.

Reference
---------
Computed in float64 from the SAME fp16 / bf16 operands the kernel reads, as canonical [batches, heads, rows, d] VIEWS
(attention_reference.rows_view / head_major_view) of whatever layout the kernel was handed:

    t = c q k^T  (log2 units, c = scale log2 e),   w = softmax_j(t ln 2)  over the first n keys,
    per_head:  ref = weight w                      mean:  ref = (weight / heads) sum_h w          (+ old: accumulate)

q_prescaled: the operand is the STORED prescaled q and c = 1 exactly, which is also what the kernel multiplies by.
`weight` is taken as the fp32 value the launcher receives (a C float argument).

Bound
-----
Per element, |y - ref| <= ulp_f32(ref) + E (gemm_reference.check); u = 2^-24.  E follows the kernel's arithmetic.

Scores.  Products of fp16 / bf16 operands are exact in fp32; their fp32 sum over d <= 160 in the MFMA chain is off by at
most TAU ||q_i|| ||k_j|| (Cauchy-Schwarz, TAU = 256 u as for dd_gemm): in log2 units
        eps_s = TAU (c ||q_i|| ||k_j|| + [prescaled] A_i),      A_i = max_j |t_ij|.
(The A_i term is the room the contract leaves a prescaled form that starts its MFMA chain from the negated maximum, as
dd_attn5 does; this kernel starts every chain from zero and does not use it.)

Argument.  The row maximum mx is the EXACT maximum of the n fp32 scores: no running maximum, no lazy threshold, no
rescale — none of attention_reference's THR or per-rescale terms.  m = fl(mx c) and x = fma(s, c, -m): whatever error m
carries is the SAME for every key of the row and cancels in the normalisation exactly.  What does not cancel: c is an fp32
product of two rounded values (<= 3 u relative) and stretches (t_ij - M_i); the fma rounds once, relative to
|x| <= |t_ij - M_i| (+ the common |m| u, whose rounding u^2 |M_i| is below 2^-28 for any |M_i| < 2^20 and sits inside
EXP_REL).  Together fewer than ARG_REL = 16 u roundings relative to |t_ij - M_i|.  v_exp_f32 is accurate to one fp32 unit:
EXP_REL = 2^-22, ONCE.  So the unnormalised p_ij carries the relative error
        delta_ij = expm1( ln2 (eps_s + ARG_REL |t_ij - M_i|) ) (1 + EXP_REL) + EXP_REL.
No u_P term and no storage-type subnormal term: the probabilities are never rounded to the storage type, and the output
is fp32.  What remains of the number format is its own floor: v_exp_f32 and the multiplies may flush a result below the
fp32 normal range to zero, an ABSOLUTE error of at most FLUSH32 = 2^-126 per weight (1e-38: it only matters where the
reference itself is that small, i.e. for keys more than 126 log2 units under the row maximum).

Normalisation.  w'_ij / w_ij = (1 + delta_ij) / sum_k w_ik (1 + delta_ik), so with dbar_i = sum_k w_ik delta_ik (< 1/2,
asserted) the weight is off by at most w_ij (delta_ij + dbar_i) / (1 - dbar_i).  The denominator is the fp32 sum of the n
unrounded p (all positive: at most (n - 1) u relative), then one division and one multiply: (n + 8) u relative.
        E_w = w_ij ( (delta_ij + dbar_i) / (1 - dbar_i) + (n + 8) u ) + FLUSH32.

Output.  per_head: P = weight w, one multiply whose rounding is check's ulp term: E = |weight| E_w.
Head mean: an fp32 sum of `heads` weights in head order (heads - 1 adds, each at most u of the running sum <= sum_h w),
times fl(weight / heads) (one rounding of the quotient); the final multiply is the ulp term:
        E = |weight / heads| ( sum_h E_w + (heads + 2) u sum_h w ).
Accumulate: P = old + value.  The value is rounded before the add (or not at all, where the compiler fuses the two into
one fma) and the add's own rounding is the ulp term of the total: one fp32 add per call,
        E += u (|old| + |value|).

No constant above is fitted to a measurement.  What this bound CANNOT see: a fault that changes a weight by less than
delta — with eps_s around 2^-16 c ||q|| ||k||, a relative 1e-4 at the norms of the test data: a mis-scaled chunk of keys,
a wrong head in the mean or a key past n that leaks into the sum are all far outside it, a swapped pair of equal-scoring
keys is not.  On near-uniform rows (small scores) every weight is about 1 / n and a permutation of the KEYS of a row would
pass: hence the test data include peaked softmaxes and one dominant key at the last valid position.
"""
import torch

from tests.attention_reference import (ARG_REL, EXP_REL, LN2, LOG2E, TAU, U32, head_major_view,  # noqa: F401  (re-exported)
                                       rows_view)
from tests.gemm_reference import check, nan_like, rand, ulp  # noqa: F401  (re-exported for the tests)

FLUSH32 = 2.0 ** -126


def weights(q4, k4, scale, n_keys=None, prescaled=False):
    """q4 [B, H, lq, d], k4 [B, H, >= n, d] storage-type (or float64) views -> (w, E_w), each [B, H, lq, n] float64."""
    n = k4.shape[2] if n_keys is None else int(n_keys)
    c = 1.0 if prescaled else float(scale) * LOG2E
    q = q4.to(torch.float64)
    k = k4[:, :, :n].to(torch.float64)
    t = c * (q @ k.transpose(2, 3))
    x = t - t.amax(dim=3, keepdim=True)
    p = torch.exp2(x)
    w = p / p.sum(dim=3, keepdim=True)
    eps = TAU * c * q.norm(dim=3)[..., :, None] * k.norm(dim=3)[..., None, :]
    if prescaled:
        eps = eps + TAU * t.abs().amax(dim=3, keepdim=True)
    delta = torch.expm1(LN2 * (eps + ARG_REL * x.abs())) * (1 + EXP_REL) + EXP_REL
    dbar = (w * delta).sum(dim=3, keepdim=True)
    if not bool((dbar < 0.5).all()):
        raise AssertionError("weight error bound %.3g is not small: the first-order bound does not apply" % float(dbar.max()))
    return w, w * ((delta + dbar) / (1 - dbar) + (n + 8) * U32) + FLUSH32


def reference(q4, k4, scale, *, n_keys=None, prescaled=False, per_head=False, weight=1.0, old=None):
    """-> (ref, E) float64: [B, H, lq, n] with per_head, else [B, lq, n].  old: what an accumulating call found in the
    output (the same shape), taken as exact; accumulated() chains the bounds of successive calls instead."""
    w, e = weights(q4, k4, scale, n_keys, prescaled)
    heads = q4.shape[1]
    wt = float(torch.tensor(float(weight), dtype=torch.float32))
    if per_head:
        ref, e = wt * w, abs(wt) * e
    else:
        wh = wt / heads
        s = w.sum(dim=1)
        ref, e = wh * s, abs(wh) * (e.sum(dim=1) + (heads + 2) * U32 * s)
    if old is not None:
        od = old.to(torch.float64)
        e = e + U32 * (od.abs() + ref.abs())
        ref = ref + od
    return ref, e


def accumulated(calls):
    """calls: [(ref, E), ...] of successive accumulate = 1 launches into a zeroed output -> (ref, E) of the total:
    the fp64 sum, and each call's own bound plus its one fp32 add."""
    ref = e = None
    for r, er in calls:
        if ref is None:
            ref, e = r.clone(), er + U32 * r.abs()
        else:
            e = e + er + U32 * (ref.abs() + r.abs())
            ref = ref + r
    return ref, e
