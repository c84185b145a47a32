"""dd_attn_probs through ops.attention_probs: every element against the fp64 reference and bound of attn_probs_reference.py.

CASES crosses the eight key counts (1, both sides of the 78-token base context, a 16-key tile boundary on both sides, the
five-bucket context 238 and the limit 256) with head_dim 40 / 80 / 160 at 2 and 8 heads and both dtypes, and cycles the rest
through them so that every value meets varied company: lq in {1, 28, 35, 91} (a single row, partial 16-row blocks, several
blocks), the two operand layouts Attention.run_cross produces (row-major column slices with `scale`; head-major prescaled
q), per-head and head-mean output, an output pitch that takes the 16-byte stores and one that takes the scalar ones, and
the data families of the attention tests:
  randn   ordinary scores;
  peaked  three times the operand magnitude: a few keys carry the row, most weights are tiny (the exp2 argument term);
  offset  a large score offset common to a row (80 - 160 log2 units): the maximum subtraction, and the prescaled A_i term;
  spike   one dominant key at the LAST valid position: the ragged 16-key tile, the tail mask, the key count itself.
Operands are slices of wider NaN-filled buffers (a read outside the slice poisons the result); outputs sit in a
NaN-filled frame (pitch padding, guard rows above and below, a guard batch entry) that must come back intact."""
import collections
import itertools

import pytest
import torch

from dualdiff_amd import ops
from tests import attn_probs_reference as AR

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
LKS = [1, 77, 78, 110, 128, 129, 238, 256]
HEADS_DIMS = [(2, 40), (8, 40), (2, 80), (8, 80), (2, 160), (8, 160)]
LQS = [1, 28, 35, 91]
KINDS = ["randn", "peaked", "offset", "spike"]
Case = collections.namedtuple("Case", "dtype lk heads d lq kind hm per_head vec")


def cases():
    out = []
    for di, li, hi in itertools.product(range(len(DTYPES)), range(len(LKS)), range(len(HEADS_DIMS))):
        heads, d = HEADS_DIMS[hi]
        out.append(Case(DTYPES[di], LKS[li], heads, d, LQS[(li + hi) % 4], KINDS[(li + 2 * hi + di) % 4],
                        bool((li + hi // 2 + di) % 2), bool((li // 2 + hi) % 2), bool((li + hi + hi // 2) % 2)))
    return out


def test_case_table_covers_what_it_claims():
    cs = cases()
    for dtype in DTYPES:
        mine = [c for c in cs if c.dtype == dtype]
        assert {(c.lk, c.heads, c.d) for c in mine} == set((lk, h, d) for lk in LKS for h, d in HEADS_DIMS)
        for field, values in (("lq", LQS), ("kind", KINDS), ("hm", [False, True]), ("per_head", [False, True]),
                              ("vec", [False, True])):
            for d in (40, 80, 160):
                assert {getattr(c, field) for c in mine if c.d == d} == set(values), (dtype, d, field)
            for lk in LKS:
                assert len({getattr(c, field) for c in mine if c.lk == lk}) > 1, (dtype, lk, field)


# ---- data, layouts, outputs --------------------------------------------------------------------------------------------

def _randn(shape, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(shape, generator=g, device=dev, dtype=torch.float32)


def make_qk(kind, b, h, lq, lk, n, d, dtype, pre, seed, dev):
    """Canonical q [b, h, lq, d], k [b, h, lk, d] in the storage type; q as STORED (prescaled when pre).  n: valid keys."""
    q, k = _randn((b, h, lq, d), seed, dev), _randn((b, h, lk, d), seed + 1, dev)
    if kind == "peaked":
        q, k = q * 3.0, k * 3.0
    elif kind == "offset":                              # every score of a row shares 9 sqrt(d) (natural units)
        q, k = q + 3.0, k + 3.0
    elif kind == "spike":                               # the last valid key dominates row 0 (and scores high elsewhere)
        k[:, :, n - 1] = q[:, :, 0] * 4.0
    if pre:
        q = q * (d ** -0.5 * AR.LOG2E)
    return q.to(dtype), k.to(dtype)


def lay_rows(t4, dev):
    """[b, h, l, d] -> the middle third of a [b * l, 3 C] NaN buffer (a column slice of a fused projection) + its view."""
    b, h, l, d = t4.shape
    c = h * d
    buf = AR.nan_like((b * l, 3 * c), t4.dtype, dev)
    op = buf[:, c:2 * c]
    AR.rows_view(op, b, l, h, d).copy_(t4)
    return op, AR.rows_view(op, b, l, h, d)


def lay_hm(t4, dev):
    """[b, h, l, d] -> planes h .. 2h-1 of a (3 h, b * l, d) NaN buffer (the Q planes of a head-major projection)."""
    b, h, l, d = t4.shape
    buf = AR.nan_like((3 * h, b * l, d), t4.dtype, dev)
    op = buf[h:2 * h]
    AR.head_major_view(op, b, l, h, d).copy_(t4)
    return op, AR.head_major_view(op, b, l, h, d)


def framed_out(b, heads, lq, lk, vec, dev, fill=float("nan")):
    """(frame, out): out (b, [heads,] lq, lk) inside a filled frame with a guard batch entry, a guard row above and below
    every (batch, head) block and pitch padding.  vec: rows start 16-byte aligned (pitch % 4 == 0), else they do not."""
    pitch = (lk + 3) // 4 * 4 + (4 if vec else 5)
    lead = (b + 1,) if heads is None else (b + 1, heads)
    frame = torch.full(lead + (lq + 2, pitch), fill, dtype=torch.float32, device=dev)
    return frame, frame[:b, ..., 1:lq + 1, :lk]


def frame_intact(frame, out, fill=float("nan")):
    b, lq, lk = out.shape[0], out.shape[-2], out.shape[-1]
    guard = torch.ones_like(frame, dtype=torch.bool)
    guard[:b, ..., 1:lq + 1, :lk] = False
    g = frame[guard]
    return bool(torch.isnan(g).all()) if fill != fill else bool((g == fill).all())


def launch(c, q, k, b, lk, out, **kw):
    scale = None if c.hm else c.d ** -0.5
    return ops.attention_probs(q, k, b, c.lq, lk, c.heads, c.d, scale, q_prescaled=c.hm, per_head=c.per_head, out=out, **kw)


# ---- every element ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", cases(), ids=lambda c: "%s-lk%d-h%dd%d-lq%d-%s-%s-%s-%s" % (
    str(c.dtype)[6:], c.lk, c.heads, c.d, c.lq, c.kind, "hm" if c.hm else "rows", "heads" if c.per_head else "mean",
    "vec" if c.vec else "scalar"))
def test_every_element_within_the_bound(gpu, c):
    b = 3
    q4, k4 = make_qk(c.kind, b, c.heads, c.lq, c.lk, c.lk, c.d, c.dtype, c.hm, 100 + c.lk + c.d, gpu)
    q, qv = (lay_hm if c.hm else lay_rows)(q4, gpu)
    k, kv = lay_rows(k4, gpu)
    ref, e = AR.reference(qv, kv, c.d ** -0.5, prescaled=c.hm, per_head=c.per_head)
    frame, out = framed_out(b, c.heads if c.per_head else None, c.lq, c.lk, c.vec, gpu)
    launch(c, q, k, b, c.lk, out)
    ratio = AR.check(out, ref, e, str(c), torch.float32)
    print("%s: max err/bound %.3f" % (c, ratio))
    assert frame_intact(frame, out)
    # The rows are probability distributions (their head mean in mean mode), and their sum does not depend on the score
    # errors at all: sum_j p_j / fl(sum p) is off by the fp32 sum (n - 1 adds), the division and the multiply, the head sum
    # adds heads - 1 roundings, the stores at most 2 u in total.  A fault the per-element bound could hide in many small
    # weights shows here.
    assert float((out.double().sum(-1) - 1).abs().max()) <= (c.lk + c.heads + 12) * AR.U32
    frame2, out2 = framed_out(b, c.heads if c.per_head else None, c.lq, c.lk, c.vec, gpu)
    launch(c, q, k, b, c.lk, out2)
    assert torch.equal(out, out2)                        # no atomics: the same bits on a second run


def test_head_major_keys_and_default_output(gpu):
    """k as head-major planes too (ops accepts what ops.attention accepts), and out=None: a fresh (batch, lq, lk) tensor."""
    dtype, b, h, d, lq, lk = torch.float16, 2, 8, 40, 35, 78
    q4, k4 = make_qk("randn", b, h, lq, lk, lk, d, dtype, True, 7, gpu)
    q, qv = lay_hm(q4, gpu)
    k, kv = lay_hm(k4, gpu)
    ref, e = AR.reference(qv, kv, None, prescaled=True)
    out = ops.attention_probs(q, k, b, lq, lk, h, d, q_prescaled=True)
    assert out.shape == (b, lq, lk) and out.dtype == torch.float32
    AR.check(out, ref, e, "head-major k", torch.float32)
    ref, e = AR.reference(qv, kv, None, prescaled=True, per_head=True)
    out = ops.attention_probs(q, k, b, lq, lk, h, d, q_prescaled=True, per_head=True)
    assert out.shape == (b, h, lq, lk)
    AR.check(out, ref, e, "head-major k, per head", torch.float32)


# ---- the key count in device memory ---------------------------------------------------------------------------------------

LK_DEV = [(110, 83), (128, 1), (238, 205)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("cap,n", LK_DEV)
@pytest.mark.parametrize("hm", [False, True], ids=["rows", "hm"])
@pytest.mark.parametrize("per_head", [False, True], ids=["mean", "heads"])
def test_device_key_count(gpu, dtype, cap, n, hm, per_head):
    """lk_dev below the capacity: elements within the bound over the n real keys, columns n .. cap-1 exactly zero after a
    store, the frame intact — and the bits of an exact-length launch on the same keys.  Keys n .. cap-1 are NaN: not read."""
    heads, d, lq, b = (2, 80, 28, 2) if cap == 128 else (8, 40, 35, 2)
    c = Case(dtype, cap, heads, d, lq, "spike", hm, per_head, cap != 238)
    q4, k4 = make_qk("spike", b, heads, lq, cap, n, d, dtype, hm, 300 + cap, gpu)
    k4[:, :, n:] = float("nan")
    q, qv = (lay_hm if hm else lay_rows)(q4, gpu)
    k, kv = lay_rows(k4, gpu)
    ref, e = AR.reference(qv, kv, d ** -0.5, n_keys=n, prescaled=hm, per_head=per_head)
    lk_dev = torch.tensor([n], dtype=torch.int32, device=gpu)
    frame, out = framed_out(b, heads if per_head else None, lq, cap, c.vec, gpu)
    launch(c, q, k, b, cap, out, lk_dev=lk_dev)
    AR.check(out[..., :n], ref, e, "lk_dev %d of %d" % (n, cap), torch.float32)
    assert bool((out[..., n:] == 0).all()) and not bool(torch.signbit(out[..., n:]).any())
    assert frame_intact(frame, out)
    kx, _ = lay_rows(k4[:, :, :n].contiguous(), gpu)                       # the same keys at their exact length
    exact = launch(c, q, kx, b, n, None)
    assert torch.equal(out[..., :n], exact)


# ---- accumulate -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("per_head", [False, True], ids=["mean", "heads"])
@pytest.mark.parametrize("vec", [False, True], ids=["scalar", "vec"])
def test_accumulate_two_calls(gpu, dtype, per_head, vec):
    """Two accumulating calls with weight 0.5 on different q into a zeroed output = the fp64 sum of the two halves; with a
    device key count the columns past it keep what they held (a sentinel), and the frame stays intact."""
    heads, d, lq, b, cap, n = 8, 80, 35, 2, 110, 83
    hm = not per_head
    c = Case(dtype, cap, heads, d, lq, "peaked", hm, per_head, vec)
    lk_dev = torch.tensor([n], dtype=torch.int32, device=gpu)
    frame, out = framed_out(b, heads if per_head else None, lq, cap, vec, gpu, fill=7.0)
    out[..., :n] = 0.0
    parts = []
    for call in range(2):
        q4, k4 = make_qk("peaked", b, heads, lq, cap, n, d, dtype, hm, 500 + 10 * call, gpu)
        k4[:, :, n:] = float("nan")
        q, qv = (lay_hm if hm else lay_rows)(q4, gpu)
        k, kv = lay_rows(k4, gpu)
        parts.append(AR.reference(qv, kv, d ** -0.5, n_keys=n, prescaled=hm, per_head=per_head, weight=0.5))
        launch(c, q, k, b, cap, out, accumulate=True, weight=0.5, lk_dev=lk_dev)
    ref, e = AR.accumulated(parts)
    AR.check(out[..., :n], ref, e, "accumulate x2", torch.float32)
    assert bool((out[..., n:] == 7.0).all())             # not touched
    assert frame_intact(frame, out, fill=7.0)
    # and on top of what a STORE left there (old != 0), against reference(old=...)
    q4, k4 = make_qk("randn", b, heads, lq, cap, cap, d, dtype, hm, 600, gpu)
    q, qv = (lay_hm if hm else lay_rows)(q4, gpu)
    k, kv = lay_rows(k4, gpu)
    old = out.clone()
    ref, e = AR.reference(qv, kv, d ** -0.5, prescaled=hm, per_head=per_head, weight=0.25, old=old)
    launch(c, q, k, b, cap, out, accumulate=True, weight=0.25)
    AR.check(out, ref, e, "accumulate on old", torch.float32)
    assert frame_intact(frame, out, fill=7.0)
