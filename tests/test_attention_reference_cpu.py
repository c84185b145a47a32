"""Self-test of the fp64 reference / error bound in attention_reference.py (CPU only).

`emulate` is the kernel's loop in torch: 32-key chunks of fp32 scores, the lazy rescale at 5 log2 units triggered per
16-row block, P rounded to the storage type, zero rows for the padded keys of the ragged last chunk, and both
denominators (d = 40: the ones column of V, summed from the ROUNDED P; d = 80 / 160: l_run, summed from the unrounded p),
in the plain and in the prescaled-q form.  The bound must pass it — also with the chunks visited in another order — and a
correctly rounded fp64 result, and must fail every fault below, injected one at a time."""
import pytest
import torch

from tests import attention_reference as A

DTYPES = [torch.float16, torch.bfloat16]
B, H, LQ = 3, 2, 80


def _any16(cond):
    return cond.view(-1, 16).any(dim=1).repeat_interleave(16)


def emulate(q, k, v, c, dtype, *, pre, ones, n=None, order=None, skip=None, pads_in_denominator=False,
            pads_own_max=False):
    """One plane: q (lq, d), k / v (>= n, d) storage type -> the fp32 normalised output (lq, d) before its rounding.
    skip = (chunk, first row): that chunk is left out for the 16 rows from `first row`."""
    lq, d = q.shape
    n = k.shape[0] if n is None else n
    nch = (n + 31) // 32
    kp = torch.zeros((nch * 32, d), dtype=torch.float32)
    vp = torch.zeros((nch * 32, d + 1), dtype=torch.float32)
    kp[:n], vp[:n, :d], vp[:n, d] = k[:n].float(), v[:n].float(), 1.0
    if pads_in_denominator:
        vp[n:, d] = 1.0
    s_all = q.float() @ kp.t()
    cf = torch.tensor(c, dtype=torch.float32)
    m = torch.zeros(lq) if pre else torch.full((lq,), -1e30)
    l = torch.zeros(lq)
    acc = torch.zeros((lq, d + 1))
    for idx, ch in enumerate(order or range(nch)):
        keep = (m.clone(), l.clone(), acc.clone())
        s = s_all[:, ch * 32:ch * 32 + 32].clone()
        pad = torch.arange(ch * 32, ch * 32 + 32) >= n
        tail = bool(pad.any())
        if not ones and tail:
            s[:, pad] = -float("inf")
        if pre:
            s = s - m[:, None]
            first = idx == 0
            trig = torch.ones(lq, dtype=torch.bool) if first else _any16(s.amax(dim=1) > A.THR)
            sm = s.clone()
            if ones and tail and not pads_own_max:
                sm[:, pad] = -float("inf")
            mx = sm.amax(dim=1)
            if not first:
                mx = mx.clamp(min=0.0)
            mx = torch.where(trig, mx.clamp(min=-1e30), torch.zeros(lq))
            alpha = torch.ones(lq) if first else torch.exp2(-mx)
            s = torch.where(trig[:, None], sm, s) - mx[:, None]
            m = m + mx
        else:
            trig = _any16(s.amax(dim=1) * cf - m > A.THR)
            sm = s.clone()
            if ones and tail and not pads_own_max:
                sm[:, pad] = -float("inf")
            m_new = torch.where(trig, torch.maximum(m, sm.amax(dim=1) * cf), m)
            alpha = torch.exp2(m - m_new)
            m = m_new
            s = torch.where(trig[:, None], sm, s) * cf - m[:, None]
        pe = torch.exp2(s)
        l = l * alpha + pe.sum(dim=1)
        acc = acc * alpha[:, None] + pe.to(dtype).float() @ vp[ch * 32:ch * 32 + 32]
        if skip is not None and skip[0] == ch:
            r = slice(skip[1], skip[1] + 16)
            m[r], l[r], acc[r] = keep[0][r], keep[1][r], keep[2][r]
    den = acc[:, d] if ones else l
    return acc[:, :d] / den[:, None]


def _data(dtype, d, lk, kind, pre):
    """q4 [B, H, LQ, d], k4 / v4 [B, H, lk, d], c.  The stored q is the prescaled one when pre."""
    scale = d ** -0.5
    qs = scale * A.LOG2E if pre else 1.0
    q = A.rand((B, H, LQ, d), torch.float32, 1, device="cpu")
    k = A.rand((B, H, lk, d), torch.float32, 2, device="cpu")
    v = A.rand((B, H, lk, d), torch.float32, 3, device="cpu")
    if kind == "negative":                                  # every real score far below zero (and below -126 log2 units)
        q, k = q.abs() + 1.5, -(k.abs() + 1.0) * (4.0 if d == 40 else 2.0)
    elif kind == "offset":
        v = v * 0.25 + 3.0
    elif kind == "boundary":                                # the keys on either side of a chunk boundary carry weight
        for j in (63, 64):
            if j < lk:
                k[:, :, j] = q[:, :, j % LQ] * 1.5
    elif kind == "spike":
        k[:, :, lk - 1] = q[:, :, 7] * 4.0
        k[:, :, lk // 2] = q[:, :, 9] * 3.0
    return (q * qs).to(dtype), k.to(dtype), v.to(dtype), (1.0 if pre else scale * A.LOG2E), scale


def _emulate_all(q4, k4, v4, c, dtype, pre, kmap=None, **kw):
    """-> fp32 [B, H, LQ, d]"""
    d = q4.shape[3]
    out = torch.empty(q4.shape, dtype=torch.float32)
    for b in range(B):
        kb = b if kmap is None else kmap[b]
        for h in range(H):
            out[b, h] = emulate(q4[b, h], k4[kb, h], v4[kb, h], c, dtype, pre=pre, ones=d % 16 != 0, **kw)
    return out


def _ref(q4, k4, v4, scale, pre, **kw):
    ref, e = A.reference(q4, k4, v4, A.LN2 if pre else scale, prescaled=pre, **kw)
    return ref.view(B, H, LQ, -1), e.view(B, H, LQ, -1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [40, 80, 160])
@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("kind", ["plain", "negative", "offset", "spike", "boundary"])
@pytest.mark.parametrize("lk", [1, 33, 70, 300])
def test_bound_passes_correct_results(dtype, d, pre, kind, lk):
    q4, k4, v4, c, scale = _data(dtype, d, lk, kind, pre)
    ref, e = _ref(q4, k4, v4, scale, pre)
    A.check(ref.to(dtype), ref, e, "correctly rounded")
    y = _emulate_all(q4, k4, v4, c, dtype, pre)
    A.check(y.to(dtype), ref, e, "emulation")
    nch = (lk + 31) // 32
    if nch > 1:
        g = torch.Generator().manual_seed(5)
        order = torch.randperm(nch, generator=g).tolist()
        y = _emulate_all(q4, k4, v4, c, dtype, pre, order=order)
        A.check(y.to(dtype), ref, e, "emulation, chunk order %s" % order)


def test_bound_is_not_vacuous():
    """On offset V at d = 40 (the centred form) the emulation's own rounding reaches a good part of the bound."""
    for dtype in DTYPES:
        q4, k4, v4, c, scale = _data(dtype, 40, 300, "offset", False)
        ref, e = _ref(q4, k4, v4, scale, False)
        r = A.check(_emulate_all(q4, k4, v4, c, dtype, False).to(dtype), ref, e, "emulation")
        assert r > 0.05, "max err / bound = %.3g" % r


def _fails(y, ref, e, what):
    with pytest.raises(AssertionError, match="outside the bound"):
        A.check(y, ref, e, what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [40, 80])
@pytest.mark.parametrize("pre", [False, True])
def test_bound_catches_each_loop_fault(dtype, d, pre):
    """Faults inside the key loop.  All of them are far above bf16 rounding on these inputs, so both types run."""
    ones = d % 16 != 0
    # one 32-key chunk skipped for one 16-row block
    q4, k4, v4, c, scale = _data(dtype, d, 300, "plain", pre)
    ref, e = _ref(q4, k4, v4, scale, pre)
    A.check(_emulate_all(q4, k4, v4, c, dtype, pre).to(dtype), ref, e, "correct")
    _fails(_emulate_all(q4, k4, v4, c, dtype, pre, skip=(4, 16)).to(dtype), ref, e, "chunk skipped")
    # a key count off by one in either direction at a chunk boundary (the buffer holds 70 rows, 64 are real)
    q4, k4, v4, c, scale = _data(dtype, d, 70, "boundary", pre)
    ref, e = _ref(q4, k4, v4, scale, pre, n_keys=64)
    A.check(_emulate_all(q4, k4, v4, c, dtype, pre, n=64).to(dtype), ref, e, "correct, 64 of 70 keys")
    _fails(_emulate_all(q4, k4, v4, c, dtype, pre, n=63).to(dtype), ref, e, "one key short")
    _fails(_emulate_all(q4, k4, v4, c, dtype, pre, n=65).to(dtype), ref, e, "one key too many")
    if ones:
        # the ragged tail's padded keys left in the denominator (ones column not zeroed / not restored between passes)
        q4, k4, v4, c, scale = _data(dtype, d, 70, "plain", pre)
        ref, e = _ref(q4, k4, v4, scale, pre)
        A.check(_emulate_all(q4, k4, v4, c, dtype, pre).to(dtype), ref, e, "correct")
        _fails(_emulate_all(q4, k4, v4, c, dtype, pre, pads_in_denominator=True).to(dtype), ref, e, "pads in denominator")
        # padded keys allowed to own the running max on all-negative rows: every real probability underflows
        q4, k4, v4, c, scale = _data(dtype, d, 70, "negative", pre)
        ref, e = _ref(q4, k4, v4, scale, pre)
        A.check(_emulate_all(q4, k4, v4, c, dtype, pre).to(dtype), ref, e, "correct")
        _fails(_emulate_all(q4, k4, v4, c, dtype, pre, pads_own_max=True).to(dtype), ref, e, "pads own the max")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [40, 80])
def test_bound_catches_each_pair_and_store_fault(dtype, d):
    """Faults around the loop: the neighbour pair, accumulate, the output store.  Both types: each moves whole rows."""
    pre = False
    q4, k4, v4, c, scale = _data(dtype, d, 70, "plain", pre)
    left, right = [2, 0, 1], [1, 2, 0]
    lt, rt = torch.tensor(left, dtype=torch.int32), torch.tensor(right, dtype=torch.int32)
    o1 = _emulate_all(q4, k4, v4, c, dtype, pre, kmap=left)
    o2 = _emulate_all(q4, k4, v4, c, dtype, pre, kmap=right)
    ref, e = _ref(q4, k4, v4, scale, pre, kv_map=lt, kv_map2=rt)
    A.check((o1 + o2).to(dtype), ref, e, "pair")
    _fails((o1 + o1).to(dtype), ref, e, "second neighbour from the first map")
    wrong = o1.clone()
    wrong[:, :, 16:32], wrong[:, :, 32:48] = o1[:, :, 32:48], o1[:, :, 16:32]
    _fails((wrong + o2).to(dtype), ref, e, "stash added to the wrong row block")
    # accumulate
    old = A.rand((B, H, LQ, d), dtype, 9, device="cpu")
    refa, ea = _ref(q4, k4, v4, scale, pre, kv_map=lt, old4=old)
    A.check((o1 + old.float()).to(dtype), refa, ea, "accumulate")
    _fails(o1.to(dtype), refa, ea, "accumulate overwrites")
    # stores
    ref1, e1 = _ref(q4, k4, v4, scale, pre, kv_map=lt)
    y = o1.to(dtype)
    A.check(y, ref1, e1, "single")
    bad = y.clone()
    bad[:, :, 64:] = float("nan")
    _fails(bad, ref1, e1, "last partial query block unwritten")
    bad = y.clone()
    bad[:, 0], bad[:, 1] = y[:, 1], y[:, 0]
    _fails(bad, ref1, e1, "one head stored in its neighbour's columns")


def test_mis_scaled_chunk_is_seen_in_fp16_only():
    """What the bound cannot see (module docstring): a 2 % error of one chunk's probabilities is below bf16's rounding of
    P.  Stated here so that nobody reads the bf16 leg as covering it."""
    d, lk = 40, 300
    for dtype, seen in ((torch.float16, True), (torch.bfloat16, False)):
        q4, k4, v4, c, scale = _data(dtype, d, lk, "plain", False)
        ref, e = _ref(q4, k4, v4, scale, False)
        y = torch.empty(q4.shape, dtype=torch.float32)
        for b in range(B):
            for h in range(H):
                w = torch.softmax((q4[b, h].double() @ k4[b, h].double().t()) * scale, dim=1)
                w[:, 128:160] *= 1.02
                y[b, h] = (w @ v4[b, h].double() / w.sum(dim=1, keepdim=True)).float()
        if seen:
            _fails(y.to(dtype), ref, e, "2 % chunk")
        else:
            A.check(y.to(dtype), ref, e, "2 % chunk, bf16")
