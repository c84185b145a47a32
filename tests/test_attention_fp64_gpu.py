"""Every reachable dd_attn5_kernel instantiation, every operand layout of ops.attention and the device key count
(`lk_dev`, also of dd_xattn320) against the fp64 reference and per-element bound of attention_reference.py.

`attn_plan` (csrc/attention.hip) picks (head_dim, 16-row blocks per wave, key tile) from the shape; each plan exists for
q_prescaled x neighbour pair x fp16 / bf16.  PLANS names one shape per plan (found with dd_attention_kernel_name, which
needs no GPU), `cases()` expands it, and test_case_table_selects_every_instantiation (no GPU) asserts that every case
selects the instantiation it is tagged with and that together they select all 68.  The GPU tests launch them through
ops.attention with NaN-filled outputs and compare every element (sampled planes only where a case has more than 96:
attention_reference.xcd_sample)."""
import collections
import ctypes

import pytest
import torch

from dualdiff_amd import _native
from tests import attention_reference as A

DTYPES = [torch.float16, torch.bfloat16]
_TN = {torch.float16: "_Float16", torch.bfloat16: "__bf16"}

# plan (d, qt, key tile) -> (batch, heads, lq, key counts per data kind).  The 32- / 48-row plans need lq >= 256 and at least
# 512 128-row blocks; d = 40 then takes 48 rows when the 192-row split wastes less of a generation than the 128-row one
# (352 planes x 300 rows: 704 workgroups of 192 rows on 768 slots against 1056 of 128 on 1024), 32 rows when both fill
# the chip alike (256 planes x 500 rows: 1024 on 1024).  128-key tiles need lk >= 512.  lq is never a multiple of the
# 64 / 128 / 192-row workgroup.
SHORT = {"randn": (129, 64, 1), "offset": (127, 32), "spike": (65, 128, 31), "negative": (33, 63)}
LONG = {"randn": (520, 640), "offset": (577,), "spike": (513,), "negative": (545,)}
PLANS = collections.OrderedDict([
    ((40, 1, 64), (3, 2, 100, SHORT)),
    ((40, 2, 64), (32, 8, 500, SHORT)),
    ((40, 3, 64), (44, 8, 300, SHORT)),
    ((40, 3, 128), (44, 8, 300, LONG)),
    ((80, 1, 64), (3, 2, 100, SHORT)),
    ((80, 2, 64), (22, 8, 300, SHORT)),
    ((80, 2, 128), (22, 8, 300, LONG)),
    ((160, 1, 64), (3, 2, 100, SHORT)),
    ((160, 2, 64), (22, 8, 300, SHORT)),
])
LAYOUT = {"randn": "fused", "offset": "hm", "spike": "bm", "negative": "fused"}
Case = collections.namedtuple("Case", "plan dtype pre pair batch heads lq lk kind layout")


def has_plan(plan, pre):
    return not (plan == (40, 3, 128) and pre)          # the prescaled 48-row kernel spills with 128-key tiles: 64 there


def instantiation(plan, dtype, pre, pair):
    d, qt, tile = plan
    return "dd_attn5_kernel<%s, %d, %d, %d, 1, %d, %s, %s>" % (_TN[dtype], d, qt, tile, 3 if qt == 3 else 1,
                                                              "true" if pre else "false", "true" if pair else "false")


def expected_instantiations():
    """From the plan rules of attn_plan, not from PLANS: an instantiation added later without a case fails the table test."""
    plans = [(40, 1, 64), (40, 2, 64), (40, 3, 64), (40, 3, 128), (80, 1, 64), (80, 2, 64), (80, 2, 128), (160, 1, 64),
             (160, 2, 64)]
    return {instantiation(p, dt, pre, pair) for p in plans for dt in DTYPES for pre in (False, True)
            for pair in (False, True) if has_plan(p, pre)}


def cases(plan=None, dtype=None):
    out = []
    for p, (b, h, lq, lks) in PLANS.items():
        for dt in DTYPES:
            if (plan is not None and p != plan) or (dtype is not None and dt != dtype):
                continue
            for pre in (False, True):
                if not has_plan(p, pre):
                    continue
                for pair in (False, True):
                    for kind in ("randn", "offset", "spike", "negative"):
                        for lk in lks[kind]:
                            out.append(Case(p, dt, pre, pair, b, h, lq, lk, kind, LAYOUT[kind]))
    return out


def kernel_name(lib, batch, heads, lq, lk, d, dtype, pre, pair):
    a = _native.AttnDesc()
    a.q = a.k = a.v = a.o = 4096                        # aligned dummies: the planner dereferences nothing
    c = heads * d
    a.ldq = a.ldo = a.ldk = a.ldv = c
    a.q_batch_stride = a.o_batch_stride = lq * c
    a.k_batch_stride = a.v_batch_stride = lk * c
    a.batch, a.heads, a.head_dim, a.lq, a.lk = batch, heads, d, lq, lk
    a.scale, a.dtype, a.q_prescaled = d ** -0.5, _native.DD_F16 if dtype == torch.float16 else _native.DD_BF16, int(pre)
    if pair:
        a.kv_batch_map = a.kv_batch_map2 = 4096
    return lib.dd_attention_kernel_name(ctypes.byref(a)).decode().split(" grid=")[0]


def test_case_table_selects_every_instantiation():
    lib = _native.load()
    want = expected_instantiations()
    assert len(want) == 68
    seen = set()
    for c in cases():
        name = kernel_name(lib, c.batch, c.heads, c.lq, c.lk, c.plan[0], c.dtype, c.pre, c.pair)
        assert name == instantiation(c.plan, c.dtype, c.pre, c.pair), (c, name)
        seen.add(name)
    for plan, dtype, pre, pair, b, h, lq, cap, counts in lk_dev_cases():
        name = kernel_name(lib, b, h, lq, cap, plan[0], dtype, pre, pair)
        assert name == instantiation(plan, dtype, pre, pair), (plan, cap, name)
        if plan[2] == 128:                              # counts below 512 take the 64-key tile as an exact-length launch
            other = kernel_name(lib, b, h, lq, counts[0], plan[0], dtype, pre, pair)
            assert other == instantiation((plan[0], plan[1], 64), dtype, pre, pair), other
    assert seen == want, (sorted(want - seen), sorted(seen - want))


def test_xcd_sample_keeps_what_it_must():
    for b, h, lq, rows in ((44, 8, 300, 192), (32, 8, 500, 128), (22, 8, 300, 128), (13, 8, 77, 64)):
        s = A.xcd_sample(b, h, lq, rows)
        n = b * h
        assert s[0] == 0 and s[-1] == n - 1 and 2 * len(s) >= n and len(set(s)) == len(s)
        nqb = -(-lq // rows)
        nwg = nqb * n
        item = lambda blk: ((blk & 7) * (nwg // 8 + 1) if (blk & 7) < nwg % 8 else
                            (nwg % 8) * (nwg // 8 + 1) + ((blk & 7) - nwg % 8) * (nwg // 8)) + (blk >> 3)
        assert sorted(item(i) for i in range(nwg)) == list(range(nwg))      # the mapping the sample is built on
        for xcd in range(1, 8):                          # first item of every XCD's range and the one before it
            first = item(xcd)
            assert first // nqb in s and (first - 1) // nqb in s


# ---- data and layouts --------------------------------------------------------------------------------------------------

def _randn(shape, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(shape, generator=g, device=dev, dtype=torch.float32)


def make_data(kind, b, bk, h, lq, lk, d, dtype, pre, seed, dev):
    """Canonical fp32-valued, storage-typed q [b, h, lq, d], k / v [bk, h, lk, d]; q as STORED (prescaled when pre)."""
    q, k, v = _randn((b, h, lq, d), seed, dev), _randn((bk, h, lk, d), seed + 1, dev), _randn((bk, h, lk, d), seed + 2, dev)
    if kind == "offset":
        v = v * 0.25 + 3.0
    elif kind == "spike":                               # one late in the sequence, one on the last key (the ragged chunk)
        n = min(b, bk)
        k[:n, :, lk - 1] = q[:n, :, 7 % lq] * 4.0
        k[:n, :, (3 * lk) // 4] = q[:n, :, 9 % lq] * 3.0
    elif kind == "negative":                            # every real score near -110 log2 units: padded keys (0) top them
        q = q.abs() + 1.5
        k = -(k.abs() + 1.0) * 3.0 * (40.0 / d) ** 0.5
    if pre:
        q = q * (d ** -0.5 * A.LOG2E)
    return q.to(dtype), k.to(dtype), v.to(dtype)


def lay_out(t4, layout, dev):
    """Canonical [b, h, l, d] -> (operand for ops.attention, canonical VIEW of that operand's memory)."""
    b, h, l, d = t4.shape
    c = h * d
    if layout == "fused":                               # the middle third of a [rows, 3C] buffer, NaN on both sides
        buf = A.nan_like((b * l, 3 * c), t4.dtype, dev)
        op = buf[:, c:2 * c]
        A.rows_view(op, b, l, h, d).copy_(t4)
        return op, A.rows_view(op, b, l, h, d)
    if layout == "hm":
        op = t4.permute(1, 0, 2, 3).reshape(h, b * l, d).contiguous()
        return op, A.head_major_view(op, b, l, h, d)
    if layout == "bm":                                  # the K heads of a (batches, [K heads | V heads], l, d) buffer
        buf = A.nan_like((b, 2 * h, l, d), t4.dtype, dev)
        buf[:, h:] = t4
        return buf[:, h:], buf[:, h:]
    raise ValueError(layout)


def new_out(b, lq, h, d, dtype, dev, fill=float("nan")):
    buf = torch.full((b * lq, h * d + 64), fill, dtype=dtype, device=dev)
    return buf, buf[:, :h * d]


def compare(y4, q4, k4, v4, scale, rows_per_wg, stats, what, **kw):
    """fp64 check of an output [B, H, lq, d]: all planes, or xcd_sample's when there are more than 96 (then every plane
    is still checked for NaN)."""
    b, h, lq, d = y4.shape
    planes = None
    if b * h > 96:
        planes = A.xcd_sample(b, h, lq, rows_per_wg)
        assert 2 * len(planes) >= b * h
        assert not bool(torch.isnan(y4).any()), what + ": NaN in the output"
    ref, e = A.reference(q4, k4, v4, scale, planes=planes, **kw)
    y = A.take_planes(y4, planes)
    stats[0].append(A.check(y, ref, e, what))
    stats[1].append(A.mean_ratio(y, ref, e))


def ring_maps(b, dev, permutation):
    left = [(i - 1) % b for i in range(b)]
    right = [(i + 1) % b for i in range(b)]
    if not permutation:                                 # several batches read the same neighbour
        left = [min(i, b - 1 - i) for i in range(b)]
        right = [0 if i % 2 else b - 1 for i in range(b)]
    return (torch.tensor(left, dtype=torch.int32, device=dev), torch.tensor(right, dtype=torch.int32, device=dev))


@pytest.fixture(scope="module")
def ops(gpu):
    from dualdiff_amd import ops as O
    return O


# ---- every instantiation -------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("plan", list(PLANS), ids=lambda p: "d%d_qt%d_kv%d" % p)
def test_every_instantiation_matches_fp64(ops, gpu, plan, dtype):
    d, qt, _tile = plan
    scale = d ** -0.5
    stats = ([], [])
    for i, c in enumerate(cases(plan, dtype)):
        what = "%s %s pre=%d pair=%d lk=%d %s" % (instantiation(plan, dtype, c.pre, c.pair), c.kind, c.pre, c.pair, c.lk,
                                                   c.layout)
        q4, k4, v4 = make_data(c.kind, c.batch, c.batch, c.heads, c.lq, c.lk, d, dtype, c.pre, 100 + 8 * i, gpu)
        q_op, qv = lay_out(q4, "fused" if c.layout == "bm" else c.layout, gpu)
        k_op, kv = lay_out(k4, c.layout, gpu)
        v_op, vv = lay_out(v4, c.layout, gpu)
        obuf, out = new_out(c.batch, c.lq, c.heads, d, dtype, gpu)
        y4 = A.rows_view(out, c.batch, c.lq, c.heads, d)
        m1, m2 = ring_maps(c.batch, gpu, permutation=c.kind != "offset")
        kw = dict(kv_batch_map=m1, kv_batch_map2=m2) if c.pair else \
            (dict(kv_batch_map=m1) if c.kind in ("offset", "spike") else {})
        ops.attention(q_op, k_op, v_op, c.batch, c.lq, c.lk, c.heads, d, scale, out=out, q_prescaled=c.pre, **kw)
        rkw = dict(kv_map=kw.get("kv_batch_map"), kv_map2=kw.get("kv_batch_map2"), prescaled=c.pre)
        sc = A.LN2 if c.pre else scale
        compare(y4, qv, kv, vv, sc, 64 * qt, stats, what, **rkw)
        assert bool(torch.isnan(obuf[:, c.heads * d:]).all()), what + ": wrote past the output's columns"
        if c.pair and c.kind == "randn":                # a third neighbour by accumulate onto the pair's result
            old = out.clone()
            m3 = torch.flip(m1, dims=[0]).contiguous()
            ops.attention(q_op, k_op, v_op, c.batch, c.lq, c.lk, c.heads, d, scale, out=out, q_prescaled=c.pre,
                          kv_batch_map=m3, accumulate=True)
            compare(y4, qv, kv, vv, sc, 64 * qt, stats, what + " + accumulate", kv_map=m3, prescaled=c.pre,
                    old4=A.rows_view(old, c.batch, c.lq, c.heads, d))
    torch.cuda.synchronize()
    print("\n[attention fp64] " + A.report_line("d%d qt%d kv%d %s" % (plan + (_TN[dtype],)), *stats))


# ---- sequence strides (temporal attention), the chunk walk ----------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("d", [40, 80, 160])
def test_sequence_strides_match_fp64(ops, gpu, d, dtype):
    """Temporal attention as video_blocks passes it: the sequence runs over the T frames of every token of a fused
    (T * tokens, 3C) projection — seq_strides = (tokens * 3C, 3C), out_seq_strides = (tokens * C, C) — and, frame-split,
    against keys gathered into a (T_all, tokens, 2C) buffer: kv_seq_strides = (tokens * 2C, 2C)."""
    h, t_n, tokens = 8, 6, 150
    c = h * d
    scale = d ** -0.5
    stats = ([], [])
    qkv = (_randn((t_n * tokens, 3 * c), 7, gpu)).to(dtype)
    obuf = A.nan_like((t_n * tokens, c), dtype, gpu)
    ops.attention(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], tokens, t_n, t_n, h, d, scale, out=obuf,
                  seq_strides=(tokens * 3 * c, 3 * c), out_seq_strides=(tokens * c, c))
    view = lambda t, l, w, col: A.seq_view(t[:, col:], tokens, l, h, d, tokens * w, w)
    compare(view(obuf, t_n, c, 0), view(qkv, t_n, 3 * c, 0), view(qkv, t_n, 3 * c, c), view(qkv, t_n, 3 * c, 2 * c), scale,
            64, stats, "seq_strides d=%d" % d)
    t_all = 9                                           # gathered keys of more frames than the local queries
    kv_all = (_randn((t_all * tokens, 2 * c), 8, gpu) * 0.5 + 0.25).to(dtype)
    obuf = A.nan_like((t_n * tokens, c), dtype, gpu)
    ops.attention(qkv[:, :c], kv_all[:, :c], kv_all[:, c:], tokens, t_n, t_all, h, d, scale, out=obuf,
                  seq_strides=(tokens * 3 * c, 3 * c), out_seq_strides=(tokens * c, c),
                  kv_seq_strides=(tokens * 2 * c, 2 * c))
    compare(view(obuf, t_n, c, 0), view(qkv, t_n, 3 * c, 0), view(kv_all, t_all, 2 * c, 0), view(kv_all, t_all, 2 * c, c),
            scale, 64, stats, "kv_seq_strides d=%d" % d)
    print("\n[attention fp64] " + A.report_line("seq strides d%d %s" % (d, _TN[dtype]), *stats))


@pytest.mark.gpu
def test_sequence_strides_chunk_walk_matches_fp64(ops, gpu):
    """batch * heads = 8200 * 8 > 65535: ops.attention walks the batch in chunks of 8191 entries.  Tiny sequences."""
    dtype, h, d, t_n, tokens = torch.float16, 8, 40, 4, 8200
    c = h * d
    qkv = (_randn((t_n * tokens, 3 * c), 9, gpu)).to(dtype)
    obuf = A.nan_like((t_n * tokens, c), dtype, gpu)
    ops.attention(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], tokens, t_n, t_n, h, d, d ** -0.5, out=obuf,
                  seq_strides=(tokens * 3 * c, 3 * c), out_seq_strides=(tokens * c, c))
    assert not bool(torch.isnan(obuf).any())
    view = lambda t, w, col: A.seq_view(t[:, col:], tokens, t_n, h, d, tokens * w, w)
    # every plane on either side of the chunk boundaries (batch 8190 | 8191) and a stride-7 sample: far more than half is
    # not needed for 4 x 4 score matrices, but ALL are cheap
    ref, e = A.reference(view(qkv, 3 * c, 0), view(qkv, 3 * c, c), view(qkv, 3 * c, 2 * c), d ** -0.5)
    r = A.check(A.take_planes(view(obuf, c, 0)), ref, e, "seq_strides chunk walk")
    print("\n[attention fp64] chunk walk 65600 planes   max err/bound %.3f" % r)


# ---- lk_dev: the key count read from device memory ------------------------------------------------------------------------

def lk_dev_cases():
    """(plan, dtype, pre, pair, batch, heads, lq, capacity, counts).  Capacity >= 512 selects the 128-key tile while the
    exact-length launches at counts < 512 take the 64-key one."""
    out = []
    for p, (b, h, lq, lks) in PLANS.items():
        cap = 520 if lks is LONG else 100
        counts = (1, 31, 32, 33, 63, 64, 65, cap - 1, cap)
        for dt in DTYPES:
            for pre in (False, True):
                if has_plan(p, pre):
                    for pair in (False, True):
                        out.append((p, dt, pre, pair, b, h, lq, cap, counts))
    return out


def capacity_kv(k4, v4, n, dev):
    """K / V rows at capacity strides, rows n.. NaN: 4-D batch-major operands (capacity) and their [:n] slices (the same
    strides with lk = n)."""
    kc, vc = k4.clone(), v4.clone()
    kc[:, :, n:] = float("nan")
    vc[:, :, n:] = float("nan")
    return kc, vc


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("plan", list(PLANS), ids=lambda p: "d%d_qt%d_kv%d" % p)
def test_lk_dev_matches_fp64_and_the_exact_length_launch(ops, gpu, plan, dtype):
    d, qt, _tile = plan
    scale = d ** -0.5
    stats = ([], [])
    cnt = torch.zeros(1, dtype=torch.int32, device=gpu)
    for (p, dt, pre, pair, b, h, lq, cap, counts) in lk_dev_cases():
        if p != plan or dt != dtype:
            continue
        q4, k4, v4 = make_data("spike" if pre else "offset", b, b, h, lq, cap, d, dtype, pre, 500 + pre + 2 * pair, gpu)
        q_op, qv = lay_out(q4, "fused", gpu)
        m1, m2 = ring_maps(b, gpu, permutation=True)
        kw = dict(kv_batch_map=m1, kv_batch_map2=m2) if pair else {}
        sc = A.LN2 if pre else scale
        for n in counts:
            what = "%s lk_dev=%d of %d" % (instantiation(plan, dtype, pre, pair), n, cap)
            kc, vc = capacity_kv(k4, v4, n, gpu)
            cnt.fill_(n)
            _, out = new_out(b, lq, h, d, dtype, gpu)
            ops.attention(q_op, kc, vc, b, lq, cap, h, d, scale, out=out, q_prescaled=pre, lk_dev=cnt, **kw)
            _, exact = new_out(b, lq, h, d, dtype, gpu)
            ops.attention(q_op, kc[:, :, :n], vc[:, :, :n], b, lq, n, h, d, scale, out=exact, q_prescaled=pre, **kw)
            compare(A.rows_view(out, b, lq, h, d), qv, kc, vc, sc, 64 * qt, stats, what, n_keys=n,
                    kv_map=kw.get("kv_batch_map"), kv_map2=kw.get("kv_batch_map2"), prescaled=pre)
            assert torch.equal(out, exact), what + ": differs from the launch with lk = %d on the same strides" % n
    print("\n[attention fp64] " + A.report_line("lk_dev d%d qt%d kv%d %s" % (plan + (_TN[dtype],)), *stats))


@pytest.mark.gpu
@pytest.mark.parametrize("d", [40, 80, 160])
def test_lk_dev_through_sequence_strides_and_the_clamp(ops, gpu, d):
    """The capacity layout through seq_strides / kv_seq_strides (2-D operands), and the documented clamp to [1, lk]: a
    count of 0 behaves as 1, a count above the capacity as the capacity (all rows valid there)."""
    dtype, b, h, lq, cap = torch.float16, 5, 4, 70, 96
    c = h * d
    scale = d ** -0.5
    q4, k4, v4 = make_data("randn", b, b, h, lq, cap, d, dtype, False, 900, gpu)
    q_op, qv = lay_out(q4, "fused", gpu)                 # row pitch 3C
    stats = ([], [])
    cnt = torch.zeros(1, dtype=torch.int32, device=gpu)

    def launch(k_op, v_op, lk, lk_dev):
        _, out = new_out(b, lq, h, d, dtype, gpu)
        ops.attention(q_op, k_op, v_op, b, lq, lk, h, d, scale, out=out, lk_dev=lk_dev,
                      seq_strides=(3 * c, lq * 3 * c), out_seq_strides=(c + 64, lq * (c + 64)),
                      kv_seq_strides=(3 * c, cap * 3 * c))
        return out

    for n, eff in ((0, 1), (1, 1), (33, 33), (95, 95), (96, 96), (97, 96), (1 << 30, 96), (-5, 1)):
        kc, vc = (k4, v4) if eff == cap else capacity_kv(k4, v4, eff, gpu)
        k_op, kv = lay_out(kc, "fused", gpu)
        v_op, vv = lay_out(vc, "fused", gpu)
        cnt.fill_(n)
        out = launch(k_op, v_op, cap, cnt)
        exact = launch(k_op, v_op, eff, None)
        compare(A.rows_view(out, b, lq, h, d), qv, kv, vv, scale, 64, stats, "d=%d lk_dev=%d -> %d" % (d, n, eff), n_keys=eff)
        assert torch.equal(out, exact), "count %d does not behave as %d" % (n, eff)
    print("\n[attention fp64] " + A.report_line("lk_dev clamp / seq d%d" % d, *stats))


@pytest.mark.gpu
def test_lk_dev_changes_between_replays_of_one_graph(ops, gpu):
    """One captured launch, the count rewritten between replays: each replay equals the eager launch for that count."""
    dtype, d = torch.bfloat16, 80
    b, h, lq, cap = PLANS[(80, 2, 128)][0], PLANS[(80, 2, 128)][1], PLANS[(80, 2, 128)][2], 520
    scale = d ** -0.5
    q4, k4, v4 = make_data("randn", b, b, h, lq, cap, d, dtype, False, 950, gpu)
    q_op, _ = lay_out(q4, "fused", gpu)
    cnt = torch.full((1,), cap, dtype=torch.int32, device=gpu)
    _, out = new_out(b, lq, h, d, dtype, gpu)
    ops.attention(q_op, k4, v4, b, lq, cap, h, d, scale, out=out, lk_dev=cnt)      # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.attention(q_op, k4, v4, b, lq, cap, h, d, scale, out=out, lk_dev=cnt)
    for n in (33, 520, 64, 511, 1):
        cnt.fill_(n)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _, eager = new_out(b, lq, h, d, dtype, gpu)
        ops.attention(q_op, k4[:, :, :n], v4[:, :, :n], b, lq, n, h, d, scale, out=eager)
        assert torch.equal(out, eager), "replay with %d keys differs from the eager launch" % n


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("head_major", [False, True], ids=["rows", "planes"])
@pytest.mark.parametrize("ln", [False, True], ids=["plain", "ln_out"])
def test_xattn320_lk_dev_equals_the_exact_length_launch(ops, gpu, dtype, head_major, ln):
    """dd_xattn320 at a capacity layout with NaN rows past the count: inside the fp64 bound at the count
    (attention_reference.xattn_reference) and bit-identical to the exact-length launches on the same strides (one per
    instance: the wrapper derives the instance stride from lk, the row and head strides are the capacity layout's)."""
    inst, n_rows, c, h, d = 3, 100, 320, 8, 40
    x = A.rand((inst * n_rows, c), dtype, 1)
    res = A.rand((inst * n_rows, c), dtype, 2)
    wq_raw, wo_raw = A.rand((c, c), dtype, 3, c ** -0.5), A.rand((c, c), dtype, 4, c ** -0.5)
    wq, wo = ops.xattn_pack_weight(wq_raw), ops.xattn_pack_weight(wo_raw)
    ratios, means = [], []
    bo = A.rand((c,), dtype, 5)
    g_, b_ = (1.0 + 0.1 * A.rand((c,), torch.float32, 8)).to(dtype), A.rand((c,), dtype, 9, 0.1)
    lno = (g_, b_, 1e-5) if ln else None
    cnt = torch.zeros(1, dtype=torch.int32, device=gpu)
    for cap in (128, 98):
        bank = A.rand((inst * cap, 1920), dtype, 6)
        for n in (1, 31, 32, 33, 63, 64, 65, cap - 1, cap, 0, cap + 7):
            eff = min(max(n, 1), cap)
            kv = bank.clone()
            kv.view(inst, cap, 1920)[:, eff:] = float("nan")
            k, v = kv[:, 640:960], kv[:, 960:1280]
            if head_major:
                k = k.reshape(inst * cap, h, d).permute(1, 0, 2).contiguous()
                v = v.reshape(inst * cap, h, d).permute(1, 0, 2).contiguous()
            cnt.fill_(n)
            y = ops.xattn320(x, wq, wo, bo, k, v, inst, n_rows, cap, d ** -0.5, res=res, ln_out=lno, lk_dev=cnt)
            k4 = A.rows_view(kv[:, 640:960], inst, cap, h, d)
            v4 = A.rows_view(kv[:, 960:1280], inst, cap, h, d)
            ref, e = A.xattn_reference(x, wq_raw, wo_raw, bo, k4, v4, d ** -0.5, res=res, n_keys=eff)
            ratios.append(A.check(y, ref, e, "xattn320 capacity %d count %d" % (cap, n)))
            means.append(A.mean_ratio(y, ref, e))
            for i in range(inst):
                rows = slice(i * n_rows, (i + 1) * n_rows)
                keys = slice(i * cap, i * cap + eff)
                ki, vi = (k[:, keys], v[:, keys]) if head_major else (k[keys], v[keys])
                yi = ops.xattn320(x[rows], wq, wo, bo, ki, vi, 1, n_rows, eff, d ** -0.5, res=res[rows], ln_out=lno)
                assert torch.equal(y[rows], yi), "capacity %d count %d instance %d" % (cap, n, i)
                if ln:
                    assert torch.equal(y._ln_out[rows], yi._ln_out)
    print("\n[attention fp64] " + A.report_line("xattn320 lk_dev %s %s%s" % (_TN[dtype], "planes" if head_major else "rows",
                                                                            " ln_out" if ln else ""), ratios, means))
