"""small_ops_reference.py without a GPU: every reference against an independent torch formulation, every checker against a
legal fp32 evaluation of its kernel's arithmetic (must pass) and against the faults it is there for (must fail), and the
ambiguity condition of the guided noise on the inputs test_small_ops_fp64_gpu.py uses.

The faults: a store that rounds toward zero; one element two units of T off; one 16-byte vector (8 elements) left at an
old value (NaN as the GPU test pre-fills it, and a finite stale value); the last column and the last row not written;
and for the two convolutions a kernel that ignores channels 3..7 of a cin = 8 input.  The first two are faults of a
rounding to T, so they are applied to the outputs stored in T (the UniPC history and the fp32 posterior are fp32:
two fp32 units are inside any fp32 arithmetic bound).  A truncating store is not applied where every inexact result is an
exact tie (sums of operands near 1000, scaling by a power of two): either neighbour answers a tie equally closely."""
import pytest
import torch
import torch.nn.functional as F

from oracle import leaf_ops as L
from tests import small_ops_reference as S

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]


def rnd(shape, dtype, seed, scale=1.0):
    return S.rand(shape, dtype, seed, scale, device="cpu")


# ---- the faults -----------------------------------------------------------------------------------------------------------

STALE = 3.0                              # a finite old value that no case has as a result


def toward_zero(ref, dtype):
    r = ref.to(dtype)
    over = r.double().abs() > ref.abs()
    return torch.where(over, r.view(torch.int16) - 1, r.view(torch.int16)).view(dtype)


def two_ulp(y, at):
    m = y.clone().reshape(-1)
    m.view(torch.int16)[at] += 2
    return m.reshape(y.shape)


def stale_vector(y, at, nan):
    m = y.clone().reshape(-1)
    m[at:at + 8] = float("nan") if nan else STALE
    return m.reshape(y.shape)


def rounding_faults(ref, dtype):
    y = ref.to(dtype)
    at = int(ref.abs().reshape(-1).argmax())
    return [("toward zero", toward_zero(ref, dtype)), ("two ulp", two_ulp(y, at))]


def write_faults(y):
    at = (y.numel() // 2) // 8 * 8
    out = [("stale vector (NaN)", stale_vector(y, at, True)), ("stale vector", stale_vector(y, at, False))]
    last_col, last_row = y.contiguous().clone(), y.contiguous().clone()
    last_col[..., -1] = STALE
    last_row.reshape(-1, y.shape[-1])[-1] = STALE
    out += [("last column", last_col)]
    if y.dim() > 1:
        out += [("last row", last_row)]
    return out


def must_pass_and_catch(check, clean, mutants):
    """check(y) raises AssertionError on a wrong y."""
    check(clean)
    for name, y in mutants:
        assert not torch.equal(torch.nan_to_num(y.double(), nan=1e300), torch.nan_to_num(clean.double(), nan=1e300)), name
        with pytest.raises(AssertionError):
            check(y)
            pytest.fail("the checker accepted: " + name)


# ---- add, scale, silu -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_add_scale_silu(dtype):
    n = 8 * 255
    for k, kind in enumerate(S.ADD_KINDS):
        a, b, c = S.add_operands(kind, k, n, dtype, rnd)
        off = 1000.0 if kind == "cancel" else kind[1]
        if kind == "cancel":                  # a + b does round in fp32, and the result is a thousand times smaller
            assert bool(((a.float() + b.float()).double() != a.double() + b.double()).any())
            assert float((a.double() + b.double() + c.double()).abs().median()) < 4.0
        # operands near 1000 are multiples of half a unit of their sum: every inexact sum is a tie, which either
        # neighbour answers equally closely, so a truncating store shows on the other two kinds only
        rf = (lambda r: rounding_faults(r, dtype)) if off == 0.0 else (lambda r: rounding_faults(r, dtype)[1:])
        ref, e = S.add_ref(a, b)
        assert torch.equal(ref, a.double() + b.double())
        must_pass_and_catch(lambda y: S.closest(y, ref, e, "add2"), (a.float() + b.float()).to(dtype),
                            rf(ref) + write_faults(ref.to(dtype)))
        ref3, e3 = S.add_ref(a, b, c)
        must_pass_and_catch(lambda y: S.closest(y, ref3, e3, "add3"), ((a.float() + b.float()) + c.float()).to(dtype),
                            (rounding_faults(ref3, dtype) if kind == "cancel" else rf(ref3)) + write_faults(ref3.to(dtype)))
        refs, es = S.silu_ref(a)
        assert torch.allclose(refs, F.silu(a.double()), rtol=1e-15, atol=0)
        must_pass_and_catch(lambda y: S.closest(y, refs, es, "silu"), F.silu(a.float()).to(dtype),
                            rf(refs) + write_faults(refs.to(dtype)))           # silu(x) = x near 1000: nothing to round


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("s", [0.37, 0.18215, 1 / 0.18215, 0.125, -1.0, 0.0])
def test_scale_every_finite_value(dtype, s):
    """The fp32 product rounded to T passes at every finite value of T, subnormal ones included."""
    x = S.finite_patterns(dtype)
    assert x.numel() % 8 == 0 and x.numel() == {torch.float16: 63488, torch.bfloat16: 65280}[dtype]
    ref, e = S.scale_ref(x, s)
    y = (x.float() * torch.tensor(s, dtype=torch.float32)).to(dtype)
    muts = write_faults(y)
    if s != 0.0:
        muts += rounding_faults(ref, dtype)[1:] + ([("toward zero", toward_zero(ref, dtype))] if abs(s) not in (1.0, 0.125) else [])
    must_pass_and_catch(lambda v: S.closest(v, ref, e, "scale"), y, muts)


def test_overflow_edge():
    """Where the correct rounding is infinite the result must be infinite, unless ref is within E of the threshold."""
    big = torch.tensor([65504.0, 65519.9, 65520.1, 70000.0, -70000.0], dtype=torch.float64)
    inf, mx = float("inf"), 65504.0
    y = torch.tensor([mx, mx, inf, inf, -inf], dtype=torch.float16)
    assert S.closest(y, big, 0.0, "edge") == 0.0
    for bad in ([mx, mx, mx, inf, -inf], [mx, mx, inf, mx, -inf], [mx, mx, inf, inf, inf], [mx, inf, inf, inf, -inf]):
        with pytest.raises(AssertionError):
            S.closest(torch.tensor(bad, dtype=torch.float16), big, 0.0, "edge")
    S.closest(torch.tensor([mx, mx, mx, inf, -inf], dtype=torch.float16), big, 0.5, "edge")     # 65520.1 is within 0.5
    S.closest(torch.tensor([mx, inf, inf, inf, -inf], dtype=torch.float16), big, 0.5, "edge")


# ---- sampler steps --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_guided_noise_ambiguity(dtype):
    """At most MAX_AMBIGUOUS of the elements of every case the GPU test runs (all 8 steps of the UniPC runs)."""
    worst = worst_fused = 0.0
    for n in S.STEP_N:
        for g in S.STEP_G:
            for step in range(8):
                es, amb, fused = S.guided(S.step_eps(n, dtype, g, step), g)
                e1, e3 = es[0], es[-1]
                assert len(es) == (3 if dtype == torch.float16 else 2)
                share = float(amb.double().mean())
                worst, worst_fused = max(worst, share), max(worst_fused, float(fused.double().mean()))
                assert share <= S.MAX_AMBIGUOUS, (n, g, step, share)
                if g == 0.0:
                    assert share == 0.0 and torch.equal(e1, S.step_eps(n, dtype, g, step)[0]) and torch.equal(e3, e1)
    print("largest ambiguous share %s: %.2e; the fma rounded once differs on at most %.2e" % (dtype, worst, worst_fused))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_round_once(dtype):
    """One rounding from fp64: equal to torch's two (through fp32) except next to a rounding boundary, never farther from z
    than either neighbour, ties to even, the overflow threshold; fp16 against numpy's conversion."""
    import numpy as np
    fi = torch.finfo(dtype)
    z = torch.cat([rnd((200000,), torch.float64, 1, 3.0), rnd((20000,), torch.float64, 2, 1e-6),
                   S.finite_patterns(dtype).double() * (1 + 2.0 ** -30)])
    mid = S.finite_patterns(dtype).double().sort().values
    mid = (mid[:-1] + mid[1:]) / 2                                    # every midpoint of neighbouring values, ties included
    z = torch.cat([z, mid, mid * (1 + 2.0 ** -40), mid * (1 - 2.0 ** -40),
                   torch.tensor([fi.max * (1 + 2.0 ** -30), -fi.max * 1.01, 0.0, -0.0, fi.max * 4], dtype=torch.float64)])
    r = S.round_once(z, dtype)
    two = z.to(dtype)
    assert float((r != two).double().mean()) < 0.5 and bool((r != two).any())
    if dtype == torch.float16:
        with np.errstate(over="ignore"):
            want = torch.from_numpy(z.numpy().astype(np.float16))
        assert torch.equal(torch.nan_to_num(r.double()), torch.nan_to_num(want.double()))
    fin = torch.isfinite(r.double())
    up = (r.view(torch.int16) + 1).view(dtype).double()
    down = (r.view(torch.int16) - 1).view(dtype).double()
    err = (r.double() - z).abs()
    ok = (err <= (up - z).abs()) & (err <= (down - z).abs())
    assert bool(ok[fin & torch.isfinite(up) & (r.double() != 0)].all())
    ties = torch.cat([torch.zeros(z.numel() - 3 * mid.numel() - 5, dtype=torch.bool), torch.ones(mid.numel(), dtype=torch.bool),
                      torch.zeros(2 * mid.numel() + 5, dtype=torch.bool)])
    assert bool(((r.view(torch.int16)[ties & fin] & 1) == 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_ddim(dtype):
    from dualdiff_amd.pipeline.pipeline_bev_controlnet import ddim_schedule
    n = 8 * 255
    _, tab = ddim_schedule(50)
    x = rnd((n,), dtype, 1)
    mixed_seen = False
    for row in (0, 25, 49):
        coef = tab[row]
        eps = rnd((2, n), dtype, 2 + row)
        es, amb, fused = S.guided(eps, 3.3)
        e1 = es[0]
        ref, e = S.ddim_ref(x, e1, coef)
        # the oracle (fp32, guided noise not rounded): fed the rounded noise as both halves it is one legal fp32 evaluation
        want = L.cfg_ddim_ref(torch.stack([e1, e1]), x, coef, 0.0)
        assert bool(((want.double() - ref).abs() <= e).all())
        cands = [[S.ddim_ref(x, ek, coef)] for ek in es]
        must_pass_and_catch(lambda y: S.closest_either([y], cands, "ddim"), want.to(dtype),
                            rounding_faults(ref, dtype) + write_faults(ref.to(dtype)))
        # the other evaluations of the guided noise are accepted, and only because their candidates are there
        for k, ek in enumerate(es[1:], 1):
            other = L.cfg_ddim_ref(torch.stack([ek, ek]), x, coef, 0.0).to(dtype)
            S.closest_either([other], cands, "ddim")
            differs = other != want.to(dtype)
            if bool(differs.any()):
                with pytest.raises(AssertionError):
                    S.closest_either([other], cands[:1], "ddim")
                # one evaluation per launch: where each result misses the other's candidate on two elements or more, one
                # that takes a single element from the other evaluation fails under every candidate
                if int((~S.closest_ok(want.to(dtype), *cands[k][0])[0]).sum()) >= 2:
                    mixed = want.to(dtype).clone()
                    at = int((~S.closest_ok(other, *cands[0][0])[0]).nonzero()[0])
                    mixed[at] = other[at]
                    with pytest.raises(AssertionError):
                        S.closest_either([mixed], cands, "ddim")
                    mixed_seen = True
    assert mixed_seen or dtype != torch.float16          # the single rounding differs often enough at g = 3.3


def test_unipc_follows_restatement():
    """unipc_ref with the fp32 table against the step-by-step restatement in fp64, re-seeded from the same state every
    step: the fp32 rounding of the coefficients (at most three deep on a leaf term) is 3u of the absolute terms, E / 2 = 4u."""
    from dualdiff_amd.pipeline.schedulers import unipc_schedule
    from oracle.unipc import UniPCRestated
    n = 4096
    sch = UniPCRestated()
    ts = sch.set_timesteps(8)
    _, tab = unipc_schedule(8)
    x = rnd((n,), torch.float64, 1)
    hist = torch.zeros((3, n), dtype=torch.float64)
    for i, t in enumerate(ts.tolist()):
        e = rnd((n,), torch.float64, 10 + i)
        want = sch.step(e, t, x)
        outs = S.unipc_ref(x, e, hist, tab[i])
        assert bool(((outs[0][0] - want).abs() <= outs[0][1] / 2).all()), i
        assert torch.equal(outs[3][0], hist[1])
        assert bool(((outs[1][0] - sch.last_sample).abs() <= outs[1][1] / 2).all()), i
        assert bool(((outs[2][0] - sch.model_outputs[-1]).abs() <= outs[2][1] / 2).all()), i
        x = outs[0][0]
        hist = torch.stack([outs[1][0], outs[2][0], outs[3][0]])
        sch.last_sample = hist[0]
        sch.model_outputs = [hist[2], hist[1]]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_unipc_checker(dtype):
    """An fp32 evaluation of dd_unipc_coef::step passes on all four outputs; faults of any one output are caught."""
    from dualdiff_amd.pipeline.schedulers import unipc_schedule
    n = 8 * 255
    _, tab = unipc_schedule(8)
    x = rnd((n,), dtype, 1)
    hist = torch.zeros((3, n), dtype=torch.float32)
    for i in range(4):
        c = tab[i]
        eps = rnd((2, n), dtype, 20 + i)
        es, amb, fused = S.guided(eps, 3.3)
        e1 = es[0]
        cands = [S.unipc_ref(x, ek, hist, c) for ek in es]
        xv, ev = x.float(), e1.float()
        x0 = c[0] * xv + c[1] * ev
        xc = c[3] * hist[0] + c[4] * hist[1] + c[5] * hist[2] + c[6] * x0 if float(c[2]) != 0.0 else xv
        r = (c[7] * xc + c[8] * x0 + c[9] * hist[1]).to(dtype)
        outs = [r, xc, x0, hist[1].clone()]
        dts = [None, torch.float32, torch.float32, torch.float32]
        chk = lambda k: (lambda y: S.closest_either(outs[:k] + [y] + outs[k + 1:], cands, "unipc", dts))
        must_pass_and_catch(chk(0), r, rounding_faults(cands[0][0][0], dtype) + write_faults(r))
        for k in (1, 2, 3):
            if i > 0 or k == 2:                    # step 0: last = x and m2 = 0 repeat under a roll
                must_pass_and_catch(chk(k), outs[k], write_faults(outs[k]))
        x, hist = r, torch.stack([xc, x0, hist[1]])


# ---- VAE posterior --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("sample", [False, True], ids=["mode", "sample"])
def test_posterior(dtype, sample):
    m, h, w, scale = 2, 3, 5, 0.18215
    mom = rnd((m * h * w, 8), dtype, 1, 4.0)
    wq, bq = rnd((8, 8), torch.float32, 2), rnd((8,), torch.float32, 3, 8.0)
    noise = rnd((m, 4, h, w), dtype, 4) if sample else None
    ref, e = S.posterior_ref(mom, wq, bq, m, h, w, noise, scale)
    s32 = float(torch.tensor(scale, dtype=torch.float32))

    def formulation(dt):
        p = F.conv2d(mom.to(dt).reshape(m, h, w, 8).permute(0, 3, 1, 2), wq.to(dt).reshape(8, 8, 1, 1), bq.to(dt))
        mean, logvar = p.chunk(2, dim=1)
        z = mean + torch.exp(0.5 * logvar.clamp(-30.0, 20.0)) * noise.to(dt) if sample else mean
        return torch.tensor(s32, dtype=dt) * z
    assert torch.allclose(formulation(torch.float64), ref, rtol=1e-12, atol=1e-12)
    if sample:
        lv = (mom.double() @ wq.double().t() + bq.double())[:, 4:]
        assert bool((lv < -30).any()) and bool((lv > 20).any())          # both clamp ends are in the data
    y32 = formulation(torch.float32)
    S.closest(y32, ref, e, "posterior f32", torch.float32)
    must_pass_and_catch(lambda y: S.closest(y, ref, e, "posterior"), y32.to(dtype),
                        rounding_faults(ref, dtype) + write_faults(ref.to(dtype)))
    must_pass_and_catch(lambda y: S.closest(y, ref, e, "posterior f32", torch.float32), y32, write_faults(y32))


# ---- convolutions ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cin,cout,stride,silu,nchw", [(8, 16, 1, True, False), (8, 16, 2, False, False),
                                                        (16, 32, 2, True, False), (8, 3, 1, False, True)])
def test_conv(dtype, cin, cout, stride, silu, nchw):
    m, h, w = 2, 9, 11
    x = rnd((m * h * w, cin), dtype, 1)
    wt = rnd((cout, cin, 3, 3), dtype, 2, (9 * cin) ** -0.5)
    b = rnd((cout,), dtype, 3)
    wp = L.pack_conv_weight(wt)
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1

    def formulation(xx, dt):
        y = F.conv2d(xx.to(dt).reshape(m, h, w, cin).permute(0, 3, 1, 2), wt.to(dt), b.to(dt), stride=stride, padding=1)
        y = F.silu(y) if silu else y
        return y.contiguous() if nchw else y.permute(0, 2, 3, 1).reshape(-1, cout)
    ref, e = S.conv_ref(x, wp, b, m, h, w, stride, silu)
    if nchw:
        ref, e = S.to_nchw(ref, m, ho, wo), S.to_nchw(e, m, ho, wo)
    assert torch.allclose(formulation(x, torch.float64), ref, rtol=1e-12, atol=1e-12)
    clean = formulation(x, torch.float32).to(dtype)
    muts = rounding_faults(ref, dtype) + write_faults(ref.to(dtype))
    if cin == 8:
        thin = x.clone()
        thin[:, 3:] = 0
        muts.append(("padding channels ignored", formulation(thin, torch.float32).to(dtype)))
    must_pass_and_catch(lambda y: S.conv_check(y, ref, e, "conv"), clean, muts)


# ---- softmax rows ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_softmax(dtype):
    rows, cols = 5, 203
    s = rnd((rows, cols), torch.float32, 1)
    s[1, 7] += 80.0
    s[2] = 3.25
    s[3] += 1e4
    s[4, ::3] = float("-inf")
    ref, e = S.softmax_ref(s)
    assert torch.allclose(ref, torch.softmax(s.double(), dim=1), rtol=1e-13, atol=0)
    assert bool(torch.isfinite(e).all())
    clean = torch.softmax(s, dim=1).to(dtype)
    at = 8 * 3                                                     # inside row 0 (randn logits)
    muts = rounding_faults(ref, dtype) + [("stale vector (NaN)", stale_vector(clean, at, True)),
                                          ("stale vector", stale_vector(clean, at, False))]
    last_col, last_row = clean.clone(), clean.clone()
    last_col[:, -1] = STALE
    last_row[-1] = STALE
    must_pass_and_catch(lambda y: S.closest(y, ref, e, "softmax"), clean, muts + [("last column", last_col), ("last row", last_row)])


# ---- embeddings, layout -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("dim,flip,shift", [(2, True, 0.0), (6, False, 1.0), (320, True, 0.0), (320, False, 1.0)])
def test_timestep(dtype, dim, flip, shift):
    t = torch.tensor([0.0, 1.0, 500.5, 981.0, 999.0])
    ref, e = S.timestep_ref(t, dim, flip, shift)
    want = L.timestep_embedding_ref(t, dim, flip, shift)
    assert bool(((want.double() - ref).abs() <= e).all())
    # dim = 2 is ten values, and those of the large arguments carry an e of half a bf16 unit: too few to show a truncation
    must_pass_and_catch(lambda y: S.closest(y, ref, e, "timestep"), want.to(dtype),
                        rounding_faults(ref, dtype) + write_faults(ref.to(dtype)))


@pytest.mark.parametrize("dtype", [torch.float32] + DTYPES, ids=["f32"] + IDS)
def test_fourier(dtype):
    x = (rnd((5, 6, 3), torch.float32, 1) * 30.0).to(dtype)
    freqs = [2.0 ** i for i in range(4)]
    ref, e = S.fourier_ref(x, freqs, True)
    xf = x.float()
    want = torch.cat([xf] + [f(xf * k) for k in freqs for f in (torch.sin, torch.cos)], dim=-1)
    assert ref.shape == want.shape and bool(((want.double() - ref).abs() <= e).all())
    assert float(e[..., :3].max()) == 0.0 and float(e.max()) == 2.0 ** -22          # power-of-two frequencies: exact arguments
    assert float(S.fourier_ref(x, [3.0], False)[1].max()) > 2.0 ** -22
    for out in DTYPES:
        must_pass_and_catch(lambda y: S.closest(y, ref, e, "fourier"), want.to(out),
                            rounding_faults(ref, out) + write_faults(ref.to(out)))
    S.closest(want, ref, e, "fourier f32", torch.float32)


def test_layout():
    x = rnd((2, 3, 4, 3 * 5), torch.float16, 1)
    y = S.nhwc_ref(x, 8, views=3)
    assert y.shape == (2 * 3 * 4 * 5, 8) and float(y[:, 3:].abs().max()) == 0.0
    assert torch.equal(y[(1 * 3 + 2) * 20 + 3 * 5 + 4, :3], x[1, :, 3, 2 * 5 + 4])
    one = S.nhwc_ref(x, 5)
    assert torch.equal(S.nchw_ref(one, 2, 3, 4, 15), x)
    assert torch.equal(one[:, :3], x.permute(0, 2, 3, 1).reshape(-1, 3))
