"""The fused optimizer step on the GPU (`FusedAdamW`, `ops.adamw_step`: dd_adamw_step's three launches) against the numpy
restatement tests/adamw_reference.py, which tests/test_adamw_cpu.py pins to torch.optim.AdamW + clip_grad_norm_ in float64.

The table: eleven rows carved from flat buffers so that the parameters' and gradients' addresses are 4-, 8- and 16-byte
aligned in turn — 1, 3, 255, 256, 257, C - 1, C, C + 1 and 3 C + 5 elements (C = ops.adamw_chunk()), an empty row, a row
whose gradient is None.  Four steps, gradients of norm 200 (the clip bites) and 0.5 (the coefficient clamps to 1) in turn,
at the reference's hyper-parameters and at a loud setting.

What is asserted: m, v, p and the shadows are the fp32 form's BITS when that form is given the kernel's own fp32 scalars;
those scalars are within tests.adamw_reference.scalar_bounds of their float64 values; every step is inside
tests.adamw_reference.bounds of the float64 form from the same state.  Nothing here is fitted to what the kernels give.
"""
import numpy as np
import pytest
import torch

from dualdiff_amd import ops
from dualdiff_amd.networks.layers import derived
from dualdiff_amd.pipeline import FusedAdamW
from tests import adamw_reference as R

pytestmark = pytest.mark.gpu

C = ops.adamw_chunk()
SHADOWS = {"fp16": torch.float16, "bf16": torch.bfloat16}
GAP = 8                                             # sentinel elements between two rows of a flat buffer


@pytest.fixture(scope="module")
def fix():
    return R.fixture(C)


class Flat:
    """rows carved from one flat buffer, their byte addresses 4-, 8- and 16-aligned in turn (starting at `turn`); the
    elements between the rows hold a sentinel that nothing may overwrite"""

    def __init__(self, sizes, dtype, dev, turn=0, sentinel=7.0):
        per4 = 4 // torch.empty((), dtype=dtype).element_size()          # elements per 4 bytes
        at, self.offsets = 0, []
        for i, n in enumerate(sizes):
            at = (at + 4 * per4 - 1) // (4 * per4) * (4 * per4) + (1, 2, 0)[(i + turn) % 3] * per4
            self.offsets.append(at)
            at += n + GAP
        self.flat = torch.full((at + GAP,), sentinel, dtype=dtype, device=dev)
        self.rows = [self.flat[o:o + n] for o, n in zip(self.offsets, sizes)]
        self.sentinel = sentinel
        assert self.flat.data_ptr() % 16 == 0
        assert {r.data_ptr() % 16 for r in self.rows[:3]} == {4 % 16, 8, 0} or per4 != 1

    def fill(self, arrays):
        for r, a in zip(self.rows, arrays):
            if a is not None:
                r.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(r.dtype))

    def gaps_intact(self):
        keep = torch.ones_like(self.flat, dtype=torch.bool)
        for o, r in zip(self.offsets, self.rows):
            keep[o:o + r.numel()] = False
        return bool((self.flat[keep] == self.sentinel).all())


def half_bits(t):
    return t.detach().view(torch.int16).cpu().numpy().view(np.uint16)


class Run:
    """a FusedAdamW over the fixture's rows"""

    def __init__(self, dev, state, hyper, shadow="fp16", turn=0, **kw):
        sizes = [p.size for p in state["p"]]
        self.p, self.g = Flat(sizes, torch.float32, dev, turn), Flat(sizes, torch.float32, dev, turn)
        self.sh = Flat(sizes, SHADOWS[shadow], dev, turn)
        self.p.fill(state["p"])
        self.sh.fill(state["p"])
        self.shadow = shadow
        args = dict(hyper)
        args.update(kw)
        self.opt = FusedAdamW(self.p.rows, shadows=dict(zip(self.p.rows, self.sh.rows)), **args)
        self.m = [self.opt.state[p]["exp_avg"] for p in self.p.rows]
        self.v = [self.opt.state[p]["exp_avg_sq"] for p in self.p.rows]

    def set_grads(self, gs, scale=None):
        for p, buf, g in zip(self.p.rows, self.g.rows, gs):
            if g is None:
                p.grad = None
            else:
                buf.copy_(torch.from_numpy(g if scale is None else g * np.float32(scale)))
                p.grad = buf

    def read(self):
        blk = self.opt._state_block.cpu()
        f = lambda name: ops.adamw_state_field(blk, name).item()                         # noqa: E731
        st = dict(p=[t.cpu().numpy() for t in self.p.rows], m=[t.cpu().numpy() for t in self.m],
                  v=[t.cpu().numpy() for t in self.v], step=f("step"), b1p=f("beta1_pow"), b2p=f("beta2_pow"),
                  skipped=f("skipped"), found_inf=f("found_inf"))
        scal = {k: np.float32(f(k)) for k in ("grad_norm", "lr", "inv_scale") + R.SCALAR_NAMES}
        return st, scal, [half_bits(t) for t in self.sh.rows]

    def versions(self):
        return [[t._version for t in ts] for ts in (self.p.rows, self.m, self.v, self.sh.rows)]


def same_state(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for k in "pmv" for x, y in zip(a[k], b[k])) and \
        all(a[k] == b[k] for k in ("step", "b1p", "b2p", "skipped", "found_inf"))


def check_step(before, got, scal, shadows, gs, hyper, table, shadow, grad_scale=None):
    """the three conditions of a taken step -> the worst error / bound against the float64 form"""
    want, _ = R.step(before, gs, hyper, table, grad_scale=grad_scale, scalars=scal)
    assert (got["step"], got["skipped"], got["found_inf"]) == (want["step"], want["skipped"], 0)
    assert (got["b1p"], got["b2p"]) == (want["b1p"], want["b2p"])
    for i in range(len(gs)):
        for a in "pmv":
            assert np.array_equal(got[a][i].view(np.uint32), want[a][i].view(np.uint32)), (a, i)
        assert np.array_equal(shadows[i], R.shadow_bits(want["p"][i], shadow)), i
    ref, s64 = R.step(before, gs, hyper, table, form="float64", grad_scale=grad_scale)
    n = sum(g.size for g in gs if g is not None)
    en, ec, rel = R.scalar_bounds(n, s64["grad_norm"], s64["clip_coef"], hyper["max_grad_norm"])
    print("grad_norm %.9g (float64 %.17g, bound %.3g)  clip_coef %.9g (float64 %.17g, bound %.3g)"
          % (scal["grad_norm"], s64["grad_norm"], en, scal["clip_coef"], s64["clip_coef"], ec))
    assert abs(float(scal["grad_norm"]) - s64["grad_norm"]) <= en and abs(float(scal["clip_coef"]) - s64["clip_coef"]) <= ec
    for key in R.SCALAR_NAMES[1:] + ("lr",):                                             # one fp32 rounding of the float64 value
        assert scal[key] == np.float32(s64[key]), key
    worst = 0.0
    inv = R.inv_scale_of(grad_scale)
    for i, g in enumerate(gs):
        if g is None:
            continue
        row = {a: before[a][i] for a in "pmv"}
        for a, bound in zip("mvp", R.bounds(row, g, s64, inv_scale=inv, clip_rel=rel)):
            worst = max(worst, R.worst_ratio(got[a][i], ref[a][i], bound))
    assert worst < 1.0
    return worst


# ---- cases 1, 2 and 6: four steps ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,shadow", [("defaults", "fp16"), ("loud", "bf16")])
def test_four_steps_are_the_fp32_form(gpu, fix, name, shadow):
    """cases 1 and 2: bits, scalars, bounds, shadows, version counts, a derived entry — and case 6 on the way: a schedule
    whose first entry is zero (p keeps its bits while m and v move) and which ends before the steps do"""
    hyper = R.HYPERS[name]
    state, grads = fix
    table = [np.float32(0.0), np.float32(hyper["lr"]), np.float32(hyper["lr"] / 2)]
    run = Run(gpu, state, hyper, shadow, lr_table=torch.tensor(table, device=gpu))

    class Holder:
        pass
    holder, built = Holder(), []
    key_row = 4
    pack = lambda: derived(holder, "w", [run.sh.rows[key_row]], lambda: built.append(1) or len(built))   # noqa: E731
    assert pack() == 1 and pack() == 1
    before, worst = R.copy_state(state), 0.0
    for k, gs in enumerate(grads):
        run.set_grads(gs)
        v0 = run.versions()
        run.opt.step()
        v1 = run.versions()
        got, scal, shadows = run.read()
        worst = max(worst, check_step(before, got, scal, shadows, gs, hyper, table, shadow))
        assert scal["lr"] == table[min(k, 2)]
        for i, g in enumerate(gs):
            rose = [b[i] > a[i] for a, b in zip(v0, v1)]               # p, m, v, shadow
            assert rose[1:3] == [g is not None] * 2, (i, rose)        # p and shadow are views: one count per flat buffer
            assert g is None or (rose[0] and rose[3]), (i, rose)
            assert torch.equal(run.sh.rows[i], run.p.rows[i].to(SHADOWS[shadow]))
            if g is None:
                for a in "pmv":
                    assert np.array_equal(got[a][i], state[a][i])
        assert pack() == k + 2 and pack() == k + 2                    # rebuilt once per taken step
        if k == 0:
            for i, g in enumerate(gs):
                assert np.array_equal(got["p"][i].view(np.uint32), state["p"][i].view(np.uint32))
                assert g is None or g.size == 0 or (np.any(got["m"][i] != 0) and np.any(got["v"][i] != 0))
        before = got
    assert run.p.gaps_intact() and run.g.gaps_intact() and run.sh.gaps_intact()
    assert int(run.opt.steps_taken) == 4 and int(run.opt.skipped) == 0 and int(run.opt.found_inf) == 0
    for gbuf, g in zip(run.g.rows, grads[-1]):                        # the gradients are not rewritten
        assert g is None or np.array_equal(gbuf.cpu().numpy(), g)
    print("%s: worst error / bound against the float64 form = %.3f" % (name, worst))


@pytest.mark.parametrize("turn", [0, 1, 2])
def test_rows_that_share_their_misalignment(gpu, fix, turn):
    """ops.adamw_step on a table whose p, g, m and v all sit at the same offset of a 16-byte line (views into flat
    buffers): the scalar head, the 16-byte body and the scalar tail of launch 3 — and shadows that are only 2-byte
    aligned.  Bits of the fp32 form; nothing outside the rows is written."""
    hyper = R.LOUD
    state, grads = fix
    sizes = [p.size for p in state["p"]]
    p, g, m, v = (Flat(sizes, torch.float32, gpu, turn) for _ in range(4))
    sh = Flat([n + 1 for n in sizes], torch.float16, gpu, turn)
    shadow_rows = [r[1:] for r in sh.rows]                               # 2 bytes past a 4-byte boundary
    p.fill(state["p"])
    start = R.copy_state(state)
    rng = np.random.default_rng(5)
    start["m"] = [rng.normal(0, 1e-3, n).astype(np.float32) for n in sizes]
    start["v"] = [(rng.normal(0, 1e-3, n) ** 2).astype(np.float32) for n in sizes]
    start["step"], start["b1p"], start["b2p"] = 7, 0.9 ** 7, 0.999 ** 7
    m.fill(start["m"])
    v.fill(start["v"])
    g.fill(grads[0])
    rows = [(p.rows[i], None if grads[0][i] is None else g.rows[i], m.rows[i], v.rows[i], shadow_rows[i])
            for i in range(len(sizes))]
    table, shadow_dtype = ops.adamw_table(rows)
    assert shadow_dtype == torch.float16
    block = ops.adamw_state(7, hyper["betas"]).to(gpu)
    lr = torch.tensor([hyper["lr"]], dtype=torch.float32, device=gpu)
    ops.adamw_step(table.to(gpu), ops.adamw_chunks(sizes).to(gpu), block, lr, betas=hyper["betas"], eps=hyper["eps"],
                   weight_decay=hyper["weight_decay"], max_grad_norm=hyper["max_grad_norm"])
    host = block.cpu()
    scal = {k: np.float32(ops.adamw_state_field(host, k).item()) for k in R.SCALAR_NAMES}
    want, _ = R.step(start, grads[0], hyper, [np.float32(hyper["lr"])], scalars=scal)
    assert int(ops.adamw_state_field(host, "step")) == 8
    for i in range(len(sizes)):
        for a, flat in (("p", p), ("m", m), ("v", v)):
            assert np.array_equal(flat.rows[i].cpu().numpy().view(np.uint32), want[a][i].view(np.uint32)), (a, i)
        if grads[0][i] is not None:
            assert np.array_equal(half_bits(shadow_rows[i]), R.shadow_bits(want["p"][i], "fp16")), i
            assert float(sh.rows[i][0]) == sh.sentinel
    assert all(f.gaps_intact() for f in (p, g, m, v, sh))


# ---- case 3: non-finite gradients ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["inf_last", "nan_first"])
def test_a_non_finite_gradient_skips_the_step(gpu, fix, where):
    hyper = R.DEFAULTS
    state, grads = fix
    run, clean = Run(gpu, state, hyper), Run(gpu, state, hyper)
    for r in (run, clean):
        r.set_grads(grads[0])
        r.opt.step()
    bad = [None if g is None else g.copy() for g in grads[1]]
    if where == "inf_last":
        bad[8][-1] = np.inf                                           # the last element of the last chunk with a gradient
    else:
        bad[0][0] = np.nan                                            # the first element of the first row
    run.set_grads(bad)
    snap = [f.flat.clone() for f in (run.p, run.sh)] + [t.clone() for t in run.m + run.v]
    taken = int(run.opt.steps_taken)
    v0 = run.versions()
    run.opt.step()
    now = [f.flat for f in (run.p, run.sh)] + run.m + run.v
    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(snap, now))
    assert int(run.opt.steps_taken) == taken == 1 and int(run.opt.found_inf) == 1 and int(run.opt.skipped) == 1
    assert run.versions() != v0                                       # a step that MAY be taken counts: nothing was read back
    for r in (run, clean):
        r.set_grads(grads[1])
        r.opt.step()
    a, sa, ha = run.read()
    b, sb, hb = clean.read()
    assert a["skipped"] == 1 and b["skipped"] == 0 and a["found_inf"] == 0
    a["skipped"] = 0
    assert same_state(a, b) and all(np.array_equal(x, y) for x, y in zip(ha, hb))
    assert all(sa[k].view(np.uint32) == sb[k].view(np.uint32) for k in sa)               # the same lr-table entry too


# ---- case 4: the scaler ----------------------------------------------------------------------------------------------------

def test_grad_scale_and_the_scalers_found_inf(gpu, fix):
    hyper = R.DEFAULTS
    state, grads = fix
    plain, scaled, amp = Run(gpu, state, hyper), Run(gpu, state, hyper), Run(gpu, state, hyper)
    scaler = torch.amp.GradScaler("cuda", init_scale=65536.0)
    scaler.scale(torch.zeros((), device=gpu))                         # creates the scale on the device
    for k in range(2):
        plain.set_grads(grads[k])
        plain.opt.step()
        scaled.set_grads(grads[k], scale=65536.0)
        scaled.opt.step(grad_scale=65536.0)
        amp.set_grads(grads[k], scale=65536.0)
        scaler.step(amp.opt)                                          # sets grad_scale / found_inf on the optimizer
        scaler.update()
    want, sw, hw = plain.read()
    for r in (scaled, amp):
        got, sg, hg = r.read()
        assert same_state(got, want) and all(np.array_equal(x, y) for x, y in zip(hg, hw))
        assert sg["grad_norm"].view(np.uint32) == sw["grad_norm"].view(np.uint32) and sg["inv_scale"] == np.float32(2.0 ** -16)
    before, _, _ = scaled.read()
    check = Run(gpu, state, hyper)                                    # ... and the scaled step is the fp32 form with that scale
    check.set_grads(grads[0], scale=65536.0)
    check.opt.step(grad_scale=torch.tensor(65536.0, device=gpu))
    got, scal, shadows = check.read()
    check_step(state, got, scal, shadows, [None if g is None else g * np.float32(65536.0) for g in grads[0]], hyper,
               [np.float32(hyper["lr"])], "fp16", grad_scale=65536.0)
    # an incoming found_inf of 1 skips the step
    scaled.set_grads(grads[2], scale=65536.0)
    scaled.opt.grad_scale = torch.tensor(65536.0, device=gpu)
    scaled.opt.found_inf = torch.ones((), device=gpu)
    scaled.opt.step()
    del scaled.opt.grad_scale, scaled.opt.found_inf
    after, _, _ = scaled.read()
    assert (after["step"], after["skipped"], after["found_inf"]) == (2, 1, 1)
    after["skipped"], after["found_inf"] = 0, 0
    assert same_state(after, before)
    scaled.opt.step(grad_scale=65536.0)                               # the mark is gone with the attribute
    assert int(scaled.opt.steps_taken) == 3 and int(scaled.opt.found_inf) == 0


# ---- case 5: the same bits every time ------------------------------------------------------------------------------------------

def test_same_step_same_bits_wherever_the_rows_lie(gpu, fix):
    hyper = R.LOUD
    state, grads = fix
    results = []
    for turn in (0, 0, 1):                                            # twice the same layout, once another alignment
        run = Run(gpu, state, hyper, "bf16", turn=turn)
        for gs in grads[:2]:
            run.set_grads(gs)
            run.opt.step()
        results.append(run.read())
    for st, scal, sh in results[1:]:
        assert same_state(st, results[0][0]) and all(np.array_equal(x, y) for x, y in zip(sh, results[0][2]))
        assert all(scal[k].view(np.uint32) == results[0][1][k].view(np.uint32) for k in scal)


# ---- case 7: a captured step ---------------------------------------------------------------------------------------------------

def test_captured_step_replays_as_eager_steps(gpu, fix):
    hyper = R.DEFAULTS
    state, grads = fix
    eager, graphed = Run(gpu, state, hyper), Run(gpu, state, hyper)
    for r in (eager, graphed):                                        # the warm-up step uploads the table
        r.set_grads(grads[0])
        r.opt.step()
    for gs in grads[1:]:
        eager.set_grads(gs)
        eager.opt.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.opt.step()
    assert int(graphed.opt.steps_taken) == 1                          # capturing runs nothing
    for gs in grads[1:]:
        graphed.set_grads(gs)                                         # copies into the same gradient buffers
        graph.replay()
    a, sa, ha = eager.read()
    b, sb, hb = graphed.read()
    assert a["step"] == 4 and same_state(a, b) and all(np.array_equal(x, y) for x, y in zip(ha, hb))
    assert all(sa[k].view(np.uint32) == sb[k].view(np.uint32) for k in sa)
    other = torch.cuda.CUDAGraph()
    with torch.cuda.graph(other):
        graphed.p.rows[3].grad = torch.zeros_like(graphed.p.rows[3])
        with pytest.raises(RuntimeError, match="during a stream capture"):
            graphed.opt.step()
    assert same_state(graphed.read()[0], b)


# ---- case 8: a state torch wrote -----------------------------------------------------------------------------------------------

def test_state_of_a_torch_adamw_continues(gpu):
    hyper = dict(R.LOUD, max_grad_norm=None)
    torch.manual_seed(3)
    sizes = [5, 300, C + 9]
    cpu = [torch.randn(n).mul_(0.05).requires_grad_() for n in sizes]
    ref = torch.optim.AdamW(cpu, lr=float(np.float32(hyper["lr"])), betas=hyper["betas"], eps=hyper["eps"],
                            weight_decay=hyper["weight_decay"])
    for _ in range(2):
        for p in cpu:
            p.grad = torch.randn_like(p) * 0.01
        ref.step()
    params = [p.detach().to(gpu) for p in cpu]
    opt = FusedAdamW(params, lr=1.0)                                  # every hyper-parameter comes with the state
    opt.load_state_dict(ref.state_dict())
    g = [np.random.default_rng(9).normal(0, 0.01, n).astype(np.float32) for n in sizes]
    before = dict(p=[p.detach().numpy().copy() for p in cpu], m=[ref.state[p]["exp_avg"].numpy().copy() for p in cpu],
                  v=[ref.state[p]["exp_avg_sq"].numpy().copy() for p in cpu], step=2, b1p=hyper["betas"][0] ** 2,
                  b2p=hyper["betas"][1] ** 2, skipped=0, found_inf=0)
    for p, x in zip(params, g):
        p.grad = torch.from_numpy(x).to(gpu)
    opt.step()
    host = opt._state_block.cpu()
    scal = {k: np.float32(ops.adamw_state_field(host, k).item()) for k in R.SCALAR_NAMES}
    want, _ = R.step(before, g, hyper, [np.float32(hyper["lr"])], scalars=scal)
    assert int(opt.steps_taken) == 3 and float(opt.clip_coef) == 1.0
    assert scal["step_size"] == np.float32(float(np.float32(hyper["lr"])) / (1.0 - want["b1p"]))
    for i, p in enumerate(params):
        for a, t in (("p", p), ("m", opt.state[p]["exp_avg"]), ("v", opt.state[p]["exp_avg_sq"])):
            assert np.array_equal(t.cpu().numpy().view(np.uint32), want[a][i].view(np.uint32)), (a, i)
    back = opt.state_dict()
    assert float(back["state"][0]["step"]) == 3.0 and back["state"][2]["exp_avg"].is_cuda
