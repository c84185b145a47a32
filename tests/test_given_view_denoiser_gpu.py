"""Given-view sampling through BEVDenoiser (set_inputs(..., conditional_latents=...)) on the full-width step case of
tests/golden/cases.py: two ControlNet branches, one scene of 6 views, views 0 and 3 given.

  * graph replay == eager bit for bit, and the eager run's noise predictions pushed through the restated reference
    loop (tests/given_view_reference.py) reproduce the latents — both samplers, both modes;
  * model-independent invariant of mode 2 (fixed noise): both samplers integrate a constant x0 exactly, so with the
    given views' noise pinned to n0 they stay on add_noise(c, n0, t) — up to the rounding bound of
    `_mode2_bound`; mode 1 holds the re-noised value before every step;
  * all-None conditional_latents is the plain sampler; given views change their neighbours through attn4;
  * CFG split and view split compose with given views.
"""
import pytest
import torch

from tests.given_view_reference import alphas_cumprod, reference_loop
from tests.golden import cases as C
from tests.parity_util import rel_l2, report
from tests.test_parity_r02_gpu import _LocalExchange, _denoiser, _to_dev, step_models  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

H, W, NCAM = C.H, C.W, C.N_CAM
GIVEN = (0, 3)
STEPS = {"ddim": 50, "unipc": 20}


def _clean():
    g = torch.Generator().manual_seed(1234)
    return torch.randn((1, NCAM, 4, H, W), generator=g)          # fp32 clean latents of every view


def _cond(clean, given=GIVEN):
    return [[clean[0, j] if j in given else None for j in range(NCAM)]]


def _inputs(dtype):
    inp = C.step_inputs(2)
    return (C.step_latents().cuda().to(dtype), _to_dev(inp["text"], dtype), _to_dev(inp["camera_param"], dtype),
            [_to_dev(inp["boxes_bg"], dtype), _to_dev(inp["boxes_fg"], dtype)],
            [_to_dev(inp["cond_bg"], dtype), _to_dev(inp["cond_fg"], dtype)])


_MODELS = {}


def _models(step_models, dtype):
    if dtype not in _MODELS:
        d = _denoiser(step_models, dtype, use_graph=False)
        _MODELS[dtype] = (d.unet, d.controlnets)
    return _MODELS[dtype]


def _make(step_models, dtype, sampler="ddim", steps=None, cond=None, change=True, **kw):
    from dualdiff_amd.pipeline.pipeline_bev_controlnet import BEVDenoiser
    unet, cns = _models(step_models, dtype)
    den = BEVDenoiser(unet, cns, guidance_scale=2.0, num_inference_steps=steps or STEPS[sampler], sampler=sampler, **kw)
    with torch.no_grad():
        if cond is None:
            den.set_inputs(*_inputs(dtype))
        else:
            den.set_inputs(*_inputs(dtype), conditional_latents=cond, conditional_latents_change_every_input=change)
    return den


@pytest.mark.parametrize("sampler", ["ddim", "unipc"])
@pytest.mark.parametrize("change", [True, False])
def test_given_denoiser_graph_eager_and_reference_loop(step_models, sampler, change):
    dtype, run = torch.bfloat16, 4
    clean = _clean()
    outs, eps_log = {}, []
    for graph in (False, True):
        den = _make(step_models, dtype, sampler, cond=_cond(clean), change=change, use_graph=graph)
        if not graph:
            body = den._step_body

            def logged():
                e = body()
                eps_log.append(e.float().cpu().clone().reshape(2, NCAM, 4, H, W))
                return e
            den._step_body = logged
        with torch.no_grad():
            den.run(run)
        outs[graph] = den.latents.float().cpu()
    assert torch.equal(outs[True], outs[False])
    assert len(eps_log) == run
    calls = iter(eps_log)
    ref = reference_loop(sampler, STEPS[sampler], C.step_latents().to(dtype), _cond(clean), change,
                         lambda x, t: next(calls).double(), guidance=2.0, dtype=dtype, run=run)
    rec = []
    err = report("given views %s change=%s, %d steps" % (sampler, change, run), outs[True], ref.float(), dtype, rec)
    assert err <= 1.0, rec


def _ulp(ref, dtype):
    fi = torch.finfo(dtype)
    e = torch.floor(torch.log2(ref.abs().clamp_min(fi.tiny)))
    return torch.exp2(e - (10 if dtype == torch.float16 else 7))


def _mode2_bound(sampler, coef_table, ts, c, n0, dtype, k_max):
    """Elementwise bound on |x_k - add_noise(c, n0, t_k)| for a given view in mode 2, k = 1..k_max (t_k = the next
    timestep after step k-1, 0 after the last).  First-order propagation of the rounding of every stored value: with
    eps = n0 exact, the update is linear in (x, history) with the step's coefficient row, so an error e in an input
    contributes |coef| e; each step then adds rho = ulp_T(|ref| + e)/2 (rounding, to the storage type, of a
    value within e of ref) + 2^-20 S (fp32
    arithmetic and coefficient rounding: a few 2^-24 of every term, S = sum of |coef| x (|c| + |n0|) over the
    row — 16x headroom over the per-term count).  The fp32 history (UniPC last / m1 / m2) adds only the fp32 term."""
    acp = alphas_cumprod()
    amp = c.abs() + n0.abs()

    def ref_at(t):
        return acp[t].sqrt() * c + (1 - acp[t]).sqrt() * n0

    r0 = ref_at(int(ts[0]))
    e_x = _ulp(r0.abs() + 2.0 ** -20 * amp, dtype) / 2 + 2.0 ** -20 * amp     # dd_given_views_noise
    e_last = e_m1 = e_m2 = torch.zeros_like(c)
    out = []
    for k in range(k_max):
        row = [abs(v) for v in coef_table[k].tolist()]
        t_next = int(ts[k + 1]) if k + 1 < len(ts) else 0
        fp32 = 2.0 ** -20 * (1 + sum(row)) * amp
        if sampler == "ddim":
            sa_t, _, sa_p, _ = row
            e_new = sa_p / sa_t * e_x + fp32
        else:
            a_x, _, use_c, c_l, c_1, c_2, c_0, p_x, p_0, p_1 = row
            e_x0 = a_x * e_x + fp32
            e_xc = (c_l * e_last + c_1 * e_m1 + c_2 * e_m2 + c_0 * e_x0 + fp32) if use_c else e_x
            e_new = p_x * e_xc + p_0 * e_x0 + p_1 * e_m1 + fp32
            e_last, e_m2, e_m1 = e_xc, e_m1, e_x0
        ref = ref_at(t_next)
        e_x = e_new + _ulp(ref.abs() + e_new, dtype) / 2
        out.append((ref, e_x))
    return out


@pytest.mark.parametrize("sampler", ["ddim", "unipc"])
def test_given_views_stay_on_the_noising_path(step_models, sampler):
    """Mode 2 over a whole 4-step schedule (the last step to acp[0]: DDIM's set_alpha_to_one=False, UniPC's t = 0):
    after every step the given views equal add_noise(c, n0, t_next) within `_mode2_bound`, whatever the model does.
    Mode 1: after every step but the last they hold add_noise(c, n0, t_next) within 1 ulp (+ the fp32 term)."""
    dtype, steps = torch.bfloat16, 4
    clean = _clean()
    n0 = C.step_latents().to(dtype).double()[0]
    c = clean.double()[0]
    for change in (False, True):
        den = _make(step_models, dtype, sampler, steps=steps, cond=_cond(clean), change=change, use_graph=True)
        ts = den.timesteps.tolist()
        assert len(ts) == steps
        bounds = _mode2_bound(sampler, den.coef_table.double(), ts, c, n0, dtype, steps)
        acp = alphas_cumprod()
        with torch.no_grad():
            for k in range(steps):
                den.step(k)
                x = den.latents[0].double().cpu()
                for v in GIVEN:
                    if not change:
                        ref, bnd = bounds[k][0][v], bounds[k][1][v]
                        worst = ((x[v] - ref).abs() / bnd).max().item()
                        print("mode 2 %s step %d view %d: max err / bound %.3f" % (sampler, k, v, worst))
                        assert worst <= 1.0, (sampler, k, v, worst)
                    elif k < steps - 1:
                        t = ts[k + 1]
                        ref = acp[t].sqrt() * c[v] + (1 - acp[t]).sqrt() * n0[v]
                        bnd = _ulp(ref, dtype) + 2.0 ** -20 * (c[v].abs() + n0[v].abs())
                        assert ((x[v] - ref).abs() <= bnd).all(), (sampler, k, v)


def test_all_none_is_the_plain_sampler_and_given_views_reach_neighbours(step_models):
    dtype, run = torch.bfloat16, 2
    outs = {}
    for name, cond in (("plain", None), ("none", [[None] * NCAM]), ("given", _cond(_clean()))):
        den = _make(step_models, dtype, "ddim", cond=cond, use_graph=True)
        with torch.no_grad():
            den.run(run)
        outs[name] = den.latents.float().cpu()
    assert torch.equal(outs["plain"], outs["none"])
    for v in range(NCAM):                                      # every other view neighbours view 0 or 3 (VIEW_PAIR)
        if v not in GIVEN:
            assert not torch.equal(outs["given"][0, v], outs["plain"][0, v]), v


def test_given_views_cfg_split(step_models):
    """CFG split (two half denoisers exchanging noise predictions, the local make_exchange pattern of
    test_full_step_dual_branch_graph_vs_oracle): both halves hold the same latents, equal to the unsharded run."""
    dtype, run = torch.float16, 2
    clean = _clean()
    full = _make(step_models, dtype, "unipc", cond=_cond(clean), change=False, use_graph=True)
    with torch.no_grad():
        full.run(run)
    box = {}

    def make_exchange(hf):
        def exchange(eps_half):
            box[hf] = eps_half
            if len(box) < 2:
                return None
            return torch.stack([box[0], box[1]])
        return exchange

    halves = []
    for hf in (0, 1):
        d = _make(step_models, dtype, "unipc", cond=_cond(clean), change=False, use_graph=True, cfg_half=hf,
                  cfg_exchange=make_exchange(hf))
        d._combine_halves = lambda: None                         # the test drives the exchange itself (one process)
        halves.append(d)
    with torch.no_grad():
        for i in range(run):
            for d in halves:
                d.step(i)
            eps2 = torch.stack([halves[0]._eps_half, halves[1]._eps_half])
            for d in halves:
                d._scheduler_step(eps2)
    assert halves[0].m == NCAM and torch.equal(halves[0].latents, halves[1].latents)
    rec = []
    e = report("given views, CFG split vs unsharded", halves[0].latents.float().cpu(), full.latents.float().cpu(),
               dtype, rec)
    assert e <= 1.0, rec


def test_given_views_view_split_one_gpu(step_models):
    """View split over 2 shards as threads on one GPU: the given inputs are sliced like the latents; two steps match
    the unsharded given-view run within the bar of test_view_split_denoiser_one_gpu."""
    import threading
    from dualdiff_amd.parallel import ViewShard, ViewSplitPlan
    dtype, run = torch.float16, 2
    clean = _clean()
    full = _make(step_models, dtype, "ddim", cond=_cond(clean), use_graph=False)
    with torch.no_grad():
        full.run(run)
    want = full.latents.float().cpu()
    plans = [ViewSplitPlan(2, r, C.VIEW_PAIR, cfg_split=False) for r in range(2)]
    ex = _LocalExchange(plans)
    dens = []
    for p in plans:
        d = _denoiser(step_models, dtype, use_graph=False, view_shard=ViewShard(p, ex.bind(p)))
        with torch.no_grad():
            d.set_inputs(*_inputs(dtype), conditional_latents=_cond(clean))
        assert int(d._given.mask.sum()) == sum(1 for v in GIVEN if v in p.local)
        dens.append(d)
    errs = []

    def work(den):
        try:
            with torch.no_grad(), torch.cuda.stream(torch.cuda.Stream()):
                den.run(run)
                torch.cuda.current_stream().synchronize()
        except Exception as e:          # noqa: BLE001  (reported to the main thread)
            errs.append(e)
            ex.barrier.abort()

    torch.cuda.synchronize()
    ths = [threading.Thread(target=work, args=(d,)) for d in dens]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errs, errs
    got = torch.cat([d.latents.float().cpu() for d in dens], dim=1)
    e = rel_l2(got, want)
    print("given views, view split x2: latents after %d steps vs unsharded rel-L2 %.3e" % (run, e))
    assert e <= 2e-3
