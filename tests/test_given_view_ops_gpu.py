"""Given-view kernels (dd_cfg_ddim_step_given, dd_cfg_unipc_step_given, dd_given_views_noise) on the GPU.

Rounding bound of a re-noised element.  The kernel evaluates add_noise = sa c + s1a n0 in fp32 with fp32 coefficients
(sa, s1a rounded from fp64: relative error <= 2^-24 each) and rounds once to the storage type T.  Against the fp64
add_noise `ref` of the fp64 coefficients the fp32 value is off by at most delta = 4 * 2^-24 (sa |c| + s1a |n0|)
(two coefficient roundings, the product and the sum), and the final rounding adds half an ulp of T; so
        |out - ref| <= ulp_T(ref) + delta
which is 1 ulp of T except where sa c and s1a n0 nearly cancel (there delta, an fp32-sized term, may exceed it).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]


def rnd(shape, dtype, seed, scale=1.0, device="cuda"):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype).to(device)


def ulp(ref, dtype):
    """ulp of the storage type at |ref| (subnormal spacing below the smallest normal)."""
    fi = torch.finfo(dtype)
    e = torch.floor(torch.log2(ref.abs().clamp_min(fi.tiny)))
    return torch.exp2(e - (10 if dtype == torch.float16 else 7))


def assert_renoised(out, clean, n0, sa, s1a, dtype, what):
    """out (storage type) against the fp64 add_noise; sa, s1a fp64 python floats."""
    c, n = clean.double().cpu(), n0.double().cpu()
    ref = sa * c + s1a * n
    err = (out.double().cpu() - ref).abs()
    bound = ulp(ref, dtype) + 4 * 2.0 ** -24 * (sa * c.abs() + s1a * n.abs())
    worst = (err / bound).max().item() if err.numel() else 0.0
    print("%-44s %-8s max err / bound = %.3f" % (what, str(dtype).split(".")[-1], worst))
    assert worst <= 1.0, what


def sqrt_acp(t):
    from tests.given_view_reference import alphas_cumprod
    a = alphas_cumprod()[int(t)]
    return a.sqrt().item(), (1 - a).sqrt().item()


def _given(ops, views, view_elems, seed, dtype, mode, frac=0.5, mask=None):
    g = torch.Generator().manual_seed(seed)
    if mask is None:
        mask = torch.rand(views, generator=g) < frac
        mask[0], mask[-1] = True, False                          # at least one of each
    clean = (torch.randn(views * view_elems, generator=g)).cuda()
    noise0 = rnd((views * view_elems,), dtype, seed + 1)
    gv = ops.GivenViews(mask.to(torch.uint8).cuda(), clean, noise0, torch.empty(3, device="cuda"), mode)
    return gv, mask


@pytest.fixture(scope="module")
def ops(gpu):
    from dualdiff_amd import ops as O
    return O


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sampler", ["ddim", "unipc"])
@pytest.mark.parametrize("mode", [1, 2])
def test_zero_mask_is_the_plain_kernel_bitwise(ops, dtype, sampler, mode):
    from dualdiff_amd.pipeline.pipeline_bev_controlnet import ddim_schedule
    from dualdiff_amd.pipeline.schedulers import given_view_table, unipc_schedule
    views, ve = 12, 4 * 28 * 50
    n = views * ve
    ts, tab = (ddim_schedule if sampler == "ddim" else unipc_schedule)(8)
    _, gtab = given_view_table(ts)
    gv, _ = _given(ops, views, ve, 5, dtype, mode, mask=torch.zeros(views, dtype=torch.bool))
    x_p = rnd((n,), dtype, 1)
    x_g = x_p.clone()
    dup_p, dup_g = torch.empty_like(x_p), torch.empty_like(x_p)
    hist_p = torch.zeros((3, n), dtype=torch.float32, device="cuda")
    hist_g = hist_p.clone()
    for i in range(len(ts)):
        eps = rnd((2, n), dtype, 20 + i)
        coef = tab[i].cuda()
        gv.gcoef.copy_(gtab[i])
        if sampler == "ddim":
            ops.cfg_ddim_step(eps, x_p, coef, 2.0, x_out=x_p, x_dup=dup_p)
            ops.cfg_ddim_step(eps, x_g, coef, 2.0, x_out=x_g, x_dup=dup_g, given=gv)
        else:
            ops.cfg_unipc_step(eps, x_p, hist_p, coef, 2.0, x_out=x_p, x_dup=dup_p)
            ops.cfg_unipc_step(eps, x_g, hist_g, coef, 2.0, x_out=x_g, x_dup=dup_g, given=gv)
        assert torch.equal(x_p, x_g) and torch.equal(dup_p, dup_g), i
        assert torch.equal(hist_p, hist_g), i


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("sampler", ["ddim", "unipc"])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("views,hw", [(12, (28, 50)), (48, (28, 50)), (12, (14, 25))])
def test_given_run_follows_restatement(ops, dtype, sampler, mode, views, hw):
    """A whole 8-step run: non-given elements bitwise equal to the plain kernel fed the same inputs; re-noised given
    elements within the bound of the module docstring; every element follows the restated scheduler step with the
    reference's given-view rule (the kernel's stored sample and history fed back, as test_cfg_unipc_sequence does);
    x_out == x_dup.  (14, 25): view_elems = 1400, n not a multiple of 256."""
    from dualdiff_amd.pipeline.pipeline_bev_controlnet import ddim_schedule
    from dualdiff_amd.pipeline.schedulers import given_view_table, unipc_schedule
    from tests.given_view_reference import make_scheduler
    ve = 4 * hw[0] * hw[1]
    n, g = views * ve, 2.0
    ts_ = (ddim_schedule if sampler == "ddim" else unipc_schedule)(8)
    tab = ts_[1]
    _, gtab = given_view_table(ts_[0])
    sch = make_scheduler(sampler)
    ts = sch.set_timesteps(8)
    assert list(ts) == ts_[0].tolist()
    gv, mask = _given(ops, views, ve, 7 + views, dtype, mode)
    sel = mask.repeat_interleave(ve)                             # element -> given
    n0 = gv.noise0.double().cpu()
    x = rnd((n,), dtype, 3)
    hist = torch.zeros((3, n), dtype=torch.float32, device="cuda")
    dup = torch.empty_like(x)
    for i, t in enumerate(ts.tolist()):
        eps = rnd((2, n), dtype, 40 + i)
        coef = tab[i].cuda()
        gv.gcoef.copy_(gtab[i])
        x_in, hist_in = x.clone(), hist.clone()
        # the plain kernel on the same inputs
        x_plain, hist_plain = x_in.clone(), hist_in.clone()
        if sampler == "ddim":
            ops.cfg_ddim_step(eps, x_plain, coef, g, x_out=x_plain)
            ops.cfg_ddim_step(eps, x, coef, g, x_out=x, x_dup=dup, given=gv)
        else:
            ops.cfg_unipc_step(eps, x_plain, hist_plain, coef, g, x_out=x_plain)
            ops.cfg_unipc_step(eps, x, hist, coef, g, x_out=x, x_dup=dup, given=gv)
        assert torch.equal(x, dup)
        xc, pc = x.cpu(), x_plain.cpu()
        assert torch.equal(xc[~sel], pc[~sel]), "step %d: non-given elements differ from the plain kernel" % i
        if sampler == "unipc" and mode == 1:                      # history advanced from the step's real input
            assert torch.equal(hist, hist_plain)
        if sampler == "unipc":
            assert torch.equal(hist.cpu()[:, ~sel], hist_plain.cpu()[:, ~sel])
        # restated step: the reference's rule on the kernel's input
        e32 = eps.float().cpu()
        guided = (e32[0] + g * (e32[1] - e32[0])).to(dtype).double()
        if mode == 2:
            guided = torch.where(sel, n0, guided)
        ref = sch.step(guided, t, x_in.double().cpu())
        renoise = mode == 1 and i < len(ts) - 1
        if renoise:                                               # the top of the next step (given_view.py:283-295)
            sa, s1a = sqrt_acp(ts[i + 1])
            assert_renoised(xc[sel], gv.clean.cpu()[sel], n0[sel], sa, s1a, dtype, "step %d re-noised" % i)
            keep = ~sel
        else:
            keep = torch.ones_like(sel)
        y, r = xc[keep].double(), ref[keep]
        err = (y - r).abs().max().item()
        tol = 3.0 * (2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7) * r.abs().max().item()
        assert err <= tol, (i, err, tol)
        if sampler == "unipc":                                    # follow the kernel so errors do not compound
            sch.last_sample = hist[0].cpu().double()
            sch.model_outputs = [hist[2].cpu().double(), hist[1].cpu().double()]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("views,hw", [(12, (28, 50)), (48, (14, 25))])
def test_given_views_noise(ops, dtype, views, hw):
    from dualdiff_amd.pipeline.pipeline_bev_controlnet import ddim_schedule
    from dualdiff_amd.pipeline.schedulers import given_view_table
    ve = 4 * hw[0] * hw[1]
    n = views * ve
    ts, _ = ddim_schedule(50)
    t0, _ = given_view_table(ts)
    gv, mask = _given(ops, views, ve, 9, dtype, 1)
    sel = mask.repeat_interleave(ve)
    x = rnd((n,), dtype, 4)
    dup = rnd((n,), dtype, 5)
    x0, dup0 = x.cpu(), dup.cpu()
    ops.given_views_noise(x, gv, t0, x_dup=dup)
    xc, dc = x.cpu(), dup.cpu()
    assert torch.equal(xc[~sel], x0[~sel]) and torch.equal(dc[~sel], dup0[~sel])
    assert torch.equal(xc[sel], dc[sel])
    sa, s1a = sqrt_acp(ts[0])
    assert_renoised(xc[sel], gv.clean.cpu()[sel], gv.noise0.cpu()[sel], sa, s1a, dtype, "pre-loop noising")
    # without x_dup
    y = rnd((n,), dtype, 4)
    ops.given_views_noise(y, gv, t0)
    assert torch.equal(y.cpu(), xc)
