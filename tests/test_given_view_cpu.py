"""Given-view sampling (pipeline_bev_controlnet_given_view.py) on the host: the fused per-element rule against the
reference loop restated in fp64, the add_noise table, input conversion and the C-ABI argument checks.  CPU only."""
import ctypes
import os

import numpy as np
import pytest
import torch

from dualdiff_amd.pipeline.pipeline_bev_controlnet import ddim_schedule, given_view_inputs
from dualdiff_amd.pipeline.schedulers import given_view_table, unipc_schedule
from tests.given_view_reference import alphas_cumprod, fused_loop, linear_model, reference_loop

B, N, C, H, W = 2, 6, 4, 3, 5
MASKS = {
    "none": [],
    "all": [(i, j) for i in range(B) for j in range(N)],
    "first": [(0, 0)],
    "last": [(B - 1, N - 1)],
    "first_and_last": [(0, 0), (B - 1, N - 1), (1, 2)],
}


def _timesteps(sampler, steps):
    return (ddim_schedule if sampler == "ddim" else unipc_schedule)(steps)[0]


@pytest.mark.parametrize("sampler,steps", [("ddim", 50), ("unipc", 20)])
@pytest.mark.parametrize("change", [True, False])
@pytest.mark.parametrize("mask", sorted(MASKS))
def test_fused_rule_equals_reference_loop(sampler, steps, change, mask):
    gen = torch.Generator().manual_seed(3)
    lat = torch.randn((B, N, C, H, W), generator=gen, dtype=torch.float64)
    clean = torch.randn((B, N, C, H, W), generator=gen, dtype=torch.float64)
    given = torch.zeros((B, N), dtype=torch.bool)
    for i, j in MASKS[mask]:
        given[i, j] = True
    cond = [[clean[i, j] if given[i, j] else None for j in range(N)] for i in range(B)]
    want = reference_loop(sampler, steps, lat, cond, change, linear_model(11))
    t0, gcoef = given_view_table(_timesteps(sampler, steps), dtype=torch.float64)
    got = fused_loop(sampler, steps, lat, clean, given, 1 if change else 2, linear_model(11), t0, gcoef)
    assert (got - want).abs().max().item() <= 1e-12
    if mask == "none":                          # nothing given: the plain sampler
        plain = reference_loop(sampler, steps, lat, [[None] * N] * B, change, linear_model(11))
        assert torch.equal(want, plain)
    else:                                       # the given views really are held
        free = fused_loop(sampler, steps, lat, clean, torch.zeros_like(given), 1, linear_model(11), t0, gcoef)
        assert (got - free).abs().max().item() > 1e-3


@pytest.mark.parametrize("sampler,steps", [("ddim", 50), ("ddim", 8), ("unipc", 20), ("unipc", 8)])
def test_given_view_table(sampler, steps):
    ts = _timesteps(sampler, steps)
    acp = alphas_cumprod()
    t0, g = given_view_table(ts)
    assert t0.dtype == g.dtype == torch.float32 and t0.shape == (2,) and g.shape == (len(ts), 3)
    t0d, gd = given_view_table(ts, dtype=torch.float64)
    nxt = ts.tolist()[1:] + [0]                 # the sample both samplers end on: acp[0] (DDIM prev < 0, UniPC t = 0)
    for i, t in enumerate(nxt):
        assert abs(gd[i, 0].item() ** 2 - acp[t].item()) <= 1e-14
        assert abs(gd[i, 1].item() ** 2 - (1 - acp[t]).item()) <= 1e-14
    assert gd[:-1, 2].eq(1).all() and gd[-1, 2].item() == 0
    assert abs(t0d[0].item() ** 2 - acp[int(ts[0])].item()) <= 1e-14
    assert abs(t0d[1].item() ** 2 - (1 - acp[int(ts[0])]).item()) <= 1e-14
    assert torch.equal(t0, t0d.float()) and torch.equal(g, gd.float())
    if sampler == "ddim":                       # steps_offset: row i holds the a_prev of ddim_schedule's step i
        _, coef = ddim_schedule(steps)
        assert torch.allclose(g[:, :2], coef[:, 2:], rtol=0, atol=1e-7)
        assert int(ts[-1]) == 1


def test_existing_tables_unchanged():
    ts, coef = ddim_schedule(50)
    assert ts[0].item() == 981 and ts[-1].item() == 1 and coef.shape == (50, 4)
    ts2, tab = unipc_schedule(20)
    assert tab.shape == (len(ts2), 10) and ts2[0].item() == 999


def test_list_of_lists_conversion():
    gen = torch.Generator().manual_seed(0)
    c01 = torch.randn((C, H, W), generator=gen).half()
    c15 = torch.randn((C, H, W), generator=gen, dtype=torch.float64)
    cond = [[None] * N for _ in range(B)]
    cond[0][1], cond[1][5] = c01, c15
    clean, given = given_view_inputs(cond, (B, N, C, H, W))
    assert clean.dtype == torch.float32 and clean.shape == (B, N, C, H, W)
    assert given.dtype == torch.bool and given.tolist() == [[j == 1 for j in range(N)], [j == 5 for j in range(N)]]
    assert torch.equal(clean[0, 1], c01.float()) and torch.equal(clean[1, 5], c15.float())
    assert clean[0, 0].abs().sum() == 0 and clean[1, 4].abs().sum() == 0
    # the dense form round-trips
    clean2, given2 = given_view_inputs(clean.double(), (B, N, C, H, W), mask=given)
    assert torch.equal(clean2, clean) and torch.equal(given2, given)
    # all None: nothing given
    _, none = given_view_inputs([[None] * N for _ in range(B)], (B, N, C, H, W))
    assert not none.any()


def test_conversion_rejects_bad_inputs():
    ok = torch.zeros((C, H, W))
    shape = (B, N, C, H, W)
    with pytest.raises(ValueError, match=r"conditional_latents\[1\] has 5 entries"):
        given_view_inputs([[None] * N, [None] * (N - 1)], shape)
    with pytest.raises(ValueError, match="3 rows"):
        given_view_inputs([[None] * N] * 3, shape)
    bad = [[None] * N for _ in range(B)]
    bad[1][3] = torch.zeros((C, H + 1, W))
    with pytest.raises(ValueError, match=r"conditional_latents\[1\]\[3\]"):
        given_view_inputs(bad, shape)
    bad[1][3] = torch.zeros((1, C, H, W))
    with pytest.raises(ValueError, match=r"conditional_latents\[1\]\[3\]"):
        given_view_inputs(bad, shape)
    bad[1][3] = ok
    given_view_inputs(bad, shape)
    dense = torch.zeros(shape)
    with pytest.raises(ValueError, match="conditional_mask"):
        given_view_inputs(dense, shape)                                          # tensor without a mask
    with pytest.raises(ValueError, match="conditional_mask"):
        given_view_inputs(dense, shape, mask=torch.zeros((B, N + 1), dtype=torch.bool))
    with pytest.raises(ValueError, match="conditional_mask"):
        given_view_inputs(dense, shape, mask=torch.zeros((B, N), dtype=torch.float32))
    with pytest.raises(ValueError, match="has shape"):
        given_view_inputs(torch.zeros((B, N, C, H, W + 1)), shape, mask=torch.zeros((B, N), dtype=torch.bool))
    with pytest.raises(ValueError, match="conditional_mask"):
        given_view_inputs(bad, shape, mask=torch.zeros((B, N), dtype=torch.bool))   # list form with a mask


def test_given_abi_validation_without_a_gpu():
    """The new entry points reject bad arguments before any launch, on a CPU-only box."""
    from dualdiff_amd import _build, _native
    if not os.path.exists(_build.lib_path()):
        pytest.skip("library not built")
    lib = _native.load(build_if_missing=False)
    p, n, ve = 16, 4 * 1400 * 12, 4 * 1400
    for mode in (0, 3):
        assert lib.dd_cfg_ddim_step_given(p, p, p, None, p, 2.0, p, p, p, p, mode, n, ve, 0, None) == -1
        assert lib.dd_cfg_unipc_step_given(p, p, p, None, p, p, p, p, 2.0, p, p, p, p, mode, n, ve, 1, None) == -1
    for bad_ve in (0, -4, ve + 8):                                   # non-positive, not dividing n
        assert lib.dd_cfg_ddim_step_given(p, p, p, None, p, 2.0, p, p, p, p, 1, n, bad_ve, 0, None) == -1
        assert lib.dd_cfg_unipc_step_given(p, p, p, None, p, p, p, p, 2.0, p, p, p, p, 2, n, bad_ve, 0, None) == -1
        assert lib.dd_given_views_noise(p, None, p, p, p, 0.5, 0.5, n, bad_ve, 0, None) == -1
    assert lib.dd_cfg_ddim_step_given(p, p, p, None, p, 2.0, None, p, p, p, 1, n, ve, 0, None) == -1    # mask
    assert lib.dd_cfg_ddim_step_given(p, p, p, None, p, 2.0, p, None, p, p, 1, n, ve, 0, None) == -1    # clean
    assert lib.dd_cfg_ddim_step_given(p, p, p, None, p, 2.0, p, p, None, p, 2, n, ve, 0, None) == -1    # noise0
    assert lib.dd_cfg_ddim_step_given(p, p, p, None, p, 2.0, p, p, p, None, 1, n, ve, 0, None) == -1    # gcoef
    assert lib.dd_cfg_unipc_step_given(p, p, p, None, None, p, p, p, 2.0, p, p, p, p, 1, n, ve, 0, None) == -1
    assert lib.dd_cfg_ddim_step_given(p, p, p, None, p, 2.0, p, p, p, p, 1, n, ve, 2, None) == -1       # dtype
    assert lib.dd_cfg_ddim_step_given(p, p, p, None, p, 2.0, p, p, p, p, 1, 0, ve, 0, None) == -1       # n
    assert lib.dd_given_views_noise(None, None, p, p, p, 0.5, 0.5, n, ve, 0, None) == -1
    assert lib.dd_given_views_noise(p, None, None, p, p, 0.5, 0.5, n, ve, 0, None) == -1
    assert lib.dd_given_views_noise(p, None, p, p, p, 0.5, 0.5, n, ve, 5, None) == -1
    assert lib.dd_given_views_noise(p, None, p, p, p, 0.5, 0.5, 70000, 1, 0, None) == -2               # > 65535 views
    assert lib.dd_desc_size(5) == -1 and lib.dd_desc_size(99) == -1
    assert lib.dd_abi_version() == 4


def test_given_ops_fail_loudly_on_cpu_tensors():
    from dualdiff_amd import ops
    x = torch.zeros(8, dtype=torch.float16)
    g = ops.GivenViews(torch.ones(2, dtype=torch.uint8), torch.zeros(8), x.clone(), torch.zeros(3), 1)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.cfg_ddim_step(torch.zeros(2, 8, dtype=torch.float16), x, torch.zeros(4), 2.0, given=g)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.given_views_noise(x, g, torch.zeros(2))
