"""The per-pixel / per-channel conditions of tests/spatial_cases.py see what the whole-tensor metric does not — shown on the
oracle's own tensors, without a GPU.

1. The reference within its own bounds: for every case, dtype and output, emul of each of the 8 input seeds meets the three
   conditions, and its worst pixel / channel lies within the committed margin of the SMALLEST such statistic over the seeds
   (whichever seed had been the yardstick, the others pass).  The committed margins equal a fresh measurement of one cheap
   case; `python -m tests.spatial_cases --margins` re-measures the whole table.
2. Planted faults: y = emul[dtype] + (faulty oracle - oracle) in float64 stands in for a HIP output with ONE wiring
   mistake of the kind the spatial modules can make.  Each must fail the pixel or the channel condition of its case.
   WHOLE_PASSES states which of them the whole-tensor condition lets through at the case's own shape, and
   test_workload_sized_output states the gap: at the workload's 12 x 28 x 50 pixels the instance bleed — one pixel 16 % off —
   moves the whole-tensor error by 0.16 / sqrt(16800) = 1.3e-3, ON the bound of a single block (1.05 .. 1.3 x), and at the 48
   instances of the video network it is inside it (fp16) or within 1 % of it (bf16); per pixel it is > 30 x the bound.
3. The table: every case constructs on both sides, with the same state_dict keys, so load_state_dict(strict=True) is
   meaningful; outputs and their (m, h, w) agree with what the oracle returns.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

from tests import spatial_cases as S
from tests.test_spatial_blocks_gpu import APPLIES, DEFAULTS, MATRIX, expected

DTYPE_IDS = [S.tag(dt) for dt in S.DTYPES]


@pytest.fixture(scope="module")
def oracle():
    """name -> (float64 oracle module, float64 inputs, oracle_outputs of seed 0)."""
    cache = {}

    def get(name):
        if name not in cache:
            ora, sd = S.make_oracle(name)
            o = S.oracle_outputs(name, 0, (ora, sd))
            cache[name] = (copy.deepcopy(ora).double(), S.to_double(o["inp"]), o)
        return cache[name]
    return get


# ---- 1. the reference within its own bounds --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.CASES))
def test_reference_meets_its_own_conditions_on_every_seed(name):
    runs = S.seed_outputs(name)
    assert len(runs) == S.N_SEEDS == 8
    pool = S.POOL[name]
    for dt in S.DTYPES:
        m_pix, m_ch = S.MARGINS[name][S.tag(dt)]
        assert 1.0 < m_pix <= 2.0 and 1.0 < m_ch <= 2.0
        for out in S.outputs_of(name):
            pix = [S.e_pix(r["emul"][dt][out], r["ref"][out], pool).max().item() for r in runs]
            ch = [S.e_ch(r["emul"][dt][out], r["ref"][out]).max().item() for r in runs]
            for seed, r in enumerate(runs):
                ref, emul = r["ref"][out], r["emul"][dt][out]
                assert ref.dtype == torch.float64 and emul.shape == ref.shape and torch.isfinite(ref).all()
                assert S.holds(S.conditions(name, dt, emul, ref, emul)) == {"e": True, "pix": True, "ch": True}
                assert pix[seed] <= max(1e-3, m_pix * min(pix)), (out, seed, "pixel")
                assert ch[seed] <= max(1e-3, m_ch * min(ch)), (out, seed, "channel")


def test_margins_are_deterministic_and_committed():
    name = "R320_640"                                # its raw ratios lie mid-way between two-digit steps
    a = S.seed_stats(name)
    S._SEEDS.pop(name)                               # a FRESH measurement, not the cached one
    assert S.seed_stats(name) == a                   # the raw per-seed statistics included
    margins, pools = S.measure_margins([name])
    assert margins[name] == S.MARGINS[name] and pools[name] == S.POOL[name]
    assert set(S.MARGINS) == set(S.CASES) == set(S.POOL)
    assert all(p in (1, 16) for p in S.POOL.values())
    for n, per in S.MARGINS.items():                 # a pixel margin above 2 would have pooled the case
        assert set(per) == set(DTYPE_IDS) and all(1.0 < v <= 2.0 for pair in per.values() for v in pair), n


def test_narrow_outputs_measure_a_pixel_against_the_typical_pixel():
    g = torch.Generator().manual_seed(0)
    ref = torch.randn((40, 3), generator=g, dtype=torch.float64)
    ref[7] = 1e-9                                    # a pixel whose own norm is next to nothing
    y = ref.clone()
    y[7] += 1e-6
    y[20, 1] += 0.3
    e = S.e_pix(y, ref)
    scale = (3 * (ref ** 2).mean()).sqrt()
    assert e.shape == (40,) and e[7] < 1e-5 and abs(e[20].item() - 0.3 / scale.item()) < 1e-12
    assert int(e.argmax()) == 20
    e16 = S.e_pix(y, ref, 16)
    assert e16.shape == (3,) and abs(e16[1].item() - 0.3 / (4 * scale.item())) < 1e-12
    wide = torch.randn((40, 32), generator=g, dtype=torch.float64)
    assert torch.equal(S.e_pix(wide * 1.01, wide), S.e_tok(wide * 1.01, wide))
    assert S.where("DB640", "skip2", 23) == (1, 0, 3) and S.where("VDEC", "out", 3, 16) == (0, 1, 8)


# ---- 2. planted faults -------------------------------------------------------------------------------------------------
def _hooked(name, ora, inp, module, pre=None, post=None):
    hs = [module.register_forward_pre_hook(pre)] if pre is not None else []
    hs += [module.register_forward_hook(post)] if post is not None else []
    try:
        return S.run_oracle(name, ora, inp)
    finally:
        for h in hs:
            h.remove()


def fault_instance_bleed(name, ora, inp, ref):
    """conv2's tap above pixel (instance 1, row 0, col 0) reads instance 0's last row instead of the zero pad."""
    got = []
    _hooked(name, ora, inp, ora.conv2, pre=lambda _m, a: got.append(a[0]))
    a = got[0]
    h, w = a.shape[2:]
    y = {k: v.clone() for k, v in ref.items()}
    for v in y.values():
        v[h * w] += ora.conv2.weight[:, :, 0, 1] @ a[0, :, h - 1, 0]
    return y


def fault_pad0_wrong_side(name, ora, inp, ref):
    """the pad=0 downsample padded (1, 0, 1, 0) instead of (0, 1, 0, 1)."""
    return _hooked(name, ora, inp, ora.downsamplers[0].conv, pre=lambda _m, a: (F.pad(a[0][..., :-1, :-1], (1, 0, 1, 0)),))


def fault_nearest_last_column(name, ora, inp, ref):
    """the nearest map of 4 x 7 -> 7 x 13 off by one in its last column: it reads source column 5, not 6."""
    win, wout = S.CASES[name]["hw"][1], S.CASES[name]["up_size"][1]
    src = [j * win // wout for j in range(wout)]
    twin = src.index(src[-1] - 1)                    # an output column that does read the neighbouring source column

    def pre(_m, a):
        u = a[0].clone()
        assert u.shape[-1] == wout
        u[..., -1] = u[..., twin]
        return (u,)
    return _hooked(name, ora, inp, ora.upsamplers[0].conv, pre=pre)


def fault_time_vector_of_neighbour(name, ora, inp, ref):
    """instance 1's time vector used for instance 2."""
    emb = inp["emb"].clone()
    emb[2] = emb[1]
    return S.run_oracle(name, ora, dict(inp, emb=emb))


def fault_concat_order(name, ora, inp, ref):
    """the concat order [skip, h]."""
    return S.run_oracle(name, ora, dict(inp, x=inp["x2"], x2=inp["x"]))


def fault_skip_wrong_end(name, ora, inp, ref):
    """the first resnet's skip popped from the wrong end: the skips are consumed as (0, 2, 1), not (2, 1, 0)."""
    s = inp["skips"]
    return S.run_oracle(name, ora, dict(inp, skips=[s[1], s[2], s[0]]))


def fault_view_rows_shifted(name, ora, inp, ref):
    """view 0's attention output written to view 1's rows."""
    def post(_m, a, out):
        x, o = a[0], out.clone()
        o[1] = x[1] + (out[0] - x[0])
        return o
    return _hooked(name, ora, inp, ora.attentions[0], post=post)


FAULTS = {
    "instance_bleed": ("R320_640", fault_instance_bleed),
    "pad0_wrong_side": ("VDOWN128_256", fault_pad0_wrong_side),
    "nearest_last_column": ("UB1280", fault_nearest_last_column),
    "time_vector_of_neighbour": ("R320", fault_time_vector_of_neighbour),
    "concat_order": ("Rcat960", fault_concat_order),
    "skip_wrong_end": ("UB1280", fault_skip_wrong_end),
    "view_rows_shifted": ("VMID", fault_view_rows_shifted),
}
# Which faults the whole-tensor condition lets through at the case's own m x h x w (fp16, bf16): none — on outputs of 56 to
# 182 pixels even one wrong pixel is 1 / sqrt(pixels) of the tensor.  test_workload_sized_output is where it stops seeing.
WHOLE_PASSES = {f: (False, False) for f in FAULTS}


def faulty_outputs(oracle, fault):
    name, fn = FAULTS[fault]
    ora, inp, o = oracle(name)
    bad = fn(name, ora, inp, o["ref"])
    return name, o, {dt: {k: o["emul"][dt][k].double() + (bad[k] - o["ref"][k]) for k in bad} for dt in S.DTYPES}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_fault_fails_the_pixel_or_channel_condition(oracle, fault):
    name, o, ys = faulty_outputs(oracle, fault)
    whole = []
    for dt in S.DTYPES:
        cond = S.conditions(name, dt, ys[dt]["out"], o["ref"]["out"], o["emul"][dt]["out"])
        print("[spatial fault] %-24s %-12s %-8s " % (fault, name, S.tag(dt))
              + " ".join("%s=%.2e/%.2e (%.1f x)" % (k, v, b, v / b) for k, (v, b) in cond.items()))
        got = S.holds(cond)
        assert not (got["pix"] and got["ch"]), (fault, S.tag(dt), cond)
        assert cond["pix"][0] > 2 * cond["pix"][1] or cond["ch"][0] > 2 * cond["ch"][1]      # and not by a hair
        whole.append(got["e"])
    assert tuple(whole) == WHOLE_PASSES[fault]


def test_fault_is_named_where_it_was_planted(oracle):
    name, o, ys = faulty_outputs(oracle, "instance_bleed")
    for dt in S.DTYPES:
        row = int(S.e_pix(ys[dt]["out"], o["ref"]["out"]).argmax())
        assert S.where(name, "out", row) == (1, 0, 0)
    name, o, ys = faulty_outputs(oracle, "time_vector_of_neighbour")
    for dt in S.DTYPES:
        assert S.where(name, "out", int(S.e_pix(ys[dt]["out"], o["ref"]["out"]).argmax()))[0] == 2


@pytest.mark.parametrize("instances", [12, 48])
@pytest.mark.parametrize("dtype", S.DTYPES, ids=DTYPE_IDS)
def test_workload_sized_output(oracle, dtype, instances):
    """The gap: R320_640's own tensors repeated to the workload's 12 x 28 x 50 = 16800 pixels, and to the 48 instances of
    the video network (which leaves e(emul) and the per-pixel statistics as they are), the bleed planted in ONE copy."""
    name, o, ys = faulty_outputs(oracle, "instance_bleed")
    ref, emul, y = o["ref"]["out"], o["emul"][dtype]["out"], ys[dtype]["out"]
    pixels = instances * 28 * 50
    rep = pixels // ref.shape[0]
    assert rep * ref.shape[0] == pixels
    big_ref, big_emul = ref.repeat(rep, 1), emul.repeat(rep, 1)
    big_y = big_emul.double().clone()
    big_y[:ref.shape[0]] = y
    assert S.holds(S.conditions(name, dtype, big_emul, big_ref, big_emul)) == {"e": True, "pix": True, "ch": True}
    cond = S.conditions(name, dtype, big_y, big_ref, big_emul)
    print("[spatial fault] instance_bleed at %d pixels %-8s " % (pixels, S.tag(dtype))
          + " ".join("%s=%.2e/%.2e (%.2f x)" % (k, v, b, v / b) for k, (v, b) in cond.items()))
    assert cond["pix"][0] > 30 * cond["pix"][1], "the pixel condition is 30 x over"
    if instances == 12:
        assert cond["e"][0] < 1.5 * cond["e"][1], "the whole-tensor number sits on its bound"
    else:
        assert cond["e"][0] <= 1.01 * cond["e"][1], "the whole-tensor number is inside its bound, or within 1 % of it"


# ---- 3. the table --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.CASES))
def test_case_constructs_on_both_sides(oracle, name):
    _ora, _inp, o = oracle(name)
    hip = S.build_hip(name)
    assert set(hip.state_dict()) == set(o["sd"])
    assert {k: tuple(v.shape) for k, v in hip.state_dict().items()} == {k: tuple(v.shape) for k, v in o["sd"].items()}
    hip.load_state_dict(o["sd"], strict=True)
    assert list(o["ref"]) == S.outputs_of(name) == list(S.out_hw(name))
    for out, (m, h, w) in S.out_hw(name).items():
        assert o["ref"][out].shape[0] == m * h * w and o["ref"][out].dtype == torch.float64
        for dt in S.DTYPES:
            assert o["emul"][dt][out].shape == o["ref"][out].shape


def test_expected_counts_of_the_documented_paths():
    """test_spatial_blocks_gpu.expected at points worked out by hand from layers.py / vae_decoder.py / vae_encoder.py."""
    d, fused, f16 = dict(DEFAULTS), (lambda hw, c: True), torch.float16
    e = expected("R320", f16, d, fused)              # two runs of: norm1, conv1, norm2, conv2; one bank GEMM; no shortcut
    assert (e["conv3x3"], e["groupnorm"], e["gemm"], e["conv.rowvec"], e["conv.res"], e["conv.gn_next"]) == (4, 4, 1, 2, 2, 2)
    e = expected("Rcat960", f16, d, fused)           # the shortcut and norm1 read two sources
    assert (e["gemm"], e["gemm.a2"], e["groupnorm.x2"]) == (3, 2, 2)
    e = expected("DB640", f16, dict(d, GN_SPLITK=True), fused)     # conv1 -> norm2 and conv2 -> transformer norm, per layer
    assert (e["gn_splitk"], e["conv.gn_cache"], e["groupnorm"], e["conv.stride2"]) == (4, 4, 2, 1)
    assert expected("DB640", f16, dict(d, GN_SPLITK=True), lambda hw, c: False)["groupnorm"] == 6
    e = expected("UB1280", f16, d, fused)            # no row of the upfold table at 4 x 7 -> 7 x 13
    assert (e["conv.up"], e["conv.upfold"], e["gemm.a2"], e["groupnorm.x2"]) == (1, 0, 3, 3)
    assert expected("CUB640", f16, d, fused)["conv.upfold"] == 1 and expected("CUB640", torch.bfloat16, d, fused)["conv.upfold"] == 0
    assert expected("CUB640", f16, dict(d, fold_upsample=False), fused)["conv.upfold"] == 0
    e = expected("VMID", f16, d, fused)              # Q|K GEMM + 4 per view; three norms of the attention and resnets
    assert (e["gemm"], e["groupnorm"], e["conv3x3"]) == (9, 5, 4)
    e = expected("VDEC", f16, d, fused)
    assert (e["conv3x3"], e["conv.up"], e["small_cout"], e["groupnorm"]) == (1 + 4 + 24 + 3, 3, 1, 2 * 14 + 1 + 1)
    e = expected("VENC", f16, d, fused)
    assert (e["conv3x3"], e["conv.pad0"], e["conv.stride2"]) == (1 + 16 + 3 + 4 + 1, 3, 3)
    assert len(MATRIX) == 2 * (len(S.CASES) + len(APPLIES["gn_splitk"]) + len(APPLIES["no_upfold"]))
    assert APPLIES["gn_splitk"] == ["R320", "R320_640", "Rcat960", "Rcat2560", "DB640", "DB1280", "MID", "UB1280", "CUB640"]
