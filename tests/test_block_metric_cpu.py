"""The per-token / per-channel conditions of tests/block_cases.py see what the whole-tensor metric does not — shown on the
oracle's own tensors, without a GPU: y = emul[dtype] stands in for a correct output of a block; a corrupted copy of it
must fail the condition that is there to catch it.

The gap itself (`test_whole_tensor_metric_alone_misses_one_token`): one token row off by 5 % moves the whole-tensor
error of a (rows, C) output by 0.05 / sqrt(rows).  At the 56 .. 600 rows of the cases that is 2e-3 .. 7e-3 and condition
1 does see it; at a workload-sized output (12 x 700 = 8400 rows: 5.5e-4) it does not.  The test therefore states the gap
at 8400 rows, made of the largest case's own tensors repeated 14 times, which leaves e(emul) and the per-row statistics
of the uncorrupted tensors as they are."""
import pytest
import torch

from tests import block_cases as B
from tests.test_block_switches_gpu import DEFAULTS, MATRIX, expected

CASE_IDS = list(B.CASES)
DTYPE_IDS = [B.tag(dt) for dt in B.DTYPES]
LARGEST = max(B.CASES, key=lambda n: B.CASES[n][4] * (B.CASES[n][5] if B.CASES[n][0] == "MV" else
                                                      B.CASES[n][5][0] * B.CASES[n][5][1]))


@pytest.fixture(scope="module")
def oracle():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = B.oracle_outputs(name)
        return cache[name]
    return get


def _check(name, dtype, y, o):
    return B.holds(B.conditions(name, dtype, y, o["ref"], o["emul"][dtype]))


def test_largest_case_is_the_600_row_one():
    assert LARGEST == "MV320"


@pytest.mark.parametrize("dtype", B.DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("name", CASE_IDS)
def test_conditions_on_the_oracle(oracle, name, dtype):
    o = oracle(name)
    ref, emul = o["ref"], o["emul"][dtype]
    rows, c = ref.shape
    assert ref.dtype == torch.float64 and emul.shape == ref.shape and torch.isfinite(ref).all()
    assert B.e_tok(emul, ref).shape == (rows,) and B.e_ch(emul, ref).shape == (c,)
    # the stand-in for a correct output passes all three
    assert _check(name, dtype, emul, o) == {"e": True, "tok": True, "ch": True}
    # the exact output has no error at all
    assert B.e_tok(ref, ref).max().item() == 0.0 and B.e_ch(ref, ref).max().item() == 0.0

    r = rows - 3                                     # a row of the ragged tail of the last tile
    y = emul.clone()
    y[r] *= 1.05
    assert not _check(name, dtype, y, o)["tok"], "one token row scaled by 1.05"
    assert int(B.e_tok(y, ref, B.POOL[name]).argmax()) == r // B.POOL[name]        # and the metric says which one

    y = emul.clone()
    y[:, c // 2 + 1] *= 1.05
    assert not _check(name, dtype, y, o)["ch"], "one channel scaled by 1.05"
    assert int(B.e_ch(y, ref).argmax()) == c // 2 + 1

    y = emul.clone()
    y[[r, r + 1]] = y[[r + 1, r]]
    assert not _check(name, dtype, y, o)["tok"], "two adjacent token rows swapped"


@pytest.mark.parametrize("dtype", B.DTYPES, ids=DTYPE_IDS)
def test_whole_tensor_metric_alone_misses_one_token(oracle, dtype):
    o = oracle(LARGEST)
    rep = 8400 // o["ref"].shape[0]
    big = {"ref": o["ref"].repeat(rep, 1), "emul": {dtype: o["emul"][dtype].repeat(rep, 1)}}
    assert big["ref"].shape[0] == 8400
    y = big["emul"][dtype].clone()
    assert _check(LARGEST, dtype, y, big) == {"e": True, "tok": True, "ch": True}
    y[4321] *= 1.05
    got = _check(LARGEST, dtype, y, big)
    assert got["e"], "condition 1 alone still passes"
    assert not got["tok"], "condition 2 fails"


def test_pooled_rows():
    """POOL > 1 (a case whose per-row margin came out above 2): groups of 16 rows, a ragged last group kept."""
    g = torch.Generator().manual_seed(0)
    ref = torch.randn((40, 8), generator=g, dtype=torch.float64)
    y = ref.clone()
    y[35] *= 1.5
    e = B.e_tok(y, ref, 16)
    assert e.shape == (3,) and e[0] == 0 and e[1] == 0
    want = (0.25 * (ref[35] ** 2).sum() / (ref[32:] ** 2).sum()).sqrt()
    assert abs(e[2].item() - want.item()) < 1e-12


def test_round_up_to_two_significant_digits():
    assert [B.round_up_2sig(v) for v in (1.0, 1.001, 1.0671, 1.1, 1.91, 2.0001, 0.0123, 12.01)] == \
        [1.0, 1.1, 1.1, 1.1, 2.0, 2.1, 0.013, 13.0]


def test_margins_are_deterministic_and_committed():
    """Two measurements of the smallest case agree exactly, and with the committed table."""
    name = "T1280"
    a, b = B.measure_case(name), B.measure_case(name)
    assert a == b                                    # the raw per-seed statistics included
    margins, pools = B.measure_margins([name])
    assert margins[name] == B.MARGINS[name] and pools[name] == B.POOL[name]
    assert B.format_margins(margins, pools) == B.format_margins(*B.measure_margins([name]))
    for per in B.MARGINS.values():                   # every case keeps its rows apart unless the table says otherwise
        assert all(1.0 < m <= 2.0 for pair in per.values() for m in pair)
    assert set(B.MARGINS) == set(B.CASES) == set(B.POOL)


def test_expected_counts_of_the_documented_paths():
    """test_block_switches_gpu.expected at the points worked out by hand from layers.py / blocks.py."""
    d = dict(DEFAULTS)
    e = expected("T320", d)          # proj_in, attn1.to_out and dd_xattn320 each emit the next norm; the last GEMM has a2
    assert (e["xattn320"], e["layernorm"], e["gemm"], e["gemm.a2"], e["gemm.ln_out"], e["xattn320.ln_out"]) == (1, 0, 6, 1, 2, 1)
    assert expected("T320", dict(d, LN_PRODUCER=False))["layernorm"] == 3
    assert expected("T640", d)["layernorm"] == 3 and expected("T640", d)["gemm"] == 8
    e = expected("T320", dict(d, LN_FOLD="all"))        # Q|K|V, to_q and GEGLU carry ln=
    assert (e["xattn320"], e["layernorm"], e["gemm.ln"], e["gemm.ln_out"]) == (0, 0, 3, 0)
    e = expected("T320", dict(d, LN_FOLD="q"))          # to_q alone folds; norm1 and norm3 are launched
    assert (e["xattn320"], e["layernorm"], e["gemm.ln"]) == (0, 2, 1)
    e = expected("T1280", dict(d, LN_FOLD="stats"))
    assert (e["gemm.ln_stats"], e["gemm.ln"], e["gemm.stats_in"], e["layernorm"]) == (3, 3, 3, 0)
    e = expected("MV640", dict(d, LN_FOLD="stats"))     # nothing produced the block's input: norm1 is launched
    assert (e["gemm.ln_stats"], e["gemm.ln"], e["gemm.stats_in"], e["layernorm"]) == (3, 3, 3, 1)
    e = expected("MV320", dict(d, HEAD_MAJOR=False))
    assert (e["gemm.head_major"], e["attention.q_prescaled"], e["attention"], e["xattn320"]) == (0, 0, 2, 1)
    e = expected("T320", dict(d, fold_proj_out=False))
    assert (e["gemm.a2"], e["gemm"]) == (0, 7)
    e = expected("MV320", d)
    assert (e["gemm"], e["attention"], e["xattn320"], e["layernorm"], e["gemm.ln_out"], e["xattn320.ln_out"]) == (7, 2, 1, 1, 2, 1)
    assert len(MATRIX) == 3 * 2 * 10 + 2 * 2 * 9
