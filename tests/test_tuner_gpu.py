"""The run-time tile / split-K tuner itself (dualdiff_amd.tuning.tune), on shapes the tracked table does not hold.

Every other GPU test either hits the table or names its tile, so nothing else notices a tuner that leaves the descriptor
pointing at its scratch output, caches under the wrong key, or times again on every call.  The shapes are the smallest
with a real choice: 96 x 64 x 512 has eight 64-wide K steps, so tune_candidates offers split-K 2 beside 1; the pad-0 conv
is the smallest legal image.  The results are held to the fp64 bound of gemm_reference.py."""
import pytest
import torch

from dualdiff_amd import _native, ops, tuning
from dualdiff_amd._native import DD_BF16
from tests.gemm_cases import DenseCase
from tests.test_vae_encoder_gpu import Pad0Case
from tests.tuned_table import desc_from_key

pytestmark = pytest.mark.gpu


@pytest.fixture
def timed(monkeypatch):
    """The (pad_lo, tile, split, iters) of every timing the tuner makes, with the tuner switched on and no challengers."""
    calls = []
    real = tuning._time_launch

    def spy(L, d, device, warm, tile, split, iters):
        calls.append((L.pad_lo, tile, split, iters))
        return real(L, d, device, warm, tile, split, iters)
    monkeypatch.setattr(tuning, "_time_launch", spy)
    monkeypatch.setattr(tuning, "_AUTOTUNE", True)
    monkeypatch.setattr(ops, "CHALLENGE_TILES", ())
    tuning._load_default_table()
    return calls


def test_dense_shape_is_tuned_once_and_computes_fp64(gpu, timed):
    key = tuning.gemm_key(96, 64, 512, 0, DD_BF16)
    assert key not in ops.tuned_table()
    case = DenseCase(96, 64, 512, torch.bfloat16, 4242)
    before = set(ops.tuned_table())
    try:
        worst = case.run(0, 0)                 # out / ldc / accumulate / tile / split_k / ws restored after the timing
        row = ops.tuned_table()[key]
        cands = ops.tune_candidates(_native.load(), desc_from_key(key, 0, 0))
        assert any(s == 2 for _, s in cands)                  # 512 / 64 = 8 K steps: two slabs of 4
        assert row[:2] in cands and row[2] == 0, row
        assert set(ops.tuned_table()) - before == {key}
        n = len(timed)
        assert n >= len(cands) and all(c[0] == 1 for c in timed)
        worst = max(worst, case.run(0, 0))
        assert len(timed) == n, "a shape the table holds was timed again"
        assert ops.tuned_table()[key] == row
        print("\n[tuner] %r -> %r after %d timings; max err/bound %.3f" % (key, row, n, worst))
    finally:
        tuning._TUNED.pop(key, None)           # (the DD_SAVE_TUNED session hook must not see a test shape)
    assert key not in ops.tuned_table()


def test_pad0_conv_is_tuned_under_its_own_key(gpu, timed):
    shape = (1, 4, 4, 64, 64, 2, 4, 4, DD_BF16)
    key, pad1 = tuning.conv_pad0_key(*shape), tuning.conv_key(*shape)
    assert key[-1] == "p0" and key not in ops.tuned_table()
    had_pad1 = pad1 in ops.tuned_table()
    case = Pad0Case(1, 4, 4, 64, 64, torch.bfloat16, 4243)
    before = set(ops.tuned_table())
    try:
        worst = case.run()
        row = ops.tuned_table()[key]
        assert row[0] > 0 and row[1] >= 1 and row[2] == 0, row
        assert set(ops.tuned_table()) - before == {key} and (pad1 in ops.tuned_table()) == had_pad1
        n = len(timed)
        assert n > 0 and all(c[0] == 0 for c in timed), "the pad-0 conv was timed through another launch than its own"
        worst = max(worst, case.run())
        assert len(timed) == n, "a shape the table holds was timed again"
        print("\n[tuner] %r -> %r after %d timings; max err/bound %.3f" % (key, row, n, worst))
    finally:
        tuning._TUNED.pop(key, None)
    assert key not in ops.tuned_table()
