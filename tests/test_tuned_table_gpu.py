"""Replay of the tracked tile / split-K table (dualdiff_amd/tuned/gfx950.json) against fp64.

The run-time tuner keeps the FASTEST candidate that launched; nothing in it checks the result.  Here every tracked entry
is rebuilt into the call its key stands for and launched with exactly the entry's tile and split-K (no tuner lookup), and
the output is compared element by element with the fp64 reference and bound of gemm_reference.py.
  * `g` keys (rows, n, k, epilogue, dtype, a2, ln, *flags): bias unless the LayerNorm fold; `si`: the fold's input comes
    from an ln_stats=True GEMM; `hm`: the production head-major planes (the Q planes times D^-1/2 log2 e); `a2`: k1 from
    the up blocks' concat widths (tuned_table.a2_k1).
  * `c` keys (m, hin, win, cin, cout, stride, hv, wv, dtype): twice — bias only, and bias + time-embedding row vector +
    residual with alpha != 1 (the ResNet conv2 form).
Outputs are NaN-filled before the launch (accumulate: the old values), so a missed write fails."""
import collections
import ctypes
import time

import pytest
import torch

from dualdiff_amd import _native, ops
from tests.gemm_cases import ConvCase, DenseCase
from tests.tuned_table import a2_k1, desc_from_key, family, load_table

pytestmark = pytest.mark.gpu

_DT = {0: torch.float16, 1: torch.bfloat16}


def _dense_case(key, seed):
    rows, n, k, epi, dt, a2, ln = key[1:8]
    flags = key[8:]
    hm = flags[flags.index("hm") + 1] if "hm" in flags else None
    return DenseCase(rows, n, k, _DT[dt], seed, epilogue=epi, a2_k1=a2_k1(k) if a2 else None, ln=ln, si="si" in flags,
                     f32="f32" in flags, so="so" in flags, hm=hm, res="res" in flags, acc="acc" in flags)


def _conv_case(key, seed):
    m, hin, win, cin, cout, stride, hv, wv, dt = key[1:]
    return ConvCase(m, hin, win, cin, cout, stride, _DT[dt], seed, up=None if (hv, wv) == (hin, win) else (hv, wv))


@pytest.mark.parametrize("kind", ["g", "c"])
def test_tracked_table_entries_match_fp64(gpu, kind):
    lib = _native.load()
    entries = [(k, v) for k, v in load_table() if k[0] == kind]
    assert entries
    worst = collections.defaultdict(float)
    count = collections.Counter()
    failures = []
    t0 = time.time()
    for i, (key, (tile, split, _form)) in enumerate(entries):
        fam = family(lib.dd_gemm_kernel_name(ctypes.byref(desc_from_key(key, tile, split))).decode())
        case = None
        try:
            case = _dense_case(key, 1000 + 16 * i) if kind == "g" else _conv_case(key, 1000 + 16 * i)
            for form in ((None,) if kind == "g" else (False, True)):
                r = case.run(tile, split) if form is None else case.run(tile, split, full=form)
                worst[fam] = max(worst[fam], r)
                count[fam] += 1
        except AssertionError as ex:                  # a launch error is not collected: it ends the test at once
            failures.append("%r -> (%d, %d) [%s]: %s" % (key, tile, split, fam, str(ex).splitlines()[0]))
        del case
    torch.cuda.synchronize()
    print("\n[tuned table %s] %d entries, %d launches in %.1f s; per family launches / max err/bound: %s"
          % (kind, len(entries), sum(count.values()), time.time() - t0,
             {f: (count[f], round(worst[f], 3)) for f in sorted(count)}))
    assert not failures, "%d of %d tracked entries compute a wrong result:\n%s" % (len(failures), len(entries),
                                                                                 "\n".join(failures[:30]))


def test_rejected_call_is_not_cached(gpu):
    """A call no candidate can launch (the LayerNorm fold takes K in {320, 640, 1280} only) raises, and leaves no
    (0, 0, 0) entry behind for save_tuned() to write into the tracked table."""
    x = torch.randn(64, 512, device=gpu).to(torch.bfloat16)
    w = torch.randn(64, 512, device=gpu).to(torch.bfloat16)
    z = torch.zeros(64, device=gpu)
    key = ("g", 64, 64, 512, 0, _native.DD_BF16, False, True)
    with pytest.raises(RuntimeError):
        ops.gemm(x, w, None, ln=(z, z, 1e-5))
    assert key not in ops.tuned_table()
