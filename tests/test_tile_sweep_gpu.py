"""Every (tile, split-K) the run-time tuner may pick, at off-table edge shapes, against fp64.

A retune, a shape met at run time (another resolution, a capacity bucket) or a new tile can install any candidate the
tuner times (ops.tune_candidates).  Here each of them is launched at shapes where tiled kernels go wrong — one row, less
than a tile, ragged edges, N % 64 != 0, K % 64 != 0, K shorter than the rings, deep K with uneven split-K slabs,
persistent walks, ragged conv instance counts, the band conv, stride 2, upsample, Cin % 64 != 0 — and compared with the
fp64 reference and bound of gemm_reference.py.  A pair the planner turns down (dd_gemm_kernel_name: "unsupported") is
skipped; any launch error after that is a failure.  The "bias" form of each dense shape (and the bias-only form of each
conv) runs through strided views: A's pad columns hold NaN, the output's a sentinel that must survive.

The byte-extent cases straddle dma_ok's 2^30-element limit and the 2^31-byte limit of the buffer-descriptor epilogue and
the persistent pipelined walk: rows * 320 elements / rows * 640 bytes at rows = 3 355 443 and 3 355 444."""
import collections
import ctypes
import time

import pytest
import torch

from dualdiff_amd import _native, ops
from tests.gemm_cases import ConvCase, DenseCase, sample_rows
from tests.tuned_table import desc_from_key, family

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
_DTC = {torch.float16: _native.DD_F16, torch.bfloat16: _native.DD_BF16}

DENSE = [(1, 320, 1280), (37, 72, 192), (333, 328, 640), (1093, 1288, 1344), (50001, 328, 640), (336, 1280, 5760),
         (200, 320, 200), (4200, 640, 128)]
# (m, hin, win, cin, cout, stride, upsample to)
CONV = [(5, 4, 7, 128, 192, 1, None), (13, 2, 3, 64, 64, 1, None), (2, 30, 41, 64, 72, 1, None),
        (3, 14, 25, 640, 640, 2, None), (2, 4, 7, 1280, 640, 1, (7, 13)), (1, 28, 50, 96, 256, 2, None),
        (4, 7, 13, 2560, 1280, 1, None)]


class Tally:
    def __init__(self):
        self.worst = collections.defaultdict(float)
        self.count = collections.Counter()
        self.failures = []
        self.t0 = time.time()

    def run(self, lib, case, key, tile, split, **plan_kw):
        """Launch one accepted candidate; returns False when the planner turns it down."""
        return self.run_fn(lib, lambda: case.run(tile, split), key, tile, split, **plan_kw)

    def run_fn(self, lib, fn, key, tile, split, **plan_kw):
        plan = lib.dd_gemm_kernel_name(ctypes.byref(desc_from_key(key, tile, split, **plan_kw))).decode()
        if plan == "unsupported":
            return False
        assert plan != "invalid", (key, tile, split, plan_kw)
        fam = family(plan)
        try:
            r = fn()
        except AssertionError as ex:
            self.failures.append("[%s] %s" % (fam, str(ex).splitlines()[0]))
            return True
        self.worst[fam] = max(self.worst[fam], r)
        self.count[fam] += 1
        return True

    def report(self, what):
        torch.cuda.synchronize()
        print("\n[%s] %d launches in %.1f s; per family launches / max err/bound: %s"
              % (what, sum(self.count.values()), time.time() - self.t0,
                 {f: (self.count[f], round(self.worst[f], 3)) for f in sorted(self.count)}))
        assert not self.failures, "%d launches outside the bound:\n%s" % (len(self.failures), "\n".join(self.failures[:30]))


def _candidates(lib, rows, n, k, epilogue=ops.DD_EPI_NONE):
    d = _native.GemmDesc()
    d.rows, d.n, d.k, d.epilogue = rows, n, k, epilogue
    return ops.tune_candidates(lib, d)


def _gkey(rows, n, k, dtype, epi=0, a2=False, ln=False, *flags):
    return ("g", rows, n, k, epi, _DTC[dtype], a2, ln) + tuple(flags)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", DENSE, ids=["%dx%dx%d" % s for s in DENSE])
def test_dense_tile_split_sweep(gpu, shape, dtype):
    lib = _native.load()
    rows, n, k = shape
    seed = rows + 7 * n + 13 * k
    cands = _candidates(lib, rows, n, k)
    tiles = sorted({t for t, _ in cands})
    t = Tally()
    # every candidate split: bias (strided A and output), and bias + row vector + alpha + residual
    case = DenseCase(rows, n, k, dtype, seed, strided=True)
    for tile, split in cands:
        t.run(lib, case, _gkey(rows, n, k, dtype), tile, split, lda=k + 64, ldc=n + 64)
    case = DenseCase(rows, n, k, dtype, seed + 1, rowvec=True, alpha=0.7, res=True)
    accepted = collections.defaultdict(list)
    for tile, split in cands:
        if t.run(lib, case, _gkey(rows, n, k, dtype, 0, False, False, "res"), tile, split, rowvec=True):
            accepted[tile].append(split)
    # split 1 and the largest accepted split: SiLU + residual, accumulate
    for kw, key in ((dict(epilogue=ops.DD_EPI_SILU, res=True), _gkey(rows, n, k, dtype, 2, False, False, "res")),
                    (dict(acc=True), _gkey(rows, n, k, dtype, 0, False, False, "acc"))):
        case = DenseCase(rows, n, k, dtype, seed + 2, **kw)
        for tile in tiles:
            for split in sorted({1, max(accepted[tile] or [1])}):
                t.run(lib, case, key, tile, split)
    # split 1 only: two sources (k1 a multiple of 64 and not), GEGLU, head-major, fp32 output, row statistics, LN fold
    k1a = 64 * max(1, k // 128)
    variants = [(dict(a2_k1=k1a), _gkey(rows, n, k, dtype, 0, True), dict(k1=k1a)),
                (dict(a2_k1=k1a + 24), _gkey(rows, n, k, dtype, 0, True), dict(k1=k1a + 24)),
                (dict(epilogue=ops.DD_EPI_GEGLU), _gkey(rows, n, k, dtype, 1), {}),
                (dict(f32=True), _gkey(rows, n, k, dtype, 0, False, False, "f32"), {})]
    if k1a + 24 >= k:
        variants.pop(1)
    hd = next(d for d in (80, 40, 8) if n % d == 0)
    variants.append((dict(hm=hd), _gkey(rows, n, k, dtype, 0, False, False, "hm", hd), {}))
    if n % 32 == 0:
        variants.append((dict(so=True, res=True), _gkey(rows, n, k, dtype, 0, False, False, "so", "res"), {}))
    if k in (320, 640, 1280):
        variants.append((dict(ln=True), _gkey(rows, n, k, dtype, 0, False, True), {}))
    for i, (kw, key, plan_kw) in enumerate(variants):
        case = DenseCase(rows, n, k, dtype, seed + 3 + i, **kw)
        for tile in tiles:
            t.run(lib, case, key, tile, 1, **plan_kw)
    t.report("dense sweep %dx%dx%d %s" % (rows, n, k, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", CONV, ids=["%dx%dx%d_%dto%d_s%d%s" % (c[:6] + ("_up" if c[6] else "",)) for c in CONV])
def test_conv_tile_split_sweep(gpu, shape, dtype):
    lib = _native.load()
    m, hin, win, cin, cout, stride, up = shape
    case = ConvCase(m, hin, win, cin, cout, stride, dtype, m * 31 + cin + cout, up=up)
    hv, wv = up or (hin, win)
    key = ("c", m, hin, win, cin, cout, stride, hv, wv, _DTC[dtype])
    t = Tally()
    n_ok = 0
    for tile, split in _candidates(lib, case.rows, cout, 9 * cin):
        n_ok += t.run_fn(lib, lambda: case.run(tile, split, strided=True), key, tile, split, ldc=cout + 64)
        t.run_fn(lib, lambda: case.run(tile, split, full=True), key, tile, split, rowvec=True)
    assert n_ok > 0
    t.report("conv sweep %s %s" % (shape, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [3355443, 3355444])
def test_byte_extent_edges(gpu, rows, dtype):
    """n = k = 320 at the row counts that straddle rows * lda < 2^30 (dma_ok: the LDS-DMA tiles fall back to their
    register-staged twins) and rows * 640 B < 2^31 (the buffer-descriptor epilogue and dd_gemm4's persistent walk switch
    off).  Compared on the last 4096 rows plus 4096 evenly spaced ones."""
    lib = _native.load()
    n = k = 320
    case = DenseCase(rows, n, k, dtype, rows % 1000, res=True, sample=sample_rows(rows))
    key = _gkey(rows, n, k, dtype, 0, False, False, "res")
    t = Tally()
    plans = {}
    for tile in (1, 52, 72, 75, 78):
        plans[tile] = lib.dd_gemm_kernel_name(ctypes.byref(desc_from_key(key, tile, 1))).decode().split(" split=")[0]
        assert t.run(lib, case, key, tile, 1), (tile, "unsupported")
    print("\n[byte extent %d rows] plans: %s" % (rows, plans))
    big = rows * k >= (1 << 30)
    assert plans[52].startswith("dd_gemm_kernel" if big else "dd_gemm2_kernel"), plans[52]
    t.report("byte extent %d rows %s" % (rows, dtype))
