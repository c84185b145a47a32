"""The small HIP kernels (csrc/elementwise.hip, csrc/vae.hip, the layout kernel of csrc/tokens.hip) per element against the
fp64 references and bounds of small_ops_reference.py, in fp16 and bf16.

Shapes are the smallest at which each kernel takes another path: the grid-stride kernels run at one vector, at one
partial block and at 2048 blocks + 37 (a second trip of the loop with a ragged tail: `grid_for` caps the grid at 2048
blocks); the wave-per-row / wave-per-pixel kernels around 64 columns and with idle waves in the last block; the thin
conv below one 16-pixel group, at exactly one 64-pixel tile and one column past it, with partial tiles in both
directions.  Outputs are pre-filled with NaN wherever the wrapper takes `out=`.  Each test prints one `[small fp64]`
line with the number of launches compared and the worst error / bound, and passes at <= 1: for the kernels held to
"as close as the correct rounding" the error is what |y - ref| exceeds that of the correct rounding by and the bound is
E; for the convolutions it is gemm_reference.check's |y - ref| / (ulp + E)."""
import ctypes

import pytest
import torch

from tests import gemm_reference as G
from tests import small_ops_reference as S

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
_TN = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}
DEV = "cuda"
TWO_TRIPS = 2048 * 256 + 37                   # work items: the grid is capped at 2048 blocks of 256


@pytest.fixture(scope="module")
def ops(gpu):
    from dualdiff_amd import ops as O
    return O


def rnd(shape, dtype, seed, scale=1.0):
    return G.rand(shape, dtype, seed, scale, device=DEV)


def rnd_dev(shape, dtype, seed, scale=1.0):
    return G.rand_dev(shape, dtype, seed, scale, device=DEV)


def nan(shape, dtype):
    return G.nan_like(tuple(shape), dtype, DEV)


def report(family, dtype, ratios, extra=""):
    print("[small fp64] %-24s %-9s launches %4d   max err/bound %.3f%s"
          % (family, dtype if isinstance(dtype, str) else _TN[dtype], len(ratios), max(ratios), extra))
    assert max(ratios) <= 1.0


# ---- add, scale, silu -----------------------------------------------------------------------------------------------------

SCALES = [0.37, 0.18215, 1 / 0.18215, 0.125, -1.0, 0.0]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [8, 8 * 255, 8 * TWO_TRIPS])
def test_add_scale_silu(ops, dtype, n):
    fam = {"add2": [], "add3": [], "scale": [], "silu": []}
    for k, kind in enumerate(S.ADD_KINDS):
        a, b, c = S.add_operands(kind, k, n, dtype, rnd_dev)
        what = "n=%d %s" % (n, kind)
        fam["add2"].append(S.closest(ops.add(a, b, out=nan((n,), dtype)), *S.add_ref(a, b), "add2 " + what))
        fam["add3"].append(S.closest(ops.add(a, b, c, out=nan((n,), dtype)), *S.add_ref(a, b, c), "add3 " + what))
        for s in SCALES:
            fam["scale"].append(S.closest(ops.scale(a, s, out=nan((n,), dtype)), *S.scale_ref(a, s), "scale %g %s" % (s, what)))
        fam["silu"].append(S.closest(ops.silu(a, out=nan((n,), dtype)), *S.silu_ref(a), "silu " + what))
    for name, ratios in fam.items():
        report("%s n=%d" % (name, n), dtype, ratios)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_scale_silu_every_finite_value(ops, dtype):
    x = S.finite_patterns(dtype, DEV)
    n = x.numel()
    ratios = [S.closest(ops.scale(x, s, out=nan((n,), dtype)), *S.scale_ref(x, s), "scale %g, every value" % s) for s in SCALES]
    report("scale every value", dtype, ratios)
    report("silu every value", dtype, [S.closest(ops.silu(x, out=nan((n,), dtype)), *S.silu_ref(x), "silu, every value")])


# ---- layout converts: exact copies ----------------------------------------------------------------------------------------

LAYOUTS = [(1, 4, 1, 1, 8), (3, 3, 5, 7, 8), (2, 4, 28, 50, 4), (2, 5, 3, 3, 6), (2, 100, 9, 13, 104), (2, 320, 7, 9, 320)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_layout_converts_are_exact(ops, dtype):
    for i, (m, c, h, w, c_pad) in enumerate(LAYOUTS):
        x = rnd((m, c, h, w), dtype, 30 + i)
        y = ops.nchw_to_nhwc(x, c_pad)
        assert torch.equal(y, S.nhwc_ref(x, c_pad)), (m, c, h, w, c_pad)
        assert torch.equal(ops.nhwc_to_nchw(y, m, c, h, w), x), (m, c, h, w, c_pad)          # ldx = c_pad
        wide = rnd((m * h * w, c + 24), dtype, 40 + i)                                    # a column slice: ldx > c
        cols = wide[:, 8:8 + c]
        assert torch.equal(ops.nhwc_to_nchw(cols, m, c, h, w), S.nchw_ref(cols, m, c, h, w)), (m, c, h, w)
    pano = rnd((2, 3, 6, 3 * 11), dtype, 50)
    assert torch.equal(ops.nchw_to_nhwc(pano, 8, views=3), S.nhwc_ref(pano, 8, views=3))
    print("[small fp64] %-24s %-9s launches %4d   bit-equal" % ("nchw<->nhwc", _TN[dtype], 3 * len(LAYOUTS) + 1))


# ---- embeddings -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_timestep_embedding(ops, dtype):
    t5 = torch.tensor([0.0, 1.0, 500.5, 981.0, 999.0], device=DEV)
    ratios = []
    for dim in (2, 6, 320, 1280):
        for flip in (True, False):
            for shift in (0.0, 1.0):
                if dim == 2 and shift == 1.0:
                    continue                                  # half - shift = 0
                for t in (t5, t5[3:4]):
                    y = ops.timestep_embedding(t, dim, dtype, flip, shift, out=nan((t.numel(), dim), dtype))
                    ref, e = S.timestep_ref(t, dim, flip, shift)
                    ratios.append(S.closest(y, ref, e, "timestep dim=%d flip=%d shift=%g n=%d" % (dim, flip, shift, t.numel())))
    report("timestep_embedding", dtype, ratios)


FOURIER = [((12, 6, 7, 3), 4, True), ((60, 8, 3), 4, True), ((5, 3), 8, False), ((40, 1), 4, True), ((7, 3), 16, True)]


def _fourier(ops, x, freqs, inc, out_dtype):
    # ops.fourier_embed hands the launcher the input's type for both sides; the six mixed in / out pairs (camera and box
    # features are read in one type and written in another) are only reachable through the C entry point itself
    from dualdiff_amd import _native
    dims = x.shape[-1]
    out = nan(tuple(x.shape[:-1]) + (dims * (int(inc) + 2 * len(freqs)),), out_dtype)
    arr = (ctypes.c_float * len(freqs))(*freqs)
    _native.check(_native.load().dd_fourier_embed(ops._ptr(x), ops._ptr(out), x.numel() // dims, dims, arr, len(freqs), int(inc),
                                                  ops._FDT[x.dtype], ops._FDT[out_dtype], ops._stream()), "fourier_embed")
    return out


@pytest.mark.parametrize("tout", [torch.float32] + DTYPES, ids=["to_f32", "to_f16", "to_bf16"])
@pytest.mark.parametrize("tin", [torch.float32] + DTYPES, ids=["f32", "f16", "bf16"])
def test_fourier_embed(ops, tin, tout):
    ratios = []
    for i, (shape, nf, inc) in enumerate(FOURIER):
        x = (rnd(shape, torch.float32, 60 + i) * 30.0).to(tin)
        freqs = [2.0 ** k for k in range(nf)]
        y = _fourier(ops, x, freqs, inc, tout)
        ref, e = S.fourier_ref(x, freqs, inc)
        ratios.append(S.closest(y, ref, e, "fourier %s nf=%d inc=%d" % (shape, nf, inc)))
        if tin == tout:
            assert torch.equal(ops.fourier_embed(x, freqs, inc), y)
    report("fourier_embed", "%s->%s" % (_TN[tin], _TN[tout]), ratios)


# ---- softmax rows ---------------------------------------------------------------------------------------------------------

SOFTMAX_KINDS = ["randn", "randn x 30", "spike", "constant", "offset 1e4", "-inf entries"]


def _logits(kind, rows, cols, seed):
    """A (rows, cols) column slice of a NaN-filled wider fp32 matrix (lds > cols; an over-read would poison the row)."""
    s = rnd((rows, cols), torch.float32, seed, 30.0 if kind == "randn x 30" else 1.0)
    r = torch.arange(rows, device=DEV)
    if kind == "spike":
        s[r, (7 * r + 3) % cols] += 80.0
    elif kind == "constant":
        s[:] = (0.25 * r.float() - 3.0)[:, None]
    elif kind == "offset 1e4":
        s += 1e4
    elif kind == "-inf entries":
        keep = s[:, cols - 1].clone()
        s[:, ::3] = float("-inf")
        s[:, cols - 1] = keep                                 # at least one finite entry per row
    wide = torch.full((rows, cols + 40), float("nan"), dtype=torch.float32, device=DEV)
    wide[:, 16:16 + cols] = s
    return wide[:, 16:16 + cols]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", SOFTMAX_KINDS)
def test_softmax_rows(ops, dtype, kind):
    ratios = []
    for rows in (1, 5, 203):
        for cols in (1, 63, 64, 65, 203, 1400):
            s = _logits(kind, rows, cols, 70 + cols)
            assert s.stride(0) > cols
            p = ops.softmax_rows(s, dtype, pad_to=8)
            ldp = (cols + 7) // 8 * 8
            assert p.shape == (rows, ldp) and p.dtype == dtype
            assert bool((p[:, cols:] == 0).all()), "padding columns are not zero"
            ratios.append(S.closest(p[:, :cols], *S.softmax_ref(s), "softmax %s %dx%d" % (kind, rows, cols)))
    report("softmax_rows " + kind, dtype, ratios)


# ---- convolutions ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cin,cout", [(8, 1), (128, 3), (320, 4), (320, 8), (512, 3)])
def test_conv3x3_small_cout(ops, dtype, cin, cout):
    ratios = []
    for i, (m, h, w) in enumerate([(1, 1, 1), (1, 1, 7), (3, 3, 2), (2, 28, 50)]):
        x = rnd((m * h * w, cin), dtype, 80 + i)
        wt = rnd((cout, 9 * cin), dtype, 90 + i, (9 * cin) ** -0.5)
        for b in (rnd((cout,), dtype, 95 + i), None):
            y = ops.conv3x3_small_cout(x, wt, b, m, h, w, out=nan((m, cout, h, w), dtype))
            ref, e = S.conv_ref(x, wt, b, m, h, w)
            ratios.append(S.conv_check(y, S.to_nchw(ref, m, h, w), S.to_nchw(e, m, h, w),
                                       "conv_small %d->%d %dx%dx%d bias=%s" % (cin, cout, m, h, w, b is not None)))
    report("conv3x3_small %d->%d" % (cin, cout), dtype, ratios)


def test_conv3x3_small_cout_rejects_nine(ops):
    x = rnd((2 * 3 * 3, 64), torch.float16, 1)
    with pytest.raises(RuntimeError):
        ops.conv3x3_small_cout(x, rnd((9, 9 * 64), torch.float16, 2), None, 2, 3, 3)


THIN = [(8, 16, 1), (16, 16, 1), (16, 32, 2), (32, 32, 1), (8, 32, 1), (16, 32, 1), (16, 16, 2), (8, 16, 2), (32, 16, 1)]
THIN_IMAGES = {1: [(1, 1), (3, 15), (7, 64), (9, 65), (8, 17)], 2: [(1, 1), (2, 33), (7, 127), (8, 128), (9, 129)]}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("cin,cout,stride", THIN)
def test_conv3x3_thin(ops, dtype, cin, cout, stride):
    m = 2
    assert ops.thin_conv_ok(cin, cout, stride, m)
    ratios = []
    for i, (h, w) in enumerate(THIN_IMAGES[stride]):
        x = rnd((m * h * w, cin), dtype, 100 + i)              # cin = 8: all eight channels carry data
        wt = rnd((cout, 9 * cin), dtype, 110 + i, (9 * cin) ** -0.5)
        ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        for b in (rnd((cout,), dtype, 115 + i), None):
            for silu in (False, True):
                y = ops.conv3x3(x, wt, b, m, h, w, stride=stride, epilogue=ops.DD_EPI_SILU if silu else ops.DD_EPI_NONE,
                                out=nan((m * ho * wo, cout), dtype))
                ref, e = S.conv_ref(x, wt, b, m, h, w, stride, silu)
                ratios.append(S.conv_check(y, ref, e, "thin %d->%d s%d %dx%d bias=%s silu=%s"
                                           % (cin, cout, stride, h, w, b is not None, silu)))
    report("conv3x3_thin %d->%d s%d" % (cin, cout, stride), dtype, ratios)


# ---- sampler steps --------------------------------------------------------------------------------------------------------

def _guided(eps, g, what):
    es, amb, fused = S.guided(eps, g)
    share = float(amb.double().mean())
    assert share <= S.MAX_AMBIGUOUS, "%s: %.3g of the guided-noise elements are ambiguous" % (what, share)
    return es, share, float(fused.double().mean())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", S.STEP_N)
def test_cfg_ddim_step(ops, dtype, n):
    from dualdiff_amd.pipeline.pipeline_bev_controlnet import ddim_schedule
    _, tab = ddim_schedule(50)
    x = S.step_x(n, dtype, DEV)
    ratios, shares, fused = [], [], []
    for g in S.STEP_G:
        eps = S.step_eps(n, dtype, g, 0, DEV)
        es, share, fshare = _guided(eps, g, "ddim n=%d g=%g" % (n, g))
        shares.append(share)
        fused.append(fshare)
        for row in (0, len(tab) // 2, len(tab) - 1):
            coef = tab[row].to(DEV)
            y = ops.cfg_ddim_step(eps, x, coef, g, x_out=nan((n,), dtype))
            ratios.append(S.closest_either([y], [[S.ddim_ref(x, e, tab[row])] for e in es], "ddim n=%d g=%g row %d" % (n, g, row)))
            y2, dup = nan((n,), dtype), nan((n,), dtype)
            ops.cfg_ddim_step(eps, x, coef, g, x_out=y2, x_dup=dup)
            assert torch.equal(dup, y2) and torch.equal(y2, y)
    report("cfg_ddim_step n=%d" % n, dtype, ratios, "   ambiguous <= %.2e, single rounding differs <= %.2e" % (max(shares), max(fused)))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", S.STEP_N)
def test_cfg_unipc_step(ops, dtype, n):
    """A whole 8-step run per guidance scale; the reference is re-seeded from the kernel's stored sample and history
    every step, and the sample, last, m1 and m2 are compared per element every step."""
    from dualdiff_amd.pipeline.schedulers import unipc_schedule
    _, tab = unipc_schedule(8)
    f32 = torch.float32
    ratios, shares, fused = [], [], []
    for g in S.STEP_G:
        x = S.step_x(n, dtype, DEV)
        hist = torch.zeros((3, n), dtype=f32, device=DEV)
        for i in range(len(tab)):
            eps = S.step_eps(n, dtype, g, i, DEV)
            es, share, fshare = _guided(eps, g, "unipc n=%d g=%g step %d" % (n, g, i))
            shares.append(share)
            fused.append(fshare)
            before = hist.clone()
            cands = [S.unipc_ref(x, e, before, tab[i]) for e in es]
            y = nan((n,), dtype)
            dup = nan((n,), dtype) if i % 2 else None
            ops.cfg_unipc_step(eps, x, hist, tab[i].to(DEV), g, x_out=y, x_dup=dup)
            if dup is not None:
                assert torch.equal(dup, y)
            ratios.append(S.closest_either([y, hist[0], hist[1], hist[2]], cands, "unipc n=%d g=%g step %d" % (n, g, i),
                                           [None, f32, f32, f32]))
            x = y
    report("cfg_unipc_step n=%d" % n, dtype, ratios, "   ambiguous <= %.2e, single rounding differs <= %.2e" % (max(shares), max(fused)))


# ---- VAE posterior --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_vae_posterior(ops, dtype):
    ratios = []
    wq = rnd((8, 8), torch.float32, 120)
    bq = rnd((8,), torch.float32, 121)
    bq[4] += 40.0                                             # logvar channel 0 above the upper clamp end (20) ...
    bq[5] -= 50.0                                             # ... channel 1 below the lower one (-30), 2 and 3 between them
    for i, (m, h, w) in enumerate([(1, 1, 1), (2, 3, 5), (1, 28, 50)]):
        mom = rnd((m * h * w, 8), dtype, 122 + i, 2.0)
        lv = (mom.double() @ wq.double().t() + bq.double())[:, 4:]
        assert bool((lv > 20).any()) and bool((lv < -30).any())
        assert bool(((lv > -30) & (lv < 20)).any())
        noise = rnd((m, 4, h, w), dtype, 126 + i)
        for nz in (None, noise):
            for out_f32 in (False, True):
                for scale in (1.0, 0.18215):
                    z = ops.vae_posterior(mom, wq, bq, m, h, w, noise=nz, scale=scale, out_f32=out_f32)
                    assert z.dtype == (torch.float32 if out_f32 else dtype)
                    ref, e = S.posterior_ref(mom, wq, bq, m, h, w, nz, scale)
                    ratios.append(S.closest(z, ref, e, "posterior %dx%dx%d %s f32=%s scale=%g"
                                            % (m, h, w, "mode" if nz is None else "sample", out_f32, scale)))
    report("vae_posterior", dtype, ratios)
