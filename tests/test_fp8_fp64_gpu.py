"""The W8A8 projection path (csrc/gemm8.hip: dd_rowquant_fp8, dd_gemm8) per element against the fp64 references and
bounds of fp8_reference.py, in fp16 and bf16.

Shapes are the smallest at which the kernels take another path.  Row quantiser: the instantiation boundaries of
launch_rowquant (c = 512 / 520 and 1024 / 1032), its ends (8, 1536), blocks of four rows with idle waves (rows = 1, 3,
5, 9), and row pitches above the 128-rounded width, whose padding the extra trip of the store loop writes.  GEMM: rows
and channels one below, at and one above the 128 x 128 tile (64 gated channels with GEGLU), a vector of four channels,
one, two and three K steps (the single-step launch issues no second DMA), and the tile counts at which the XCD remap
changes branch.  Every output is pre-filled with NaN and, where the ABI takes a pitch, strided with a NaN pad that must
come back untouched; A8 is also handed in with lda > k_padded and NaN codes (0x7f) in the gap.  Each test prints one
`[fp8 fp64]` line with the number of launches compared and the worst error / bound, and passes at <= 1; the
quantiser's line also counts the bytes that differ from the fp32 recipe."""
import ctypes
import functools

import pytest
import torch

from tests import fp8_reference as R
from tests import gemm_reference as G
from tests import norm_reference as N

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["f16", "bf16"]
DEV = "cuda"
NAN = float("nan")
EPS = 1e-5


@pytest.fixture(scope="module")
def ops(gpu):
    from dualdiff_amd import ops as O
    return O


# ---- launches through the C entry points ----------------------------------------------------------------------------------

def rowquant_raw(ops, x, norm, ldq):
    """dd_rowquant_fp8 with a row pitch of its own, q filled with NaN codes and one guard row behind it, scale NaN."""
    from dualdiff_amd import _native
    rows, c = x.shape
    q = torch.full((rows + 1, ldq), R.NAN_CODE, dtype=torch.uint8, device=DEV)
    scale = torch.full((rows + 1,), NAN, dtype=torch.float32, device=DEV)
    g_, b_, eps = norm if norm is not None else (None, None, 0.0)
    _native.check(_native.load().dd_rowquant_fp8(ops._ptr(x), ops._ptr(g_), ops._ptr(b_), ops._ptr(q), ops._ptr(scale), rows, c,
                                                 ldq, float(eps), ops._dt(x), ops._stream()), "rowquant_fp8")
    assert bool((q[rows] == R.NAN_CODE).all()) and bool(torch.isnan(scale[rows])), "wrote past the last row"
    return q[:rows], scale[:rows]


def gemm8_raw(ops, a8, sa, w8, sw, dtype, *, bias=None, res=None, head_major=None, geglu=False, lda_gap=0):
    """dd_gemm8 through its descriptor: NaN-filled output, strided with a NaN pad (row-major) or with a guard plane
    (head-major); res with ldres > n; lda_gap bytes of NaN codes behind every row of A8."""
    from dualdiff_amd import _native
    rows, kp = a8.shape
    nw = w8.shape[0]
    n = nw // 2 if geglu else nw
    d = _native.Gemm8Desc()
    if lda_gap:
        abuf = torch.full((rows, kp + lda_gap), R.NAN_CODE, dtype=torch.uint8, device=DEV)
        abuf[:, :kp] = a8
        a8 = abuf[:, :kp]
    d.a, d.a_scale, d.lda = a8.data_ptr(), sa.data_ptr(), a8.stride(0)
    d.w, d.w_scale, d.ldw = w8.data_ptr(), sw.data_ptr(), w8.stride(0)
    d.bias = bias.data_ptr() if bias is not None else None
    if res is not None:
        rbuf, rview = G.strided(rows, n, dtype, DEV, NAN, pad=8)
        rview.copy_(res)
        d.res, d.ldres = rview.data_ptr(), rview.stride(0)
    if head_major is not None:
        hd, planes, scale = head_major
        buf = G.nan_like((n // hd + 1, rows, hd), dtype, DEV)
        out = buf[:n // hd]
        d.out, d.ldc = buf.data_ptr(), n
        d.out_headmajor_d, d.hm_scaled_planes, d.hm_scale = hd, planes, scale
    else:
        buf, out = G.strided(rows, n, dtype, DEV, NAN, pad=64)
        d.out, d.ldc = out.data_ptr(), out.stride(0)
    d.rows, d.n, d.k_padded, d.dtype, d.geglu = rows, n, kp, ops._FDT[dtype], int(geglu)
    _native.check(_native.load().dd_gemm8(ctypes.byref(d), ops._stream()), "gemm8")
    if head_major is not None:
        assert bool(torch.isnan(buf[n // hd]).all()), "wrote past the last plane"
    else:
        assert G.pad_untouched(buf, n, NAN), "wrote past column n"
    return out


@functools.lru_cache(maxsize=None)
def pool(kind, rows, n, kp, k, sw_exp=0):
    """Operands built once and shared (leading rows / channels are sliced off them); never written."""
    return tuple(t.to(DEV) for t in R.operands(kind, rows, n, kp, 11, k=k, sw_exp=sw_exp))


def take(p, rows, n):
    a8, sa, w8, sw = p
    return a8[:rows], sa[:rows], w8[:n], sw[:n]


def take_geglu(p, rows, n):
    """2n weight rows (h | g) out of the pool's first and second half."""
    a8, sa, w8, sw = p
    half = w8.shape[0] // 2
    return (a8[:rows], sa[:rows], torch.cat([w8[:n], w8[half:half + n]]).contiguous(),
            torch.cat([sw[:n], sw[half:half + n]]).contiguous())


@functools.lru_cache(maxsize=None)
def vec(n, dtype, seed):
    return G.rand((n,), dtype, seed, device=DEV)


@functools.lru_cache(maxsize=None)
def mat(rows, n, dtype, seed):
    return G.rand((rows, n), dtype, seed, device=DEV)


# ---- the row quantiser ----------------------------------------------------------------------------------------------------

def _rowquant_all_pitches(ops, x, norm):
    """The wrapper (pitch = the 128-rounded width) and the raw ABI at + 128 and + 384: the same bytes, zero padding."""
    c = x.shape[1]
    kp = (c + 127) // 128 * 128
    q, s = ops.rowquant_fp8(x, norm)
    q = q.view(torch.uint8)
    assert q.shape == (x.shape[0], kp) and s.shape == (x.shape[0],)
    for extra in (0, 128, 384):
        q2, s2 = rowquant_raw(ops, x, norm, kp + extra)
        assert torch.equal(q2[:, :kp], q) and bool((q2[:, kp:] == 0).all()), "pitch %d" % (kp + extra)
        assert torch.equal(torch.nan_to_num(s2, nan=-1.0), torch.nan_to_num(s, nan=-1.0))
    return q, s


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("c", [8, 504, 512, 520, 1024, 1032, 1536])
def test_rowquant(ops, dtype, c):
    gamma, beta = N.affine(c, dtype, 5, DEV)
    ratios, ln_ratios, pos, off, off_ln, total = [], [], [], 0, 0, 0
    for rows in (1, 3, 4, 5, 9):
        for i, kind in enumerate(R.ROWQUANT_KINDS):
            x = R.rowquant_data(kind, rows, c, dtype, 20 + i, DEV)
            what = "rowquant %s %dx%d %s" % (kind, rows, c, dtype)
            q, s = _rowquant_all_pitches(ops, x, None)
            off += R.check_rowquant(q, s, x, what)
            ratios.append(0.0)                                # check_rowquant is pass / fail: candidates, exact scale
            q, s = _rowquant_all_pitches(ops, x, (gamma, beta, EPS))
            r, p = R.check_rowquant_ln(q, s, x, gamma, beta, EPS, what + " ln")
            ln_ratios.append(r)
            pos.append(p)
            off_ln += R.bytes_off(q, ops.layernorm(x, gamma, beta, EPS))        # against the bytes of dd_layernorm's own y
            total += rows * c
    R.report("rowquant c=%d" % c, dtype, ratios, "   (candidates, exact scale)   %d of %d bytes off the fp32 recipe" % (off, total))
    R.report("rowquant+LayerNorm c=%d" % c, dtype, ln_ratios,
             "   scale at %.3f of its interval   %d of %d bytes off the fp32 recipe" % (max(pos), off_ln, total))
    assert max(pos) <= 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_tiny_rows_keep_their_zeros(ops, dtype):
    """A row far below 448 * 2^-126 (bf16: [1e-37, 0, -5e-38, ...]; fp16 cannot get there, its floor is 2^-24): 1 / scale
    must stay finite, so that a zero stays a zero and every element dequantises to within half a step."""
    x = R.rowquant_data("edge", 5, 16, dtype, 1, DEV)
    q, s = rowquant_raw(ops, x, None, 128)
    R.check_rowquant(q, s, x, "tiny rows %s" % dtype)
    s64 = s.to(torch.float64)[:, None]
    err = (R.decode(q[:, :16]) * s64 - x.to(torch.float64)).abs()
    b = 0.5 * R.spacing(x.to(torch.float64) / s64) * s64 * (1.0 + R.DELTA)
    assert bool((err <= b).all()) and bool((q[1, :16][x[1] == 0] & 0x7F == 0).all())
    R.report("rowquant tiny rows", dtype, [float((err / b.clamp(min=1e-300)).max())])


# ---- GEMM tile edges ------------------------------------------------------------------------------------------------------

EDGE_ROWS = (1, 127, 128, 129, 257)
EDGE_N = (4, 60, 64, 124, 128, 132, 260)
GEGLU_N = (4, 60, 64, 68, 132)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kp", [128, 256, 384])
def test_gemm8_tile_edges(ops, dtype, kp):
    p = pool("randn", 257, 260, kp, kp - 5)
    fam = {"plain": [], "bias": [], "bias+res": [], "head-major D=4": [], "lda > k_padded": []}
    for rows in EDGE_ROWS:
        for j, n in enumerate(EDGE_N):
            a8, sa, w8, sw = take(p, rows, n)
            what = "gemm8 %dx%dx%d %s " % (rows, n, kp, dtype)
            bias, res = vec(260, dtype, 3)[:n].clone(), mat(257, 260, dtype, 4)[:rows, :n]
            fam["plain"].append(R.check_gemm8(gemm8_raw(ops, a8, sa, w8, sw, dtype), a8, sa, w8, sw, what + "plain"))
            fam["bias"].append(R.check_gemm8(gemm8_raw(ops, a8, sa, w8, sw, dtype, bias=bias), a8, sa, w8, sw, what + "bias", bias=bias))
            fam["bias+res"].append(R.check_gemm8(gemm8_raw(ops, a8, sa, w8, sw, dtype, bias=bias, res=res), a8, sa, w8, sw,
                                                 what + "bias+res", bias=bias, res=res))
            hm = (4, (0, 1, n // 4)[(j + rows) % 3], 0.158)
            fam["head-major D=4"].append(R.check_gemm8(gemm8_raw(ops, a8, sa, w8, sw, dtype, bias=bias, head_major=hm), a8, sa, w8, sw,
                                                       what + "head-major %s" % (hm,), bias=bias, head_major=hm))
            if n in (4, 132):
                fam["lda > k_padded"].append(R.check_gemm8(gemm8_raw(ops, a8, sa, w8, sw, dtype, lda_gap=128), a8, sa, w8, sw,
                                                           what + "lda gap"))
    for name, ratios in fam.items():
        R.report("gemm8 %s kp=%d" % (name, kp), dtype, ratios)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gemm8_head_major_d40(ops, dtype):
    p = pool("randn", 257, 280, 256, 251)
    ratios = []
    for rows in (1, 129, 257):
        for n in (40, 120, 280):
            a8, sa, w8, sw = take(p, rows, n)
            for planes in (0, 1, n // 40):
                for bias in (None, vec(280, dtype, 3)[:n].clone()):
                    hm = (40, planes, 0.158)
                    ratios.append(R.check_gemm8(gemm8_raw(ops, a8, sa, w8, sw, dtype, bias=bias, head_major=hm), a8, sa, w8, sw,
                                                "gemm8 %dx%d head-major %s %s" % (rows, n, hm, dtype), bias=bias, head_major=hm))
    R.report("gemm8 head-major D=40", dtype, ratios)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kp", [128, 256, 384])
def test_gemm8_geglu_tile_edges(ops, dtype, kp):
    p = pool("randn", 257, 2 * 132, kp, kp - 5)
    ratios = []
    for rows in EDGE_ROWS:
        for n in GEGLU_N:
            a8, sa, w8, sw = take_geglu(p, rows, n)
            for bias in (None, vec(2 * n, dtype, 5)):
                y = gemm8_raw(ops, a8, sa, w8, sw, dtype, bias=bias, geglu=True)
                ratios.append(R.check_gemm8(y, a8, sa, w8, sw, "gemm8 GEGLU %dx%dx%d bias=%s %s" % (rows, n, kp, bias is not None, dtype),
                                            bias=bias, geglu=True))
    R.report("gemm8 GEGLU kp=%d" % kp, dtype, ratios)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("k", [1280, 2048])
def test_gemm8_deep_k(ops, dtype, k):
    rows, n = 129, 132
    a8, sa, w8, sw = pool("randn", rows, n, k, k - 8)
    bias, res = vec(n, dtype, 3), mat(rows, n, dtype, 4)
    ratios = [R.check_gemm8(gemm8_raw(ops, a8, sa, w8, sw, dtype), a8, sa, w8, sw, "gemm8 K=%d plain" % k),
              R.check_gemm8(gemm8_raw(ops, a8, sa, w8, sw, dtype, bias=bias, res=res, lda_gap=256), a8, sa, w8, sw,
                            "gemm8 K=%d bias+res" % k, bias=bias, res=res)]
    a8, sa, w8, sw = pool("exact-sum", rows, n, k, k - 8)
    ratios.append(R.check_exact(gemm8_raw(ops, a8, sa, w8, sw, dtype), a8, sa, w8, sw, "gemm8 K=%d exact-sum" % k))
    R.report("gemm8 K=%d" % k, dtype, ratios)


# ---- tile counts: the XCD remap -------------------------------------------------------------------------------------------

# (tiles_m * tiles_n, rows, n): 128 x 128 tiles
TILE_COUNTS = [(1, 100, 100), (7, 100, 7 * 128 - 4), (8, 200, 500), (9, 300, 300), (15, 380, 600), (16, 500, 500),
               (17, 17 * 128 - 100, 60), (27, 1100, 300)]
# the same with 64 gated channels per tile
TILE_COUNTS_GEGLU = [(1, 100, 60), (7, 100, 7 * 64 - 4), (8, 200, 252), (9, 300, 180), (15, 380, 300), (16, 500, 252),
                     (17, 17 * 128 - 100, 60), (27, 1100, 188)]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gemm8_tile_counts(ops, dtype):
    """onehot data: every output is one exact product, so a tile computed twice, never, or at the wrong place is a bit
    mismatch (or a NaN left in the output)."""
    p = pool("onehot", 17 * 128 - 100, 7 * 128 - 4, 256, 251)
    ratios = []
    for ntiles, rows, n in TILE_COUNTS:
        assert ((rows + 127) // 128) * ((n + 127) // 128) == ntiles
        a8, sa, w8, sw = take(p, rows, n)
        ratios.append(R.check_exact(gemm8_raw(ops, a8, sa, w8, sw, dtype), a8, sa, w8, sw, "gemm8 %d tiles %dx%d %s" % (ntiles, rows, n, dtype)))
    R.report("gemm8 tile counts, onehot", dtype, ratios, "   bit-equal")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gemm8_geglu_tile_counts(ops, dtype):
    """The same for GEGLU (h gelu(g) of two exact accumulators: held to the bound, which E_acc = TAU ||a|| ||w|| of a
    one-term sum makes a few units of the output type)."""
    p = pool("onehot", 17 * 128 - 100, 2 * (7 * 64 - 4), 256, 251, -7)
    ratios = []
    for ntiles, rows, n in TILE_COUNTS_GEGLU:
        assert ((rows + 127) // 128) * ((n + 63) // 64) == ntiles
        a8, sa, w8, sw = take_geglu(p, rows, n)
        y = gemm8_raw(ops, a8, sa, w8, sw, dtype, geglu=True)
        ratios.append(R.check_gemm8(y, a8, sa, w8, sw, "gemm8 GEGLU %d tiles %dx%d %s" % (ntiles, rows, n, dtype), geglu=True))
    R.report("gemm8 GEGLU tile counts, onehot", dtype, ratios)


# ---- data kinds -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["rowscale", "onehot", "exact-sum"])
def test_gemm8_data_kinds(ops, dtype, kind):
    rows, n, kp, k = 131, 132, 384, 300
    a8, sa, w8, sw = pool(kind, rows, n, kp, k)
    exact = kind != "rowscale"
    chk = R.check_exact if exact else R.check_gemm8
    hm = (4, 5, 0.25 if exact else 0.158)
    ratios = [chk(gemm8_raw(ops, a8, sa, w8, sw, dtype), a8, sa, w8, sw, "gemm8 %s plain %s" % (kind, dtype)),
              chk(gemm8_raw(ops, a8, sa, w8, sw, dtype, lda_gap=128), a8, sa, w8, sw, "gemm8 %s lda gap %s" % (kind, dtype)),
              chk(gemm8_raw(ops, a8, sa, w8, sw, dtype, head_major=hm), a8, sa, w8, sw, "gemm8 %s head-major %s" % (kind, dtype),
                  head_major=hm)]
    bias, res = vec(n, dtype, 3), mat(rows, n, dtype, 4)
    ratios.append(R.check_gemm8(gemm8_raw(ops, a8, sa, w8, sw, dtype, bias=bias, res=res), a8, sa, w8, sw,
                                "gemm8 %s bias+res %s" % (kind, dtype), bias=bias, res=res))
    a8, sa, w8, sw = pool(kind, rows, 2 * n, kp, k, 0 if kind == "exact-sum" else -7)      # h gelu(g) inside fp16
    for b in (None, vec(2 * n, dtype, 5)):
        ratios.append(R.check_gemm8(gemm8_raw(ops, a8, sa, w8, sw, dtype, bias=b, geglu=True), a8, sa, w8, sw,
                                    "gemm8 %s GEGLU %s" % (kind, dtype), bias=b, geglu=True))
    R.report("gemm8 %s" % kind, dtype, ratios, "   bit-equal without bias / GEGLU" if exact else "")


# ---- non-finite rows ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("ln", [False, True], ids=["plain", "layernorm"])
def test_nonfinite_rows(ops, dtype, ln):
    """A NaN or +Inf activation must not leave the projection as finite numbers: its row gets scale = NaN and comes out
    of dd_gemm8 non-finite in every column; every other row stays within its bound."""
    rows, c, n = 130, 520, 132
    x = R.rowquant_data("randn", rows, c, dtype, 31, DEV)
    x[3, 77] = NAN
    x[128, c - 1] = float("inf")
    x[129, 0] = float("-inf")
    gamma, beta = N.affine(c, dtype, 5, DEV)
    q, s = _rowquant_all_pitches(ops, x, (gamma, beta, EPS) if ln else None)
    bad = torch.tensor([r in (3, 128, 129) for r in range(rows)], device=DEV)
    assert torch.equal(torch.isnan(s), bad), "scale must be NaN on exactly the rows that hold a NaN or an Inf"
    assert not bool((q & 0x7F == R.NAN_CODE).any()), "NaN codes among the bytes"
    if ln:
        ratios = [R.check_rowquant_ln(q, s, x, gamma, beta, EPS, "non-finite rows ln %s" % dtype)[0]]
    else:
        R.check_rowquant(q, s, x, "non-finite rows %s" % dtype)
        ratios = [0.0]
    w8, sw = (t.to(DEV) for t in R.quantize_rows(G.rand((2 * n, c), dtype, 32, c ** -0.5, device="cpu")))
    bias = vec(2 * n, dtype, 5)
    q = q.contiguous()
    hm = (4, 1, 0.158)
    for what, kw, nw in (("plain", {}, n), ("bias", {"bias": bias[:n].clone()}, n), ("head-major", {"head_major": hm}, n),
                         ("GEGLU", {"bias": bias, "geglu": True}, 2 * n), ("GEGLU no bias", {"geglu": True}, 2 * n)):
        y = gemm8_raw(ops, q, s, w8[:nw], sw[:nw], dtype, **kw)
        ratios.append(R.check_gemm8(y, q, s, w8[:nw], sw[:nw], "gemm8 non-finite rows %s %s" % (what, dtype), **kw))
    R.report("non-finite rows %s" % ("ln" if ln else "plain"), dtype, ratios)
