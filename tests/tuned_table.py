"""Helpers shared by the tuned-table and tile-sweep tests: the tracked table, and dd_gemm descriptors rebuilt from a
table key (dummy pointers — what the planner needs to report a plan without a device)."""
import ast
import json

from dualdiff_amd import _native, ops

DUMMY = 4096                                     # aligned, never dereferenced by the planner

# up-block ResNet shortcuts (unet_2d_condition_multiview.py up blocks; layers.py ResnetBlock2D.run(x, x2=skip)):
# K = hidden width + skip width -> hidden width k1
UP_CONCAT_K1 = {2560: 1280, 1920: 1280, 1280: 640, 960: 640, 640: 320}


def a2_k1(k):
    """k1 of a two-source GEMM key (the key does not record it): the up blocks' concat widths, else 64 * floor(k / 128)."""
    return UP_CONCAT_K1.get(k, 64 * (k // 128))


def hm_planes(n, d):
    """Scaled (Q) planes of a head-major projection: the fused Q|K|V form has n / D = 3 * heads planes, a Q-only
    projection n / D = heads."""
    p = n // d
    return p // 3 if p % 3 == 0 else p


def load_table():
    with open(ops.TUNE_TABLE_PATH) as f:
        blob = json.load(f)
    assert blob["arch"] == "gfx950"
    return [(ast.literal_eval(k), tuple(int(x) for x in v)) for k, v in blob["entries"]]


def desc_from_key(key, tile, split, *, k1=None, lda=None, ldc=None, bias=True, rowvec=False):
    """dd_gemm descriptor of the call a table key stands for, with the given tile / split-K.  The overrides describe
    sweep variants the key does not record: a2's k1, padded row strides, no bias, a per-instance row vector."""
    d = _native.GemmDesc()
    d.a = d.w = d.out = DUMMY
    d.alpha = 1.0
    d.tile, d.split_k = tile, split
    if key[0] == "c":
        m, hin, win, cin, cout, stride, hv, wv, dt = key[1:]
        hout, wout = (hv - 1) // stride + 1, (wv - 1) // stride + 1
        d.rows, d.n, d.k, d.k1 = m * hout * wout, cout, 9 * cin, 9 * cin
        d.lda, d.ldc = cin, ldc or cout
        d.bias = DUMMY if bias else None
        d.dtype = dt
        d.conv = 1
        d.cin, d.hin, d.win, d.hv, d.wv, d.hout, d.wout, d.stride = cin, hin, win, hv, wv, hout, wout, stride
    if rowvec:
        d.rowvec, d.ld_rowvec, d.rows_per_inst = DUMMY, d.n, 7
    if key[0] == "c":
        return d
    rows, n, k, epi, dt, a2, ln = key[1:8]
    flags = key[8:]
    d.rows, d.n, d.k = rows, n, k
    d.epilogue, d.dtype = epi, dt
    d.k1 = (k1 or a2_k1(k)) if a2 else k
    d.lda = lda or d.k1
    if a2:
        d.a2, d.lda2 = DUMMY, k - d.k1
    if ln:
        d.ln_colsum = d.ln_bias = DUMMY
        d.ln_eps = 1e-5
    elif bias:
        d.bias = DUMMY
    d.ldc = ldc or n
    i = 0
    while i < len(flags):
        f = flags[i]
        if f == "f32":
            d.out_f32 = 1
        elif f == "so":
            d.ln_stats_out = DUMMY
        elif f == "si":
            d.ln_stats_in = DUMMY
        elif f == "hm":
            i += 1
            d.out_headmajor_d, d.hm_scaled_planes, d.hm_scale = flags[i], hm_planes(n, flags[i]), 0.125
        elif f == "res":
            d.res, d.ldres = DUMMY, n
        elif f == "acc":
            d.accumulate = 1
        else:
            raise AssertionError("unknown flag %r in %r" % (f, key))
        i += 1
    return d


def expected_split(key, plan, split):
    if key[0] == "c" and plan.startswith("dd_conv3s"):
        chunks = key[4] // 64
    else:
        chunks = -(-(9 * key[4] if key[0] == "c" else key[3]) // 64)
    if key[0] == "g" and (key[4] == ops.DD_EPI_GEGLU or key[7] or "so" in key[8:] or "hm" in key[8:]):
        split = 1                               # GEGLU / LayerNorm fold / row statistics / head-major: one K range
    split = min(max(split, 1), chunks)
    return -(-chunks // -(-chunks // split))


def family(plan):
    return plan.split("_kernel")[0]


