"""Folded nearest-upsample conv, host side (dualdiff_amd/upfold.py, the planner of csrc/gemm.hip): classification, fold,
dispatch predicate and kernel-name query, without a GPU."""
import ctypes
import os

import pytest
import torch

from dualdiff_amd import _native, upfold
from dualdiff_amd.networks.layers import Conv3x3
from tests import upfold_reference as R

PAIRS = [((3, 4), (6, 8)), ((4, 7), (7, 13)), ((7, 13), (14, 25)), ((14, 25), (28, 50)), ((5, 5), (9, 9))]
IDS = ["%dx%d-%dx%d" % (a + b) for a, b in PAIRS]
M, CIN, COUT = 2, 8, 8


def _operands(seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return lambda *shape, scale=1.0: (torch.randn(shape, generator=g, dtype=torch.float64) * scale).to(dtype)


def test_classes_of_the_step_levels():
    """4 -> 7 by hand: src = 0 0 1 1 2 2 3, taps (x 0 0) (0 0 1) (0 1 1) (1 1 2) (1 2 2) (2 2 3) (2 3 x)."""
    assert upfold.axis_classes(4, 7) == [0, 1, 0, 1, 0, 1, 2]
    assert upfold.axis_classes(7, 13) == [0, 1] * 6 + [2]
    assert upfold.axis_classes(13, 25) == [0, 1] * 12 + [2]
    assert upfold.axis_classes(3, 6) == [0, 1] * 3                     # exact 2x: the last tap +1 of class 1 leaves the source
    assert upfold.axis_classes(5, 9) == [0, 1] * 4 + [2]
    assert len(upfold.classes(14, 25, 28, 50)[2]) == 4 and len(upfold.classes(7, 13, 14, 25)[2]) == 6
    assert len(upfold.classes(4, 7, 7, 13)[2]) == 9


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_fp64_fold_equals_upsample_then_conv(pair):
    (hin, win), (hv, wv) = pair
    r = _operands(1)
    x, w = r(M * hin * win, CIN), r(COUT, 9 * CIN, scale=(9 * CIN) ** -0.5)
    wf = upfold.fold_weight(w, hin, win, hv, wv, sum_dtype=torch.float64)
    assert wf.dtype == torch.float64 and wf.shape == (len(upfold.classes(hin, win, hv, wv)[2]) * COUT, 4 * CIN)
    ref = R.brute_acc(x, w, M, hin, win, hv, wv)
    got = R.folded_acc(x, wf, M, hin, win, hv, wv)[0]
    # fp64 rounding only: both are sums of at most 9 cin products (+ the fold's own adds), each off by <= depth * 2^-53 * sum |x||w|
    tol = (9 * CIN + 4) * 2.0 ** -53 * R.brute_acc(x.abs(), w.abs(), M, hin, win, hv, wv)
    assert bool(((got - ref).abs() <= tol).all()), float(((got - ref).abs() / tol).max())
    assert float(ref.abs().max()) > 0.5                                # not vacuous


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_rounded_fold_within_one_unit_roundoff_of_the_weights(pair, dtype):
    """Weights folded in fp32 and rounded once to the storage type against the 9-tap result of the ORIGINAL weights:
    |diff| <= u * sum |x| |w'| per element."""
    (hin, win), (hv, wv) = pair
    r = _operands(2, dtype)
    x, w = r(M * hin * win, CIN), r(COUT, 9 * CIN, scale=(9 * CIN) ** -0.5)
    wf = upfold.fold_weight(w, hin, win, hv, wv)
    assert wf.dtype == dtype
    ref = R.brute_acc(x, w, M, hin, win, hv, wv)
    got = R.folded_acc(x, wf, M, hin, win, hv, wv)[0]
    sabs = R.fold_abs(x, w, M, hin, win, hv, wv)
    tol = R.UNIT_ROUNDOFF[dtype] * sabs + (9 * CIN + 4) * 2.0 ** -53 * sabs        # + the fp64 evaluation of both sides
    err = (got - ref).abs()
    print("%s %s: max |diff| / (u sum|x||w'|) = %.3f" % (pair, dtype, float((err / tol).max())))
    assert bool((err <= tol).all())
    assert float(err.max()) > 0                                        # the rounding is really there


def test_predicate():
    for (hin, win), (hv, wv) in PAIRS:
        assert upfold.ok(hin, win, hv, wv)
    assert not upfold.ok(10, 10, 11, 11)              # some coordinate sees s - 1, s, s + 1
    assert not upfold.ok(8, 8, 4, 4)                  # downscale
    assert not upfold.ok(14, 25, 14, 25)              # no resize
    assert not upfold.ok(14, 25, 28, 25) and not upfold.ok(10, 25, 11, 50)        # one axis is enough to refuse
    assert not upfold.ok(14, 25, 28, 50, cin=8) and not upfold.ok(14, 25, 28, 50, stride=2)
    assert not upfold.ok(56, 100, 112, 200)           # beyond the kernel's coordinate lists (the VAE decoder's upsamplers)
    with pytest.raises(ValueError):
        upfold.fold_weight(torch.zeros(8, 72), 10, 10, 11, 11)


def _desc(m, hin, win, hv, wv, cin, cout, tile, fold, dtype=0):
    d = _native.GemmDesc()
    d.a = d.w = d.out = 4096                          # aligned dummies: the planner dereferences nothing
    d.rows, d.n = m * hv * wv, cout
    d.k = d.k1 = (4 if fold else 9) * cin
    d.lda, d.ldc, d.alpha, d.dtype, d.conv = cin, cout, 1.0, dtype, 1
    d.cin, d.hin, d.win, d.hv, d.wv, d.hout, d.wout, d.stride = cin, hin, win, hv, wv, hv, wv, 1
    d.tile, d.upfold = tile, int(fold)
    return d


def _mangled(kernel):
    base, args = kernel.rstrip(">").split("<")
    enc = {"_Float16": "DF16_", "__bf16": "DF16b"}
    return ("_ZN12_GLOBAL__N_1%d%sI%sE" % (len(base), base, "".join(enc.get(a) or "Li%dE" % int(a) for a in args.split(", ")))).encode()


def test_kernel_name_query():
    from dualdiff_amd import _build
    lib = _native.load()
    name = lambda d: lib.dd_gemm_kernel_name(ctypes.byref(d)).decode()
    blob = open(_build.lib_path(), "rb").read()
    tiles = {12: 128, 13: 128, 14: 64, 15: 64, 20: 256, 28: 160, 44: 192, 52: 96}       # ring tiles that carry the form: rows
    for (hin, win), (hv, wv) in PAIRS + [((28, 32), (56, 64))]:
        ycls, xcls, cls = upfold.classes(hin, win, hv, wv)
        for tile, bm in tiles.items():
            for dtype in (0, 1):
                n = name(_desc(12, hin, win, hv, wv, 128, 96, tile, True, dtype))
                assert n.startswith("dd_gemm2u_kernel<%s, " % ("_Float16", "__bf16")[dtype]), n
                assert _mangled(n.split(" split=")[0]) in blob, n
                # the planner's classes are upfold.py's: every class starts on a tile boundary
                want = sum(-(-12 * ycls.count(rc) * xcls.count(cc) // bm) for rc, cc in cls)
                assert int(n.split("grid=")[1].split("x")[0]) == want, (n, want)
        # a tile without the form, and the library's own pick
        assert name(_desc(12, hin, win, hv, wv, 128, 96, 27, True)) == "unsupported"
        assert name(_desc(12, hin, win, hv, wv, 128, 96, 1, True)) == "unsupported"
        assert name(_desc(12, hin, win, hv, wv, 128, 96, 0, True)).startswith("dd_gemm2u_kernel<")
    # refused maps: the folded form is never planned for them, the 9-tap kernel takes the layer
    for (hin, win), (hv, wv) in [((10, 10), (11, 11)), ((8, 8), (4, 4)), ((56, 100), (112, 200)), ((14, 25), (14, 25))]:
        d = _desc(2, hin, win, hv, wv, 128, 96, 15, True)
        assert name(d) == "unsupported" and lib.dd_gemm(ctypes.byref(d), None) == -2, (hin, hv)
        assert lib.dd_gemm_workspace_bytes(ctypes.byref(d)) == 0
        conv = Conv3x3(128, 96)
        assert conv.folded_up(hin, win, (hv, wv)) is None
        nine = name(_desc(2, hin, win, hv, wv, 128, 96, 15, False))
        assert nine.startswith("dd_gemm2_kernel<_Float16, 2, 2, 2, 2, 3, true, false>"), nine
    assert name(_desc(2, 14, 25, 28, 50, 72, 96, 15, True)) == "unsupported"           # cin % 64
    bad = _desc(2, 14, 25, 28, 50, 128, 96, 15, True)
    bad.k = 9 * 128                                    # the folded form has k = 4 cin
    assert name(bad) == "invalid"


def test_module_folds_once_and_drops_with_the_packed_weights():
    assert Conv3x3.fold_upsample == (os.environ.get("DD_UPFOLD", "1") != "0")
    conv = Conv3x3(64, 64)
    with torch.no_grad():
        conv.weight.normal_(0, 0.05)
        conv.bias.zero_()
    conv = conv.to(torch.float16)
    wf = conv.folded_up(4, 7, (7, 13))
    assert wf.shape == (9 * 64, 4 * 64) and wf.dtype == torch.float16
    assert conv.folded_up(4, 7, (7, 13)) is wf                        # cached per size pair
    assert conv.folded_up(7, 13, (14, 25)).shape == (6 * 64, 4 * 64)
    assert torch.equal(wf, upfold.fold_weight(conv.packed, 4, 7, 7, 13))
    conv._drop_cache()
    assert "_pk_upfold" not in conv.__dict__
    assert conv.folded_up(4, 7, (7, 13)) is not wf
    # with the instance count (the model's path) the layer folds only a shape with a winning row in the tracked table
    big = Conv3x3(640, 640).to(torch.float16)
    assert big.folded_up(14, 25, (28, 50), 12) is not None and big.folded_up(14, 25, (28, 50), 5) is None
    wide = Conv3x3(1280, 1280).to(torch.float16)
    assert wide.folded_up(4, 7, (7, 13), 12) is None                  # recorded as no faster folded: tile 0
    conv.fold_upsample = False                                        # what DD_UPFOLD=0 sets
    assert conv.folded_up(4, 7, (7, 13)) is None
    assert conv.folded_up(4, 7, None) is None
