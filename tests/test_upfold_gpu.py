"""dd_gemm2u_kernel, the folded nearest-upsample conv, per element against fp64 (tests/upfold_reference.py).

Two references per case: the kernel on ITS operands (x and the folded weights) with the bound every conv launch is held
to (tests/gemm_reference.py), and end to end against the 9-tap fp64 result of the ORIGINAL weights with that bound plus
the fold term u * sum |x| |w'| (the folded weights are rounded once to the storage type).

Shapes: 2 instances; 4x7 -> 7x13 (tail classes on both axes, nine classes of 2 .. 36 rows: far smaller than a tile),
7x13 -> 14x25 (a tail on one axis), 3x4 -> 6x8 (exact 2x); Cin 64 / 128 (one and two K chunks per slot); Cout 64 / 96 (a
column tail of every tile); every tile that carries the form; split-K 1 and 2."""
import pytest
import torch

from dualdiff_amd import ops, tuning, upfold
from dualdiff_amd.networks.layers import Conv3x3
from tests import gemm_reference as G
from tests import upfold_reference as R

pytestmark = pytest.mark.gpu

TILES = (12, 13, 14, 15, 20, 28, 44, 52)            # the ring tiles whose rows carry F_UPFOLD (csrc/gemm_tiles.h)
SIZES = [((4, 7), (7, 13)), ((7, 13), (14, 25)), ((3, 4), (6, 8))]
M, ALPHA = 2, 0.7


def _rand(shape, dtype, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda", dtype=torch.float32) * scale).to(dtype)


class Case:
    """Operands and fp64 references of one (size, cin, cout, dtype), computed once."""

    def __init__(self, size, cin, cout, dtype, seed):
        (self.hin, self.win), self.up = size
        hv, wv = self.up
        self.cin, self.cout, self.dtype, self.rows = cin, cout, dtype, M * hv * wv
        self.x = _rand((M * self.hin * self.win, cin), dtype, seed + 1)
        self.w = _rand((cout, 9 * cin), dtype, seed + 2, (9 * cin) ** -0.5)
        self.wf = upfold.fold_weight(self.w, self.hin, self.win, hv, wv)
        self.bias = _rand((cout,), dtype, seed + 3, 0.5)
        self.rowvec = _rand((M, cout), dtype, seed + 4, 0.5)
        self.res = _rand((self.rows, cout), dtype, seed + 5)
        self.old = _rand((self.rows, cout), dtype, seed + 6)
        with torch.no_grad():
            own = R.folded_acc(self.x, self.wf, M, self.hin, self.win, hv, wv)
            nine = G.conv_acc(self.x, self.w, M, self.hin, self.win, 1, self.up)
            fold = R.UNIT_ROUNDOFF[dtype] * R.fold_abs(self.x, self.w, M, self.hin, self.win, hv, wv)
            self.refs = {}
            for form, kw in (("bias", {}), ("full", dict(rowvec=self.rowvec, rows_per_inst=hv * wv, alpha=ALPHA, res=self.res)),
                             ("acc", dict(old=self.old))):
                a = abs(kw.get("alpha", 1.0))
                r9, e9 = G.epilogue(*nine, bias=self.bias, **kw)
                self.refs[form] = (G.epilogue(*own, bias=self.bias, **kw), (r9, e9 + a * fold))

    def run(self, tile, split, form):
        out = self.old.clone() if form == "acc" else G.nan_like((self.rows, self.cout), self.dtype, "cuda")
        kw = dict(rowvec=self.rowvec, res=self.res, alpha=ALPHA) if form == "full" else {}
        y = ops.conv3x3(self.x, self.w, self.bias, M, self.hin, self.win, up_size=self.up, upfold=self.wf, out=out,
                        accumulate=form == "acc", tile=tile, split_k=split, **kw)
        what = "upfold %dx%d->%dx%d %d->%d %s tile %d split %d %s" % (self.hin, self.win, *self.up, self.cin, self.cout,
                                                                     self.dtype, tile, split, form)
        (ro, eo), (r9, e9) = self.refs[form]
        return G.check(y, ro, eo, what + " (own operands)"), G.check(y, r9, e9, what + " (9-tap fp64)")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("size", SIZES, ids=["4x7-7x13", "7x13-14x25", "3x4-6x8"])
def test_every_tile_and_split_against_fp64(size, dtype):
    worst = (0.0, 0.0)
    for cin in (64, 128):
        for cout in (64, 96):
            case = Case(size, cin, cout, dtype, 100 * cin + cout)
            for tile in TILES:
                for split in (1, 2):
                    for form in ("bias", "full", "acc"):
                        r = case.run(tile, split, form)
                        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    print("max err / bound: own operands %.3f, 9-tap %.3f" % worst)


def test_tracked_rows_name_tested_tiles():
    """Every tile the tracked table assigns to the folded form is one of TILES, and plans to dd_gemm2u_kernel."""
    import ast, json, os
    if not os.path.exists(tuning.UPFOLD_TABLE_PATH):
        pytest.fail("dualdiff_amd/tuned/gfx950_upfold.json is missing")
    rows = [(ast.literal_eval(k), v) for k, v in json.load(open(tuning.UPFOLD_TABLE_PATH))["entries"]]
    assert rows
    for key, v in rows:
        assert key[0] == "c" and key[-1] == "uf" and (v[0] == 0 or v[0] in TILES) and v[1] >= (v[0] != 0), (key, v)
        assert upfold.ok(key[2], key[3], key[7], key[8], key[4], key[6]), key


@pytest.mark.parametrize("tile,split", [(15, 1), (28, 2)])
def test_padding_rows_are_never_stored_and_every_pixel_once(tile, split):
    """4x7 -> 7x13, 2 instances: nine classes of 2 .. 36 rows, each padded to a whole tile.  The output sits in the middle of
    a sentinel-filled buffer and is accumulated into.  A padding row's map value is the row count: were it stored, it would
    land on the sentinel rows behind the output; rows in front, and the pad columns, must stay untouched too.  Every pixel
    must hold sentinel + v: a pixel no row maps to keeps the bare sentinel.  (Two rows mapped to ONE pixel would not show
    here — the epilogue loads the accumulate target before its stores, both would write sentinel + v; a wrong map is what
    the NaN-prefilled fp64 comparisons of test_every_tile_and_split_against_fp64 catch, on every class of these shapes.)"""
    cin, cout, hin, win, up, dtype = 64, 96, 4, 7, (7, 13), torch.float16
    rows = M * up[0] * up[1]
    x = _rand((M * hin * win, cin), dtype, 1)
    w = _rand((cout, 9 * cin), dtype, 2, (9 * cin) ** -0.5)
    wf = upfold.fold_weight(w, hin, win, *up)
    S = 64.0                                          # a fp16 binade where v (|v| < 8) adds exactly enough to tell 1 from 2 stores
    buf = torch.full((rows + 512, cout + 64), S, dtype=dtype, device="cuda")
    out = buf[256:256 + rows, :cout]
    plain = ops.conv3x3(x, w, None, M, hin, win, up_size=up, upfold=wf, tile=tile, split_k=split)
    ops.conv3x3(x, w, None, M, hin, win, up_size=up, upfold=wf, out=out, accumulate=True, tile=tile, split_k=split)
    torch.cuda.synchronize()
    assert bool((buf[:256] == S).all()) and bool((buf[256 + rows:] == S).all()), "rows outside the output were written"
    assert bool((buf[:, cout:] == S).all()), "columns past the output were written"
    once = (plain.float() + S).to(dtype)              # fp32 add of the stored value, rounded once: the accumulate epilogue on v
    err = (out.float() - once.float()).abs()
    assert float(err.max()) <= 2.0 ** -4, float(err.max())          # one fp16 unit at 64: v itself was rounded before the add
    assert float(plain.float().abs().max()) > 0.5                   # ... and v is not all zero
    assert bool(torch.isfinite(plain).all())


def test_upfold_off_is_the_nine_tap_launch_bit_for_bit(monkeypatch):
    """DD_UPFOLD=0 (Conv3x3.fold_upsample False): the layer launches exactly the 9-tap gather it launched before the
    folded form existed — same kernel, same bits as ops.conv3x3 on the packed weights.  The shape has a winning row in the
    tracked table of the folded form and its 9-tap key a row in the main one, so nothing is tuned here."""
    dtype, m, h, w_, up, c = torch.float16, 2, 8, 8, (16, 16), 640
    row = tuning.upfold_tuned(tuning.conv_upfold_key(m, h, w_, c, c, up[0], up[1], ops.DD_F16))
    assert row is not None and row[0] in TILES
    assert tuning.conv_key(m, h, w_, c, c, 1, up[0], up[1], ops.DD_F16) in {k for k, _ in __import__("tests.tuned_table", fromlist=["x"]).load_table()}
    conv = Conv3x3(c, c)
    with torch.no_grad():
        conv.weight.normal_(0, (9 * c) ** -0.5)
        conv.bias.normal_(0, 0.5)
    conv = conv.to("cuda", dtype)
    x = _rand((m * h * w_, c), dtype, 7)
    nine = ops.conv3x3(x, conv.packed, conv.bias, m, h, w_, up_size=up)
    monkeypatch.setattr(Conv3x3, "fold_upsample", False)
    assert conv.folded_up(h, w_, up, m) is None
    off = conv.run(x, m, h, w_, up_size=up)
    assert torch.equal(off, nine)
    monkeypatch.setattr(Conv3x3, "fold_upsample", True)
    assert conv.folded_up(h, w_, up, m) is not None
    assert conv.folded_up(h, w_, up, 3) is None        # no row for 3 instances: the layer folds measured wins only
    on = conv.run(x, m, h, w_, up_size=up)
    assert not torch.equal(on, nine)                  # another kernel, other rounding ...
    with torch.no_grad():
        acc, e = G.conv_acc(x, conv.packed, m, h, w_, 1, up)
        ref, e = G.epilogue(acc, e, bias=conv.bias)
        G.check(on, ref, e + R.UNIT_ROUNDOFF[dtype] * R.fold_abs(x, conv.packed, m, h, w_, *up), "Conv3x3.run folded")   # ... same result
