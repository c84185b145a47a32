"""GPU cases for the tuned-table replay and the tile sweep: the operands of one dense GEMM or conv call, its fp64
reference (gemm_reference.py, computed once), and `run(tile, split)`, which launches the call with exactly that tile and
split-K (no tuner lookup) into a NaN-filled output and checks it against the bound.  Returns max |err| / bound."""
import torch

from dualdiff_amd import ops
from tests import gemm_reference as G
from tests.tuned_table import hm_planes

SENTINEL = -3.5                 # pad columns of a strided output: exact in fp16 / bf16, never a result here
LOG2E = 1.4426950408889634


def _rand(shape, dtype, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda", dtype=torch.float32) * scale + shift).to(dtype)


class DenseCase:
    """gemm(a[, a2], w, bias, ...) with the options of a table key.  a2_k1: two sources, the first k1 wide; ln: the
    LayerNorm fold (si: its input produced by an ln_stats=True GEMM); so: ln_stats output; hm: head-major width D;
    strided: A and the output are views with 64 pad columns (A's pad NaN, the output's SENTINEL); sample: compare only
    these rows (the byte-extent cases)."""

    def __init__(self, rows, n, k, dtype, seed, *, epilogue=ops.DD_EPI_NONE, a2_k1=None, ln=False, si=False, f32=False,
                 so=False, hm=None, res=False, acc=False, rowvec=False, alpha=1.0, bias=True, strided=False,
                 sample=None):
        self.rows, self.n, self.k, self.dtype = rows, n, k, dtype
        self.epilogue, self.f32, self.so, self.acc, self.alpha, self.strided = epilogue, f32, so, acc, alpha, strided
        geglu = epilogue == ops.DD_EPI_GEGLU
        nw = 2 * n if geglu else n
        self.a2 = None
        stats_of = None
        if si:
            x0 = _rand((rows, 320), dtype, seed + 1)
            w0 = _rand((k, 320), dtype, seed + 2, 320 ** -0.5)
            b0 = _rand((k,), dtype, seed + 3, 0.5)
            self.a = ops.gemm(x0, w0, b0, ln_stats=True, tile=52, split_k=1)
            with torch.no_grad():                 # what the producer's statistics describe: its unrounded result
                acc0, e0 = G.dense_acc(x0, w0, rows=sample)
                stats_of = G.epilogue(acc0, e0, bias=b0)
        else:
            k1 = a2_k1 or k
            a = _rand((rows, k1), dtype, seed + 1, 2.0 if ln else 1.0, 1.0 if ln else 0.0)
            if strided:
                self.a_buf = torch.full((rows, k1 + 64), float("nan"), dtype=dtype, device="cuda")
                self.a = self.a_buf[:, :k1]
                self.a.copy_(a)
                del a
            else:
                self.a = a
            if a2_k1:
                self.a2 = _rand((rows, k - k1), dtype, seed + 4)
        self.w = _rand((nw, k), dtype, seed + 5, k ** -0.5)
        self.ln = None
        self.bias = None
        if ln:
            self.ln = (self.w.double().sum(1).float().contiguous(), _rand((n,), torch.float32, seed + 6), 1e-5)
        elif bias:
            self.bias = _rand((nw,), dtype, seed + 7, 0.5)
        self.rowvec = _rand((-(-rows // 7), n), dtype, seed + 8, 0.5) if rowvec else None
        self.res = _rand((rows, n), dtype, seed + 9) if res else None
        self.old = _rand((rows, n), dtype, seed + 10) if acc else None
        self.hm = (hm, hm_planes(n, hm), hm ** -0.5 * LOG2E) if hm else None
        self.sample = sample
        with torch.no_grad():
            if ln:
                acc64, e = G.ln_fold_acc(self.a, self.w, self.ln[1], self.ln[2], rows=sample, stats_of=stats_of)
            else:
                acc64, e = G.dense_acc(self.a, self.w, self.a2, rows=sample)
            if geglu:
                self.ref, self.e = G.geglu(acc64, e, self.bias)
            else:
                self.ref, self.e = G.epilogue(acc64, e, bias=self.bias, rowvec=self.rowvec, rows_per_inst=7, alpha=alpha,
                                              res=self.res, silu=epilogue == ops.DD_EPI_SILU, old=self.old, rows=sample)
            if self.hm:
                self.ref, self.e = G.head_major(self.ref, self.e, *self.hm)
        self.odt = torch.float32 if f32 else dtype

    def run(self, tile, split):
        rows, n = self.rows, self.n
        out, buf = None, None
        if self.hm:
            # gemm allocates the head-major output itself: hand the caching allocator a NaN block of that size first
            poison = torch.full((rows * n,), float("nan"), dtype=self.dtype, device="cuda")
            del poison
        elif self.strided:
            buf = torch.full((rows, n + 64), SENTINEL, dtype=self.odt, device="cuda")
            buf[:, :n] = float("nan")
            out = buf[:, :n]
        elif self.acc:
            out = self.old.clone()
        else:
            out = torch.full((rows, n), float("nan"), dtype=self.odt, device="cuda")
        y = ops.gemm(self.a, self.w, self.bias, a2=self.a2, res=self.res, rowvec=self.rowvec, rows_per_inst=7,
                     alpha=self.alpha, out=out, accumulate=self.acc, epilogue=self.epilogue, tile=tile, split_k=split,
                     ln=self.ln, out_f32=self.f32, ln_stats=self.so, head_major=self.hm)
        what = "gemm %dx%dx%d tile %d split %d" % (rows, n, self.k, tile, split)
        with torch.no_grad():
            ys = y if self.sample is None else (y[:, self.sample] if self.hm else y[self.sample])
            r = G.check(ys, self.ref, self.e, what, self.odt)
            if self.so:
                st = y._ln_stats if self.sample is None else y._ln_stats[self.sample]
                r = max(r, G.check_stats(st, self.ref, self.e, what))
            if buf is not None:
                assert bool((buf[:, n:] == SENTINEL).all()), what + ": wrote into the pad columns of the output"
        return r


class ConvCase:
    """conv3x3(x, w, bias, m, hin, win, stride, up_size) in two epilogue forms: bias only, and the ResNet conv2 form
    bias + time-embedding row vector + residual with alpha != 1 (run(..., full=True)).  The fp64 accumulator is shared."""

    ALPHA = 0.7

    def __init__(self, m, hin, win, cin, cout, stride, dtype, seed, up=None):
        self.m, self.hin, self.win, self.cin, self.cout, self.stride, self.up, self.dtype = \
            m, hin, win, cin, cout, stride, up, dtype
        hv, wv = up if up else (hin, win)
        self.hout, self.wout = (hv - 1) // stride + 1, (wv - 1) // stride + 1
        self.rows = m * self.hout * self.wout
        self.x = _rand((m * hin * win, cin), dtype, seed + 1)
        self.w = _rand((cout, 9 * cin), dtype, seed + 2, (9 * cin) ** -0.5)
        self.bias = _rand((cout,), dtype, seed + 3, 0.5)
        self.rowvec = _rand((m, cout), dtype, seed + 4, 0.5)
        self.res = _rand((self.rows, cout), dtype, seed + 5)
        with torch.no_grad():
            acc, e = G.conv_acc(self.x, self.w, m, hin, win, stride, up)
            self.refs = {False: G.epilogue(acc, e, bias=self.bias),
                         True: G.epilogue(acc, e, bias=self.bias, rowvec=self.rowvec, rows_per_inst=self.hout * self.wout,
                                          alpha=self.ALPHA, res=self.res)}

    def run(self, tile, split, full=False, strided=False):
        rows, n = self.rows, self.cout
        buf = None
        if strided:
            buf = torch.full((rows, n + 64), SENTINEL, dtype=self.dtype, device="cuda")
            buf[:, :n] = float("nan")
            out = buf[:, :n]
        else:
            out = torch.full((rows, n), float("nan"), dtype=self.dtype, device="cuda")
        kw = dict(rowvec=self.rowvec, res=self.res, alpha=self.ALPHA) if full else {}
        y = ops.conv3x3(self.x, self.w, self.bias, self.m, self.hin, self.win, stride=self.stride, up_size=self.up,
                        out=out, tile=tile, split_k=split, **kw)
        what = "conv %dx%dx%d %d->%d s%d%s tile %d split %d%s" % (self.m, self.hin, self.win, self.cin, n, self.stride,
                                                                   " up%s" % (self.up,) if self.up else "", tile, split,
                                                                   " +temb+res" if full else "")
        with torch.no_grad():
            ref, e = self.refs[full]
            r = G.check(y, ref, e, what)
            if buf is not None:
                assert bool((buf[:, n:] == SENTINEL).all()), what + ": wrote into the pad columns of the output"
        return r


def sample_rows(rows, n_last=4096, n_spread=4096):
    """The last n_last rows plus n_spread evenly spaced ones (sorted, unique)."""
    idx = torch.cat([torch.arange(rows - n_last, rows), torch.linspace(0, rows - 1, n_spread).round().long()])
    return torch.unique(idx).cuda()
