"""Self-test of the fp64 reference / error bound in gemm_reference.py (CPU only): the bound must pass a correctly rounded
result and an fp32-accumulated one summed in a random order, and must catch each fault a tiled split-K GEMM with a fused
epilogue can plausibly make — one at a time, at a modest and at a deep K."""
import pytest
import torch

from tests import gemm_reference as G

DTYPES = [torch.float16, torch.bfloat16]
ALPHA = 0.75
BT = 64                                           # output tile edge of the injected faults


def _case(dtype, rows, n, k):
    a = G.rand((rows, k), dtype, 1, device="cpu")
    w = G.rand((n, k), dtype, 2, k ** -0.5, device="cpu")
    bias = G.rand((n,), dtype, 3, 0.5, device="cpu")
    res = G.rand((rows, n), dtype, 4, device="cpu")
    acc, e_acc = G.dense_acc(a, w)
    ref, e = G.epilogue(acc, e_acc, bias=bias, alpha=ALPHA, res=res)
    return a, w, bias, res, acc, ref, e


def _out(v, dtype):
    return v.to(dtype)


def _faults(dtype, a, w, bias, res, acc, ref):
    """name -> faulty output, each a correctly rounded result with ONE fault injected."""
    rows, n = ref.shape
    k = a.shape[1]
    A, W = a.double(), w.double()
    r0, c0 = BT, BT                                        # the faulty tile: second row tile, second column tile
    out = {}

    v = ref.clone()                                        # one 64-wide K chunk missing in one output tile
    kc = (k // 64 // 2) * 64
    v[r0:r0 + BT, c0:c0 + BT] -= ALPHA * (A[r0:r0 + BT, kc:kc + 64] @ W[c0:c0 + BT, kc:kc + 64].t())
    out["missing K chunk"] = _out(v, dtype)

    nkt = k // 64                                          # split-K 16 (normalised: 16 -> ceil(nkt / ceil(nkt / 16)))
    kts = -(-nkt // 16)
    s0 = (nkt - 1) // kts * kts * 64                       # the last (possibly short) slab counted twice
    v = ref + ALPHA * (A[:, s0:] @ W[:, s0:].t())
    out["last split slab twice"] = _out(v, dtype)

    v = ref.clone()                                        # bias added twice on one column tile
    v[:, c0:c0 + BT] += ALPHA * bias.double()[None, c0:c0 + BT]
    out["bias twice on a column tile"] = _out(v, dtype)

    v = ALPHA * (acc + bias.double()[None, :] + res.double())      # res inside alpha
    out["res inside alpha"] = _out(v, dtype)

    y = _out(ref, dtype)                                   # last partial row tile never written (NaN-filled output)
    y[(rows - 1) // BT * BT:] = float("nan")
    out["last partial row tile unwritten"] = y

    y = _out(ref, dtype)                                   # one 8-column group stored one group to the right
    y[:, 40:48] = y[:, 48:56].clone()
    out["8-column group shifted"] = y

    i = int(ref.abs().argmax())                            # one element off by 4 units of the output type
    y = _out(ref, dtype)
    yi = y.view(-1)[i].double()
    y.view(-1)[i] = (yi + 4 * G.ulp(yi, dtype)).to(dtype)
    out["one element off by 4 ulp"] = y
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [640, 5760])
def test_checker_passes_correct_results(dtype, k):
    a, w, bias, res, acc, ref, e = _case(dtype, 200, 160, k)
    G.check(ref.to(dtype), ref, e, "correctly rounded")
    # fp32 accumulation over the 64-wide K chunks in a random order, fp32 epilogue: what a split-K tile schedule does
    g = torch.Generator().manual_seed(7)
    acc32 = torch.zeros(acc.shape, dtype=torch.float32)
    for c in torch.randperm(k // 64, generator=g).tolist():
        acc32 += a[:, c * 64:(c + 1) * 64].float() @ w[:, c * 64:(c + 1) * 64].float().t()
    y = (ALPHA * (acc32 + bias.float()[None, :]) + res.float()).to(dtype)
    ratio = G.check(y, ref, e, "fp32, random order")
    assert ratio > 0.05, "the bound is vacuous at this shape: max err / bound = %.3g" % ratio


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [640, 5760])
def test_checker_catches_each_fault(dtype, k):
    a, w, bias, res, acc, ref, e = _case(dtype, 200, 160, k)
    faults = _faults(dtype, a, w, bias, res, acc, ref)
    assert len(faults) == 7
    for name, y in faults.items():
        with pytest.raises(AssertionError, match="outside the bound"):
            G.check(y, ref, e, name)


def test_epilogue_forms_pass_correct_results():
    """SiLU + accumulate, GEGLU, head-major, the LayerNorm fold: an fp32 evaluation of each form, rounded, is inside
    the bound; a 2-ulp fault on the largest element is not."""
    dtype = torch.float16
    a = G.rand((96, 320), dtype, 1, device="cpu")
    w = G.rand((128, 320), dtype, 2, 320 ** -0.5, device="cpu")
    bias = G.rand((128,), dtype, 3, 0.5, device="cpu")
    old = G.rand((96, 128), dtype, 5, device="cpu")
    acc, e_acc = G.dense_acc(a, w)
    acc32 = a.float() @ w.float().t()

    ref, e = G.epilogue(acc, e_acc, bias=bias, silu=True, old=old)
    y = (torch.nn.functional.silu(acc32 + bias.float()) + old.float()).to(dtype)
    G.check(y, ref, e, "silu + accumulate")

    ref, e = G.geglu(acc, e_acc, bias)
    v = acc32 + bias.float()
    y = (v[:, :64] * torch.nn.functional.gelu(v[:, 64:])).to(dtype)
    G.check(y, ref, e, "geglu")

    ref, e = G.epilogue(acc, e_acc, bias=bias)
    ref, e = G.head_major(ref, e, 32, 2, 0.125)
    y = (acc32 + bias.float()).reshape(96, 4, 32).permute(1, 0, 2).clone()
    y[:2] *= 0.125
    y = y.to(dtype).contiguous()
    G.check(y, ref, e, "head-major")
    i = int(ref.abs().argmax())
    y.view(-1)[i] = (y.view(-1)[i].double() + 2 * G.ulp(y.view(-1)[i].double(), dtype)).to(dtype)
    with pytest.raises(AssertionError):
        G.check(y, ref, e, "head-major, 2 ulp off")

    x = (G.rand((96, 320), torch.float32, 6, device="cpu") * 3 + 1.5).to(dtype)        # non-zero mean rows
    lnb = G.rand((128,), torch.float32, 7, device="cpu")
    ref, e = G.ln_fold_acc(x, w, lnb, 1e-5)
    xf = x.float()
    mean, var = xf.mean(1, keepdim=True), xf.var(1, unbiased=False, keepdim=True)
    colsum = w.float().sum(1)
    y = ((xf @ w.float().t() - mean * colsum[None, :]) * torch.rsqrt(var + 1e-5) + lnb[None, :]).to(dtype)
    G.check(y, ref, e, "layernorm fold")
