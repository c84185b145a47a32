"""Derived weights (layers.derived) on the GPU: after an in-place update of a parameter the next EAGER call computes, bit
for bit, what a fresh module loaded with the updated weights computes — through every kernel-layout copy on the way (padded,
packed, fused, folded, fp8) — and a stream capture keeps the copy it was warmed up with."""
import pytest
import torch

from dualdiff_amd import ops
from dualdiff_amd.networks import layers as L
from dualdiff_amd.networks.txt_con_fusion import txt_con_XFormersAttn

pytestmark = pytest.mark.gpu

DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])


def _rand(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).cuda().to(dtype)


def _module(make, dtype, seed=3):
    return L.seeded_init_(make(), seed).cuda().to(dtype)


def _follows(make, run, names, dtype):
    """run(module) after `weight.mul_(0.5)` on each of `names` in turn == run(fresh module with the updated state)."""
    with torch.no_grad():
        mod = _module(make, dtype)
        prev = run(mod).clone()
        for name in names:
            mod.get_parameter(name).mul_(0.5)
            got = run(mod)
            assert not torch.equal(got, prev), name               # the update reaches the output at all
            fresh = make().cuda().to(dtype)
            fresh.load_state_dict(mod.state_dict())
            want = run(fresh)
            assert torch.isfinite(want.float()).all() and torch.equal(got, want), name
            prev = got.clone()


@DTYPES
def test_linear_padded_k(dtype):
    x = _rand((16, 189), dtype, 1)
    _follows(lambda: L.Linear(189, 320), lambda m: m.run(x), ["weight"], dtype)


@DTYPES
def test_conv3x3_packed(dtype):
    x = _rand((2 * 8 * 8, 64), dtype, 2)
    _follows(lambda: L.Conv3x3(64, 64), lambda m: m.run(x, 2, 8, 8), ["weight"], dtype)


@DTYPES
def test_conv3x3_folded_upsample(dtype):
    x = _rand((2 * 4 * 7, 64), dtype, 3)

    def run(conv):
        wf = conv.folded_up(4, 7, (7, 13))
        assert wf is not None
        return ops.conv3x3(x, conv.packed, conv.bias, 2, 4, 7, up_size=(7, 13), upfold=wf)
    _follows(lambda: L.Conv3x3(64, 64), run, ["weight"], dtype)


@DTYPES
def test_transformer_320(dtype):
    """Fused Q|K|V (attn1), fused K|V and the packed to_q / to_out of dd_xattn320 (attn2), the LayerNorm-emitting to_out and
    the folded feed-forward / proj_out GEMM."""
    x, ctx = _rand((1 * 8 * 8, 320), dtype, 4), _rand((78, 768), dtype, 5)
    names = ["transformer_blocks.0.attn1.to_q.weight", "transformer_blocks.0.attn2.to_out.0.weight",
             "transformer_blocks.0.ff.net.2.weight", "proj_out.weight"]
    _follows(lambda: L.Transformer2DModel(8, 40, 320, 768), lambda m: m.run(x, 1, 8, 8, ctx, 78), names, dtype)


@DTYPES
def test_semantic_fusion_attention(dtype):
    x, e = _rand((80, 320), dtype, 6), _rand((77, 768), dtype, 7)
    _follows(lambda: txt_con_XFormersAttn(), lambda m: m.run(x, 1, 80, e, 77), ["to_k.weight"], dtype)


@DTYPES
def test_fp8_operands_follow(dtype):
    with torch.no_grad():
        lin = _module(lambda: L.Linear(640, 1920), dtype)
        attn = _module(lambda: L.Attention(640, None, 8, 80), dtype)
        attn.fp8_mfma = True
        old = [t.clone() for t in lin.w8p + attn._w8p_qkv()]
        lin.weight.mul_(0.5)
        attn.to_k.weight.mul_(0.5)
        new = lin.w8p + attn._w8p_qkv()
        want = ops.quantize_fp8_padded(lin.weight) \
            + ops.quantize_fp8_padded(torch.cat([attn.to_q.weight, attn.to_k.weight, attn.to_v.weight]))
        for n, w in zip(new, want):
            assert n.dtype == w.dtype and torch.equal(n.float(), w.float())
        # halving a row leaves its e4m3 codes as they are and halves its scale
        assert not torch.equal(new[1], old[1]) and not torch.equal(new[3], old[3])
        # and the projection runs on the new operand
        x, norm = _rand((80, 640), dtype, 8), _module(lambda: L.LayerNorm(640), dtype)
        a8, sa = ops.rowquant_fp8(x, (norm.weight, norm.bias, norm.eps))
        assert torch.equal(attn.project_qkv(x, norm), ops.gemm8(a8, sa, want[2], want[3], None, dtype=dtype))


@DTYPES
def test_a_capture_keeps_the_copy_it_was_warmed_up_with(dtype):
    with torch.no_grad():
        lin = _module(lambda: L.Linear(320, 320), dtype)
        x = _rand((80, 320), dtype, 9)
        kv = _rand((77, 640), dtype, 10)

        def run(wq):                 # dd_xattn320 streams the packed copy (the plain GEMM reads the live parameter)
            return ops.xattn320(x, wq, wq, lin.bias, kv[:, :320], kv[:, 320:], 1, 80, 77, 40 ** -0.5)
        graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run(lin.wx)                                                 # eager warm-up, on the stream of the capture
            lin.run(x)
            before = lin.wx
            assert before is lin.wx
            lin.weight.mul_(0.5)
            eager = run(before).clone()                                 # what the old buffer computes
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=side):
                during = lin.wx
                out = run(during)
                y = lin.run(x)
        torch.cuda.current_stream().wait_stream(side)
        assert during is before
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        assert torch.equal(y, ops.gemm(x, lin.w2d, lin.bias))           # w2d aliases the parameter: always current
        after = lin.wx
        assert after is not before and torch.equal(after, ops.xattn_pack_weight(lin.w2d))
        assert not torch.equal(after, before)
