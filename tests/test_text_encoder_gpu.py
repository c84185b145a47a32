"""CLIP text encoder on the HIP path: the embedding / pooling kernel bit for bit, the causal attention against an fp64
masked softmax, the mask bit-exactly, and the model against the CPU restatement (tests/clip_text_reference.py — parity
PINNED to transformers.CLIPTextModel by tests/golden/clip_text.npz, see tests/test_text_encoder_cpu.py).

Model rule, as for the other once-per-sample modules (tests/test_vae_gpu.py, tests/test_vae_encoder_gpu.py):
    e(HIP) <= max(1e-3, 1.5 * e_floor)
with e = rel-L2 against the fp32 restatement with the same dtype-rounded weights and e_floor the restatement's own error
under oracle.numerics.storage_emulation.  Every e(HIP) goes through parity_util.log_row into the parity CSV."""
import os
import types

import pytest
import torch

from oracle.init_utils import seeded_state_dict
from oracle.numerics import storage_emulation
from tests import clip_text_reference as RT
from tests import parity_util as PU
from tests.golden import cases as C
from tests.test_ops_gpu import TOL
from tests.test_parity_r02_gpu import _denoiser, _to_dev, step_models  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, os.cpu_count() or 1))

DTYPES = [torch.float16, torch.bfloat16]
HEADS, D = 12, 64
WIDTH = HEADS * D


@pytest.fixture(scope="module")
def ops(gpu):
    from dualdiff_amd import ops as O
    return O


def rnd(shape, dtype, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


# ---- 6. embeddings and the pooling position --------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_clip_embed_rows_and_argmax(ops, dtype):
    vocab, c = 49408, 768
    tok, pos = rnd((vocab, c), dtype, 1, 0.02).cuda(), rnd((77, c), dtype, 2, 0.02).cuda()
    for b, l, seed in ((2, 77, 5), (7, 33, 6), (1, 4, 7), (28, 77, 8), (3, 1, 9), (5, 70, 10)):
        ids = RT.seeded_ids(b, l, seed)
        if b >= 5:
            ids[1] = torch.randint(0, 40000, (l,), generator=torch.Generator().manual_seed(seed))   # no EOS at all
            ids[2, :] = 7                                                                            # every id the maximum
            ids[3, l // 2] = ids[3, l - 1] = 49407
            ids[3, l // 2 + 1:l - 1] = 11                                                            # two separated maxima
        rows, pool = ops.clip_embed(ids.cuda(), tok, pos, 2)
        assert rows.shape == (b * l, c) and rows.dtype == dtype and pool.shape == (b,) and pool.dtype == torch.int32
        want = (tok[ids.cuda()].float() + pos[:l].float()).to(dtype).reshape(b * l, c)
        assert torch.equal(rows, want), (b, l)
        assert torch.equal(pool.cpu().long(), ids.argmax(-1)), (b, l, pool.cpu(), ids.argmax(-1))
    assert (RT.seeded_ids(2, 77, 5) == 49407).sum(-1).max() > 1                 # repeated maxima were in the cases


@pytest.mark.parametrize("dtype", DTYPES)
def test_clip_embed_first_occurrence_rule_and_clamp(ops, dtype):
    vocab, c, l = 1000, 64, 40
    tok, pos = rnd((vocab, c), dtype, 3).cuda(), rnd((77, c), dtype, 4).cuda()
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, 900, (6, l), generator=g)
    eos = 950
    ids[0, 17] = ids[0, 30] = eos                    # first of two
    ids[1, 0] = eos                                   # at the start
    ids[2, l - 1] = eos                               # at the end
    ids[4, 5:] = eos                                  # a padded tail; rows 3 and 5: absent -> 0
    rows, pool = ops.clip_embed(ids.cuda(), tok, pos, eos)
    assert pool.cpu().tolist() == [17, 0, l - 1, 0, 5, 0]
    assert torch.equal(pool.cpu().long(), RT.pool_position(ids, eos))
    assert torch.equal(rows, (tok[ids.cuda()].float() + pos[:l].float()).to(dtype).reshape(-1, c))
    # ids outside [0, vocab) on the device: clamped, by value — -5 reads row 0 and 60000 reads row vocab - 1
    bad = ids.clone()
    bad[0, 3], bad[1, 7], bad[5, 39] = -5, 60000, -(2 ** 40)
    bad[3, 0] = 2 ** 40
    clamped = bad.clamp(0, vocab - 1)
    assert clamped[0, 3] == 0 and clamped[1, 7] == vocab - 1
    rows, pool = ops.clip_embed(bad.cuda(), tok, pos, 2)
    torch.cuda.synchronize()
    assert torch.equal(rows, (tok[clamped.cuda()].float() + pos[:l].float()).to(dtype).reshape(-1, c))
    assert torch.equal(rows[0 * l + 3], (tok[0].float() + pos[3].float()).to(dtype))
    assert torch.equal(rows[1 * l + 7], (tok[vocab - 1].float() + pos[7].float()).to(dtype))
    assert torch.equal(pool.cpu().long(), bad.argmax(-1))          # the pooling rule sees the ids as they are


# ---- 7. causal attention against fp64 ---------------------------------------------------------------------------------------

def causal_ref(qkv, b, l):
    """fp64 softmax_{j <= i}(q_i . k_j / 8) v_j from the fused (b*l, 2304) tensor -> (b*l, 768)."""
    x = qkv.double().cpu().view(b, l, 3, HEADS, D)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))                     # (b, h, l, d)
    s = q @ k.transpose(-1, -2) * D ** -0.5
    s = s.masked_fill(torch.ones((l, l), dtype=torch.bool).triu(1), float("-inf"))
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(b * l, WIDTH)


def check(y, ref, dtype, what):
    y = y.detach().double().cpu()
    assert y.shape == ref.shape and torch.isfinite(y).all(), what
    rel = ((y - ref).abs().max() / (ref.abs().max() + 1e-12)).item()
    print("%-44s rel-to-max=%.3e (bound %.3e)" % (what, rel, 4 * TOL[dtype]))
    assert rel <= 4 * TOL[dtype], "%s: %.3e > %.3e" % (what, rel, 4 * TOL[dtype])


def run_causal(ops, qkv, b, l, out=None):
    return ops.causal_attention(qkv[:, :WIDTH], qkv[:, WIDTH:2 * WIDTH], qkv[:, 2 * WIDTH:], b, l, HEADS, D, out=out)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b", [1, 7])
@pytest.mark.parametrize("l", [1, 2, 15, 16, 17, 33, 64, 76, 77])
def test_causal_attention_against_fp64(ops, l, b, dtype):
    qkv = rnd((b * l, 3 * WIDTH), dtype, 100 * l + b).cuda()
    out = torch.full((b * l, WIDTH), float("nan"), dtype=dtype, device="cuda")
    y = run_causal(ops, qkv, b, l, out=out)
    assert y.data_ptr() == out.data_ptr()
    check(y, causal_ref(qkv, b, l), dtype, "causal attention b=%d l=%d %s" % (b, l, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_causal_attention_capacity_and_spike(ops, dtype):
    """The stated capacity (128 tokens), and a key at j <= i that dominates its row (one at j > i must not)."""
    b, l = 2, ops.CAUSAL_ATTN_MAX_L
    qkv = rnd((b * l, 3 * WIDTH), dtype, 21).cuda()
    check(run_causal(ops, qkv, b, l), causal_ref(qkv, b, l), dtype, "causal attention capacity l=%d" % l)
    b, l = 2, 77
    qkv = rnd((b * l, 3 * WIDTH), dtype, 22).cuda()
    qkv[l + 40, WIDTH:2 * WIDTH] = qkv[l + 60, :WIDTH] * 4.0          # key 40 of sequence 1 dominates query 60 (and is masked for < 40)
    qkv[9, WIDTH:2 * WIDTH] = qkv[3, :WIDTH] * 4.0                    # key 9 of sequence 0 would dominate query 3: masked
    ref = causal_ref(qkv, b, l)
    y = run_causal(ops, qkv, b, l)
    check(y, ref, dtype, "causal attention spike")
    with pytest.raises(Exception, match="-2"):
        ops.causal_attention(qkv[:, :WIDTH], qkv[:, WIDTH:2 * WIDTH], qkv[:, 2 * WIDTH:], 1, 154, HEADS, D)
    with pytest.raises(Exception, match="-2"):
        ops.causal_attention(qkv[:, :960], qkv[:, 960:1920], qkv[:, 1344:], b, l, 24, 40)


# ---- 8. nothing leaks through the mask -------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("l", [77, 48])
def test_no_leak_through_the_mask(ops, dtype, l):
    b = 3
    qkv = rnd((b * l, 3 * WIDTH), dtype, 31).cuda()
    base = run_causal(ops, qkv, b, l).clone()
    for p in (1, 16, 17, 40):
        x = qkv.clone().view(b, l, 3 * WIDTH)
        sign = torch.where(rnd((b, l - p, 2 * WIDTH), dtype, 32 + p).cuda() >= 0, 1.0, -1.0).to(dtype)
        x[:, p:, WIDTH:] = sign * 1e4                              # K and V rows p .. l-1 of every sequence
        y = run_causal(ops, x.view(b * l, 3 * WIDTH), b, l).view(b, l, WIDTH)
        assert torch.isfinite(y[:, :p].float()).all(), p
        assert torch.equal(y[:, :p], base.view(b, l, WIDTH)[:, :p]), p
        assert not torch.equal(y[:, p:], base.view(b, l, WIDTH)[:, p:])


# ---- 9. model parity -------------------------------------------------------------------------------------------------------

CASES = [(2, 77, 201), (7, 33, 202), (1, 4, 203), (28, 77, 204)]
_REF = {}
_NETS = {}


def _restatement(dtype):
    if dtype not in _REF:
        ora = RT.CLIPTextModel().eval()
        sd = {k: v.to(dtype).float() for k, v in seeded_state_dict(ora, RT.GOLDEN_SEED).items()}
        ora.load_state_dict(sd)
        _REF[dtype] = (ora, sd, {})
    return _REF[dtype]


def _ref_outputs(dtype, ids, key):
    """(exact fp32, storage-emulated) outputs of the restatement with the dtype-rounded weights, cached per case."""
    ora, _, cache = _restatement(dtype)
    if key not in cache:
        with torch.no_grad():
            exact = ora(ids)
            with storage_emulation(ora, dtype):
                emul = ora(ids)
        cache[key] = (exact, emul)
    return cache[key]


def _hip(dtype):
    from dualdiff_amd.networks.text_encoder import CLIPTextModel
    if dtype not in _NETS:
        net = CLIPTextModel()
        net.load_state_dict(_restatement(dtype)[1])
        _NETS[dtype] = net.to("cuda", dtype).eval()
    return _NETS[dtype]


def _bound(name, y, ref, emul, dtype):
    e, fl = PU.rel_l2(y, ref), PU.rel_l2(emul, ref)
    b = max(1e-3, 1.5 * fl)
    print("%-40s %-8s e_hip=%.3e e_floor=%.3e ratio=%.3f bound=%.3e" % (name, str(dtype).split(".")[-1], e, fl,
                                                                       e / max(fl, 1e-30), b))
    PU.log_row(name, dtype, e, fl, b, PU.rel_l2(y, emul))
    assert torch.isfinite(y.float()).all(), name
    assert e <= b, (name, e, fl)
    return b


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=["%dx%d" % c[:2] for c in CASES])
def test_model_against_the_restatement(gpu, case, dtype):
    b, l, seed = case
    ids = RT.seeded_ids(b, l, seed)
    (ref_last, ref_pool), (em_last, em_pool) = _ref_outputs(dtype, ids, case)
    out = _hip(dtype)(ids.cuda())
    assert out.last_hidden_state.shape == (b, l, 768) and out.pooler_output.shape == (b, 768)
    assert out.last_hidden_state.dtype == dtype and out.pooler_output.dtype == dtype
    _bound("clip text last_hidden_state %dx%d" % (b, l), out.last_hidden_state, ref_last, em_last, dtype)
    _bound("clip text pooler_output %dx%d" % (b, l), out.pooler_output, ref_pool, em_pool, dtype)
    at = RT.pool_position(ids)
    assert torch.equal(out.pooler_output, out.last_hidden_state[torch.arange(b, device="cuda"), at.cuda()])


# ---- 10. outputs and encode_prompt_ids -------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_output_forms_and_encode_prompt_ids(gpu, dtype):
    from dualdiff_amd.networks.text_encoder import encode_prompt_ids
    net = _hip(dtype)
    b, l = 6, 33
    ids = RT.seeded_ids(b, l, 301)
    uncond = RT.seeded_ids(1, l, 302)
    uncond[0, 1:] = RT.EOS                                         # the empty caption: BOS, then EOS padding
    out = net(ids)                                                  # CPU ids: range-checked, then moved
    tup = net(ids.cuda(), return_dict=False)
    assert isinstance(tup, tuple) and len(tup) == 2
    assert torch.equal(out[0], out.last_hidden_state) and torch.equal(out[1], out.pooler_output)
    assert torch.equal(tup[0], out[0]) and torch.equal(tup[1], out[1])
    last, pooled = out
    assert last is out.last_hidden_state and pooled is out.pooler_output
    assert torch.equal(net(ids.to(torch.int32).cuda())[0], out[0])
    pe = encode_prompt_ids(net, ids.cuda(), uncond.cuda())
    assert pe.shape == (1 + b, l, 768) and pe.dtype == dtype
    # uncond rows first; the one forward equals the two separate forwards row for row within the model bound
    all_ids = torch.cat([uncond, ids])
    (ref_last, _), (em_last, _) = _ref_outputs(dtype, all_ids, ("prompt", b, l))
    bound = _bound("clip text encode_prompt_ids %dx%d" % (1 + b, l), pe, ref_last, em_last, dtype)
    sep = torch.cat([net(uncond.cuda())[0], out[0]])
    assert PU.rel_l2(pe, sep.float().cpu()) <= bound
    assert PU.rel_l2(pe[:1], ref_last[:1]) <= bound and PU.rel_l2(pe[1:], ref_last[1:]) <= bound
    assert PU.rel_l2(pe[:1], ref_last[1:2]) > 10 * bound            # the order is observable


# ---- 11. class tokens ------------------------------------------------------------------------------------------------------

class StubTokenizer:
    """Fixed unpadded ids of 3 to 6 tokens per class name (BOS, 1-4 word pieces, EOS), as CLIPTokenizer returns them with
    padding="do_not_pad"."""

    def __init__(self, names):
        g = torch.Generator().manual_seed(401)
        self.table = {}
        for i, n in enumerate(names):
            body = torch.randint(1000, 40000, (1 + i % 4,), generator=g)
            self.table[n] = torch.cat([torch.tensor([RT.BOS]), body, torch.tensor([RT.EOS])])[None]

    def __call__(self, texts, padding=None, return_tensors=None):
        assert padding == "do_not_pad" and return_tensors == "pt" and len(texts) == 1
        return types.SimpleNamespace(input_ids=self.table[texts[0]].clone())


@pytest.mark.parametrize("dtype", DTYPES)
def test_set_category_token(gpu, dtype):
    from dualdiff_amd.networks.bbox_embedder import ContinuousBBoxWithTextEmbedding
    names = ["car", "truck", "construction vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian",
             "traffic cone"]
    tok = StubTokenizer(names)
    assert sorted({t.shape[1] for t in tok.table.values()}) == [3, 4, 5, 6]
    emb = ContinuousBBoxWithTextEmbedding(n_classes=len(names)).to("cuda", dtype)
    emb.set_category_token(tok, _hip(dtype), names)
    # the same path through prepare(cfg, tokenizer=..., text_encoder=...)
    emb2 = ContinuousBBoxWithTextEmbedding(n_classes=len(names)).to("cuda", dtype)
    cfg = types.SimpleNamespace(dataset=types.SimpleNamespace(object_classes=names))
    emb2.prepare(cfg, tokenizer=tok, text_encoder=_hip(dtype))
    assert torch.equal(emb.class_tokens, emb2.class_tokens)
    for i, n in enumerate(names):
        ids = tok.table[n]
        (_, ref_pool), (_, em_pool) = _ref_outputs(dtype, ids, ("class", n))
        _bound("clip text class token %d (l=%d)" % (i, ids.shape[1]), emb.class_tokens[i][None], ref_pool, em_pool, dtype)


# ---- 12. prompt_embeds into the sampler ------------------------------------------------------------------------------------

def test_prompt_embeds_feed_the_sampler(step_models):  # noqa: F811
    from dualdiff_amd.networks.text_encoder import encode_prompt_ids
    from dualdiff_amd.pipeline.pipeline_bev_controlnet import BEVDenoiser
    dtype = torch.bfloat16
    l = C.STEP_LTXT
    ids, uncond = RT.seeded_ids(1, l, 501), RT.seeded_ids(1, l, 502)
    uncond[0, 1:] = RT.EOS
    pe = encode_prompt_ids(_hip(dtype), ids.cuda(), uncond.cuda())
    assert pe.shape == (2, l, 768) and pe.dtype == dtype
    d = _denoiser(step_models, dtype, use_graph=False)
    den = BEVDenoiser(d.unet, d.controlnets, guidance_scale=2.0, num_inference_steps=50, sampler="ddim")
    inp = C.step_inputs(2)
    with torch.no_grad():
        den.set_inputs(C.step_latents().cuda().to(dtype), pe, _to_dev(inp["camera_param"], dtype),
                       [_to_dev(inp["boxes_bg"], dtype), _to_dev(inp["boxes_fg"], dtype)],
                       [_to_dev(inp["cond_bg"], dtype), _to_dev(inp["cond_fg"], dtype)])
        before = den.latents.clone()
        den.run(1)
    assert torch.isfinite(den.latents.float()).all()
    assert not torch.equal(den.latents, before)
