"""CLIP text encoder, everything that needs no GPU: the restatement against the transformers-minted fixture, the HIP model's
checkpoint surface and argument checks, and the new entry points' validation in the built library."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle.init_utils import seeded_state_dict
from tests import clip_text_reference as RT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_num_threads(min(16, os.cpu_count() or 1))

SMALL = dict(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1,
             max_position_embeddings=77)


def rel_l2(y, ref):
    return ((y.double() - ref.double()).norm() / (ref.double().norm() + 1e-30)).item()


# ---- 1. the restatement reproduces transformers.CLIPTextModel -----------------------------------------------------------

@pytest.fixture(scope="module")
def restatement():
    m = RT.CLIPTextModel().eval()
    m.load_state_dict(seeded_state_dict(m, RT.GOLDEN_SEED))
    return m


@pytest.mark.parametrize("case", RT.GOLDEN_CASES, ids=["%dx%d" % c[:2] for c in RT.GOLDEN_CASES])
def test_restatement_reproduces_transformers(restatement, case):
    """tests/golden/clip_text.npz was computed by transformers.CLIPTextModel (tests/golden/mint_clip_text.py) from the same
    seeded weights: parity of the restatement is pinned to the library the reference calls.  1e-4 is the project's
    cross-host rule for stored oracle outputs (parity_util.oracle_cache)."""
    b, l, seed = case
    tag = "%dx%d" % (b, l)
    with np.load(os.path.join(ROOT, "tests", "golden", "clip_text.npz")) as z:
        ids = torch.from_numpy(z["ids_" + tag])
        want_last = torch.from_numpy(z["last_hidden_state_" + tag])
        want_pool = torch.from_numpy(z["pooler_output_" + tag])
    assert torch.equal(ids, RT.seeded_ids(b, l, seed))
    with torch.no_grad():
        last, pooled = restatement(ids)
    e_last, e_pool = rel_l2(last, want_last), rel_l2(pooled, want_pool)
    print("\n[clip restatement %s] e_last=%.2e e_pool=%.2e" % (tag, e_last, e_pool))
    assert last.shape == want_last.shape == (b, l, 768) and pooled.shape == want_pool.shape == (b, 768)
    assert e_last < 1e-4 and e_pool < 1e-4


def test_fixture_has_a_repeated_maximum():
    """At least one fixture sequence ends in repeated 49407 padding, so pooling must take the FIRST maximum — and the pooled
    row of the fixture is that position's hidden state, not the last one's."""
    with np.load(os.path.join(ROOT, "tests", "golden", "clip_text.npz")) as z:
        ids = torch.from_numpy(z["ids_2x77"])
        last = torch.from_numpy(z["last_hidden_state_2x77"])
        pooled = torch.from_numpy(z["pooler_output_2x77"])
    n_max = (ids == ids.max(dim=-1, keepdim=True).values).sum(dim=-1)
    assert (n_max > 1).any()
    for i in range(ids.shape[0]):
        first = int((ids[i] == RT.EOS).nonzero()[0])
        assert first == int(RT.pool_position(ids)[i])
        assert torch.equal(pooled[i], last[i, first])
        if n_max[i] > 1:
            assert not torch.equal(pooled[i], last[i, -1])


# ---- 2. checkpoint surface -----------------------------------------------------------------------------------------------

def _hip_model(**kw):
    from dualdiff_amd.networks.text_encoder import CLIPTextModel
    return CLIPTextModel(**kw)


def test_state_dict_matches_the_restatement():
    ours, ref = _hip_model(), RT.CLIPTextModel()
    a, b = ours.state_dict(), ref.state_dict()
    assert list(a) == list(b) or sorted(a) == sorted(b)
    assert {k: tuple(v.shape) for k, v in a.items()} == {k: tuple(v.shape) for k, v in b.items()}
    assert all(k.startswith("text_model.") for k in a) and len(a) == 2 + 12 * 16 + 2
    cfg = ours.config
    assert (cfg.vocab_size, cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads,
            cfg.max_position_embeddings, cfg.hidden_act, cfg.layer_norm_eps, cfg.eos_token_id) == \
        (49408, 768, 3072, 12, 12, 77, "quick_gelu", 1e-5, 2)
    assert not hasattr(cfg, "use_attention_mask")


def test_both_key_layouts_load():
    ref = RT.CLIPTextModel(**SMALL)
    sd = seeded_state_dict(ref, 3)
    # transformers 4.x: prefixed, with the int64 position_ids buffer
    v4 = dict(sd)
    v4["text_model.embeddings.position_ids"] = torch.arange(77).unsqueeze(0)
    m4 = _hip_model(**SMALL)
    r = m4.load_state_dict(v4)
    assert not r.missing_keys and not r.unexpected_keys
    # transformers 5.x: no prefix, no position_ids
    v5 = {k[len("text_model."):]: v for k, v in sd.items()}
    m5 = _hip_model(**SMALL)
    r = m5.load_state_dict(v5)
    assert not r.missing_keys and not r.unexpected_keys
    for m in (m4, m5):
        got = m.state_dict()
        assert sorted(got) == sorted(sd)
        for k in sd:
            assert torch.equal(got[k], sd[k]), k
    # an unknown key is reported (strict: raised), a missing one as well
    for layout in (v4, v5):
        bad = dict(layout)
        bad["bogus.weight"] = torch.zeros(1)
        r = _hip_model(**SMALL).load_state_dict(bad, strict=False)
        assert r.unexpected_keys == ["bogus.weight"] and not r.missing_keys
        with pytest.raises(RuntimeError, match="bogus.weight"):
            _hip_model(**SMALL).load_state_dict(bad)
    short = {k: v for k, v in v5.items() if k != "final_layer_norm.bias"}
    r = _hip_model(**SMALL).load_state_dict(short, strict=False)
    assert r.missing_keys == ["final_layer_norm.bias"]
    with pytest.raises(RuntimeError, match="final_layer_norm.bias"):
        _hip_model(**SMALL).load_state_dict(short)


def test_caches_drop_on_load_and_to():
    m = _hip_model(**SMALL)
    m.load_state_dict(seeded_state_dict(RT.CLIPTextModel(**SMALL), 3))
    layer = m.text_model.encoder.layers[0]
    w, b = layer.self_attn._fused()
    assert tuple(w.shape) == (192, 64) and tuple(b.shape) == (192,)
    assert torch.equal(w[64:128], layer.self_attn.k_proj.weight) and torch.equal(b[128:], layer.self_attn.v_proj.bias)
    b2 = layer.mlp._bias2()
    assert torch.equal(b2, (layer.mlp.fc2.bias.float() * 1.702).to(b2.dtype))
    assert "_pk_qkv" in layer.self_attn.__dict__ and "_pk_b2" in layer.mlp.__dict__
    m.to(torch.float16)
    assert "_pk_qkv" not in layer.self_attn.__dict__ and "_pk_b2" not in layer.mlp.__dict__
    assert m.dtype == torch.float16 and m.device.type == "cpu"
    h = layer.mlp._bias2()
    assert h.dtype == torch.float16 and torch.equal(h, (layer.mlp.fc2.bias.float() * 1.702).half())
    layer.self_attn._fused()
    m.load_state_dict(m.state_dict())
    assert "_pk_qkv" not in layer.self_attn.__dict__ and "_pk_b2" not in layer.mlp.__dict__
    assert m.eval() is m and m.requires_grad_(False) is m


# ---- 3. argument checks --------------------------------------------------------------------------------------------------

def test_forward_argument_checks():
    m = _hip_model(**SMALL)
    ids = torch.zeros((2, 5), dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="attention_mask"):
        m(ids, attention_mask=torch.ones(2, 5))
    with pytest.raises(NotImplementedError, match="position_ids"):
        m(ids, position_ids=torch.arange(5)[None])
    with pytest.raises(NotImplementedError, match="output_attentions"):
        m(ids, output_attentions=True)
    with pytest.raises(NotImplementedError, match="output_hidden_states"):
        m(ids, output_hidden_states=True)
    with pytest.raises(ValueError, match="integer tensor"):
        m(torch.zeros((2, 5)))
    with pytest.raises(ValueError, match="integer tensor"):
        m(torch.zeros((5,), dtype=torch.int64))
    with pytest.raises(ValueError, match="1 <= l <= 77"):
        m(torch.zeros((1, 78), dtype=torch.int64))
    with pytest.raises(ValueError, match="1 <= l <= 77"):
        m(torch.zeros((1, 0), dtype=torch.int64))
    with pytest.raises(ValueError, match=r"token ids must lie in \[0, 64\)"):
        m(torch.full((1, 4), 64, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"token ids must lie in \[0, 64\)"):
        m(torch.tensor([[3, -1]]))
    with pytest.raises(RuntimeError, match="GPU only"):
        m(ids)                                       # a model that is not on the GPU
    with pytest.raises(RuntimeError, match="GPU only"):
        m(ids.to(torch.int32), output_attentions=False, output_hidden_states=False, return_dict=True)


def test_ops_fail_loudly_on_cpu_tensors():
    from dualdiff_amd import ops
    x = torch.zeros((4, 192), dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.causal_attention(x[:, :64], x[:, 64:128], x[:, 128:], 1, 4, 1, 64)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.clip_embed(torch.zeros((1, 4), dtype=torch.int64), torch.zeros((8, 64), dtype=torch.float16),
                       torch.zeros((4, 64), dtype=torch.float16), 2)


def test_encode_prompt_ids_checks_lengths():
    from dualdiff_amd.networks.text_encoder import encode_prompt_ids
    m = _hip_model(**SMALL)
    with pytest.raises(ValueError, match="different lengths"):
        encode_prompt_ids(m, torch.zeros((6, 9), dtype=torch.int64), torch.zeros((1, 7), dtype=torch.int64))


# ---- 4. the built library ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from dualdiff_amd import _build, _native
    if not os.path.exists(_build.lib_path()):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _native.load(build_if_missing=False)


def _causal(lib, q=1 << 20, k=1 << 20, v=1 << 20, o=1 << 20, ld=2304, ldo=768, bs=None, batch=2, l=77, heads=12,
            head_dim=64, dtype=0):
    bs = l * ld if bs is None else bs
    return lib.dd_causal_attention(q, k, v, o, ld, ld, ld, ldo, bs, bs, bs, l * ldo, batch, l, heads, head_dim, 0.125,
                                   dtype, None)


def test_library_exports_and_validates_causal_attention(lib):
    from dualdiff_amd import _native, ops
    assert hasattr(lib, "dd_causal_attention") and hasattr(lib, "dd_clip_embed")
    assert lib.dd_abi_version() == 4 and lib.dd_desc_size(99) == -1
    assert ops.CAUSAL_ATTN_MAX_L >= 77
    hdr = open(os.path.join(ROOT, "include", "dualdiff_hip.h")).read()
    assert "#define DD_CAUSAL_ATTN_MAX_L %d" % ops.CAUSAL_ATTN_MAX_L in hdr
    # every rejection below happens before any launch: there is no GPU here and the pointers are not memory
    for null in ("q", "k", "v", "o"):
        assert _causal(lib, **{null: None}) == -1
    assert _causal(lib, head_dim=40) == -2 and _causal(lib, head_dim=128) == -2
    assert _causal(lib, l=0) == -1 and _causal(lib, batch=0) == -1 and _causal(lib, heads=0) == -1
    assert _causal(lib, l=ops.CAUSAL_ATTN_MAX_L + 1) == -2
    assert _causal(lib, q=(1 << 20) + 8) == -1 and _causal(lib, o=(1 << 20) + 2) == -1       # misaligned
    assert _causal(lib, ld=2300) == -1 and _causal(lib, bs=77 * 2304 + 4) == -1               # strides % 8
    assert _causal(lib, dtype=2) == -1
    # dd_attention keeps refusing head_dim 64: the causal kernel is a separate entry point
    a = _native.AttnDesc()
    a.q = a.k = a.v = a.o = 16
    a.batch, a.heads, a.head_dim, a.lq, a.lk = 1, 8, 64, 4, 4
    a.ldq = a.ldk = a.ldv = a.ldo = 512
    assert lib.dd_attention(ctypes.byref(a), None) == -2


def test_library_validates_clip_embed(lib):
    P = 1 << 20

    def call(ids=P, tok=P, pos=P, out=P, pool=P, batch=2, l=77, c=768, vocab=49408, dtype=0):
        return lib.dd_clip_embed(ids, tok, pos, out, pool, batch, l, c, vocab, 2, dtype, None)

    for null in ("ids", "tok", "pos", "out", "pool"):
        assert call(**{null: None}) == -1
    assert call(c=772) == -1 and call(c=0) == -1                      # c % 8
    assert call(batch=0) == -1 and call(l=0) == -1 and call(vocab=0) == -1
    assert call(tok=P + 8) == -1 and call(pos=P + 2) == -1 and call(out=P + 4) == -1 and call(ids=P + 4) == -1
    assert call(pool=P + 2) == -1
    assert call(dtype=3) == -1
