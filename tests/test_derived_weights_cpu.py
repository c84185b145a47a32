"""layers.derived — the one cache rule for kernel-layout copies of parameters — and every site that goes through it, on CPU
tensors: pure torch, no library call.  A site FOLLOWS its parameters when, after an in-place update of each of them in turn,
the derived value equals (torch.equal) what a freshly constructed module gives after load_state_dict of the updated state."""
import pytest
import torch
import torch.nn as nn

from dualdiff_amd.networks import layers as L
from dualdiff_amd.networks.blocks import BasicMultiviewTransformerBlock
from dualdiff_amd.networks.box_adapter import Adapter_XFormersAttnProcessor
from dualdiff_amd.networks.text_encoder import CLIPMLP, CLIPAttention
from dualdiff_amd.networks.txt_con_fusion import txt_con_XFormersAttn
from dualdiff_amd.networks.vae_decoder import AutoencoderKLDecoder
from dualdiff_amd.networks.vae_encoder import AutoencoderKLEncoder


# ---- 1. the helper ---------------------------------------------------------------------------------------------------------

class _Counter:
    def __init__(self, p):
        self.p, self.calls = p, 0

    def __call__(self):
        self.calls += 1
        assert not torch.is_grad_enabled()
        return self.p.detach() * 3


def test_builds_once_and_rebuilds_after_an_update():
    h, p = L._Cached(), nn.Parameter(torch.arange(4.0))
    build = _Counter(p)
    v = L.derived(h, "x", [p], build)
    assert torch.equal(v, torch.arange(4.0) * 3) and build.calls == 1
    assert L.derived(h, "x", [p], build) is v and build.calls == 1
    assert "_pk_x" in h.__dict__
    with torch.no_grad():
        p.mul_(2)
    v2 = L.derived(h, "x", [p], build)
    assert v2 is not v and torch.equal(v2, torch.arange(4.0) * 6) and build.calls == 2
    p.data = p.data.clone()                                   # a new address under the same counter
    v3 = L.derived(h, "x", [p], build)
    assert v3 is not v2 and torch.equal(v3, v2) and build.calls == 3
    assert L.derived(h, "x", [p], build) is v3 and build.calls == 3


def test_none_and_inference_parameters():
    h, p = L._Cached(), nn.Parameter(torch.ones(3))
    build = _Counter(p)
    v = L.derived(h, "x", [p, None], build)
    assert L.derived(h, "x", [p, None], build) is v and build.calls == 1
    assert L.derived(h, "x", [None, p], build) is not v and build.calls == 2      # the order is part of the key
    with torch.inference_mode():
        q = nn.Parameter(torch.ones(3), requires_grad=False)
    with pytest.raises(RuntimeError):
        q._version
    build = _Counter(q)
    v = L.derived(h, "y", [q], build)
    assert L.derived(h, "y", [q], build) is v and build.calls == 1


def test_slots_keep_entries_apart():
    h, p = L._Cached(), nn.Parameter(torch.ones(3))
    a = L.derived(h, "s", [p], lambda: p.detach() * 2, slot=(4, 7))
    b = L.derived(h, "s", [p], lambda: p.detach() * 5, slot=(7, 13))
    assert L.derived(h, "s", [p], None, slot=(4, 7)) is a and L.derived(h, "s", [p], None, slot=(7, 13)) is b
    assert torch.equal(a, torch.full((3,), 2.0)) and torch.equal(b, torch.full((3,), 5.0))
    assert set(h.__dict__["_pk_s"]) == {(4, 7), (7, 13)}


def test_a_capture_keeps_a_stale_entry_and_builds_a_missing_one(monkeypatch):
    h, p = L._Cached(), nn.Parameter(torch.ones(3))
    build = _Counter(p)
    v = L.derived(h, "x", [p], build)
    with torch.no_grad():
        p.mul_(2)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    assert L.derived(h, "x", [p], build) is v and build.calls == 1            # stale: returned as it is
    assert torch.equal(v, torch.full((3,), 3.0))
    w = L.derived(h, "z", [p], build)                                         # missing: built
    assert build.calls == 2 and torch.equal(w, torch.full((3,), 6.0))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    v2 = L.derived(h, "x", [p], build)
    assert v2 is not v and build.calls == 3 and torch.equal(v2, w)


def test_drop_cache_forgets_the_entry_and_bumps_the_epoch():
    h, other, p = L._Cached(), L._Cached(), nn.Parameter(torch.ones(3))
    L.derived(h, "x", [p], lambda: p.detach() * 2)
    L.derived(h, "s", [p], lambda: p.detach() * 2, slot=1)
    L.derived(other, "x", [p], lambda: p.detach() * 2)
    epoch = L.CACHE_EPOCH[0]
    with torch.no_grad():
        p.mul_(2)
    L.derived(h, "x", [p], lambda: p.detach() * 2)                            # a rebuild is no drop: the epoch stays
    assert L.CACHE_EPOCH[0] == epoch
    h._drop_cache()
    assert L.CACHE_EPOCH[0] == epoch + 1
    assert not [k for k in h.__dict__ if k.startswith("_pk_")] and "_pk_x" in other.__dict__


# ---- 2. every site ---------------------------------------------------------------------------------------------------------

def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def _copy(a):
    """Values, not views: some derived tensors alias the live parameter."""
    if torch.is_tensor(a):
        return a.clone()
    return tuple(_copy(x) for x in a) if isinstance(a, (tuple, list)) else a


def _mv_block(kind):
    return lambda: BasicMultiviewTransformerBlock(64, 2, 32, cross_attention_dim=24, neighboring_view_pair={0: [1], 1: [0]},
                                                  zero_module_type=kind)


def _ln_pair():
    return nn.ModuleDict({"norm": L.LayerNorm(64), "lin": L.Linear(64, 128)})


def _resnets():
    return nn.ModuleList([L.ResnetBlock2D(32, 32, 16), L.ResnetBlock2D(32, 64, 16)])


def _blocks():
    return nn.ModuleList([L.BasicTransformerBlock(64, 2, 32, cross_attention_dim=24) for _ in range(2)])


def _kv_bank(m):
    bank = L.CrossKVBank(m)
    mods = bank.banked(24)
    assert len(mods) == 2
    return bank, mods


QKV, KV = ("to_q", "to_k", "to_v"), ("to_k", "to_v")

# (id, make module, value(module, state), source parameter names, state(module) or None)
SITES = [
    ("linear_w2d", lambda: L.Linear(189, 320), lambda m, s: m.w2d, ["weight"], None),
    ("linear_w2d_alias", lambda: L.Linear(320, 320), lambda m, s: m.w2d, ["weight"], None),
    ("conv_packed", lambda: L.Conv3x3(8, 16), lambda m, s: m.packed, ["weight"], None),
    ("conv_packed_padded", lambda: L.Conv3x3(4, 16), lambda m, s: m.packed, ["weight"], None),
    ("conv_folded_up", lambda: L.Conv3x3(64, 64), lambda m, s: m.folded_up(4, 7, (7, 13)), ["weight"], None),
    ("attention_kv", lambda: L.Attention(320, 768, 8, 40), lambda m, s: m._fused(KV), ["to_k.weight", "to_v.weight"], None),
    ("attention_qkv", lambda: L.Attention(64, None, 2, 32, bias=True), lambda m, s: (m._fused(QKV), m._fused_bias(QKV)),
     ["to_q.weight", "to_k.weight", "to_v.weight", "to_q.bias", "to_k.bias", "to_v.bias"], None),
    ("clip_attention", lambda: CLIPAttention(64, 2), lambda m, s: m._fused(),
     ["q_proj.weight", "k_proj.weight", "v_proj.weight", "q_proj.bias", "k_proj.bias", "v_proj.bias"], None),
    ("clip_mlp", lambda: CLIPMLP(64, 128), lambda m, s: m._bias2(), ["fc2.bias"], None),
    ("vae_pq", lambda: AutoencoderKLDecoder(block_out_channels=(32,)), lambda m, s: m._pq(),
     ["post_quant_conv.weight", "post_quant_conv.bias"], None),
    ("vae_q32", lambda: AutoencoderKLEncoder(block_out_channels=(32,)), lambda m, s: m._q(),
     ["quant_conv.weight", "quant_conv.bias"], None),
    ("adapter", lambda: Adapter_XFormersAttnProcessor(320, 768),
     lambda m, s: (m._fused("to_k_box", "to_v_box"), m._fused("to_k_cls", "to_v_cls")),
     ["to_k_box.weight", "to_v_box.weight", "to_k_cls.weight", "to_v_cls.weight"], None),
    ("sfa", lambda: txt_con_XFormersAttn(), lambda m, s: m._fused(), ["to_k.weight", "to_v.weight"], None),
    ("folded_out_zero_linear", _mv_block("zero_linear"), lambda m, s: (m._folded_out(1), m._folded_out(2)),
     ["attn4.to_out.0.weight", "attn4.to_out.0.bias", "connector.weight", "connector.bias"], None),
    ("folded_out_gated", _mv_block("gated"), lambda m, s: (m._folded_out(1), m._folded_out(2)),
     ["attn4.to_out.0.weight", "attn4.to_out.0.bias", "connector.alpha"], None),
    ("folded_out_none", _mv_block("none"), lambda m, s: (m._folded_out(1), m._folded_out(2)),
     ["attn4.to_out.0.weight", "attn4.to_out.0.bias"], None),
    ("folded_ff_out", lambda: L.Transformer2DModel(2, 32, 64, 24), lambda m, s: m._folded_ff_out(m.transformer_blocks[0]),
     ["transformer_blocks.0.ff.net.2.weight", "transformer_blocks.0.ff.net.2.bias", "proj_out.weight", "proj_out.bias"], None),
    ("fold_layernorm", _ln_pair,
     lambda m, s: L.fold_layernorm(m["lin"], "ln", m["norm"], [m["lin"].weight], [m["lin"].bias]),
     ["norm.weight", "norm.bias", "lin.weight", "lin.bias"], None),
    ("temb_bank", _resnets, lambda m, s: s.stacked(),
     ["0.time_emb_proj.weight", "1.time_emb_proj.weight", "0.time_emb_proj.bias", "1.time_emb_proj.bias"], L.TimeEmbProjBank),
    ("kv_bank", _blocks, lambda m, s: s[0].stacked(s[1]),
     ["0.attn2.to_k.weight", "0.attn2.to_v.weight", "1.attn2.to_k.weight", "1.attn2.to_v.weight"], _kv_bank),
]


@pytest.mark.parametrize("site", SITES, ids=[s[0] for s in SITES])
def test_site_follows_in_place_updates(site):
    _, make, value, sources, state = site
    mod = L.seeded_init_(make(), 5)
    st = None if state is None else state(mod)
    prev = _copy(value(mod, st))
    assert _same(value(mod, st), prev)
    for name in sources:
        with torch.no_grad():
            mod.get_parameter(name).mul_(0.5)
        got = value(mod, st)
        assert not _same(got, prev), name                        # the parameter is a source of the value
        fresh = make()
        fresh.load_state_dict(mod.state_dict())
        assert _same(got, value(fresh, None if state is None else state(fresh))), name
        prev = _copy(got)


def test_unpadded_w2d_is_a_view_of_the_parameter():
    lin = L.seeded_init_(L.Linear(320, 320))
    assert lin.w2d.data_ptr() == lin.weight.data_ptr() and lin.w2d is lin.w2d
    conv = L.seeded_init_(L.Linear(64, 32, conv=True))
    assert conv.w2d.data_ptr() == conv.weight.data_ptr() and tuple(conv.w2d.shape) == (32, 64)
    assert L.seeded_init_(L.Linear(189, 320)).w2d.shape == (320, 192)


def test_fold_layernorm_sums_the_rounded_matrix():
    m = L.seeded_init_(_ln_pair(), 2).to(torch.bfloat16)
    wp, (colsum, lnb, eps) = L.fold_layernorm(m["lin"], "ln", m["norm"], [m["lin"].weight], [m["lin"].bias])
    assert wp.dtype == torch.bfloat16 and colsum.dtype == lnb.dtype == torch.float32 and eps == m["norm"].eps
    assert torch.equal(colsum, wp.float().sum(dim=1))
    assert "_pk_ln" in m["lin"].__dict__


@pytest.mark.parametrize("make,value", [
    (lambda: Adapter_XFormersAttnProcessor(320, 768), lambda m: m._fused("to_k_box", "to_v_box")),
    (lambda: txt_con_XFormersAttn(), lambda m: m._fused())], ids=["adapter", "sfa"])
def test_processors_drop_their_entries_on_half_and_load(make, value):
    mod = L.seeded_init_(make())
    value(mod)
    assert [k for k in mod.__dict__ if k.startswith("_pk_")]
    epoch = L.CACHE_EPOCH[0]
    mod.half()
    assert not [k for k in mod.__dict__ if k.startswith("_pk_")] and L.CACHE_EPOCH[0] > epoch
    assert value(mod).dtype == torch.float16
    mod.load_state_dict(mod.state_dict())
    assert not [k for k in mod.__dict__ if k.startswith("_pk_")]


def test_model_invalidate_forgets_the_banks():
    from dualdiff_amd.networks.model_base import ModelBase

    class Tiny(ModelBase):
        def __init__(self):
            super().__init__()
            self._register_config()
            self.resnets = _resnets()

    m = L.seeded_init_(Tiny())
    bank = m.temb_bank
    w, b = bank.stacked()
    assert m.temb_bank is bank and tuple(w.shape) == (96, 16) and tuple(b.shape) == (96,)
    m._invalidate()
    assert m.temb_bank is not bank
