"""CLIP text encoder on the HIP path — token ids to `prompt_embeds` and class tokens.

The reference's `text_encoder` is SD-v1.5's `transformers.CLIPTextModel` (openai/clip-vit-large-patch14 text tower):
`text_encoder(batch["input_ids"])[0]` / `text_encoder(batch["uncond_ids"])[0]` (runner/base_runner.py:511-514,
runner/multiview_runner.py:427-428), diffusers' `_encode_prompt` (pipeline/pipeline_bev_controlnet.py:273) and
`text_encoder(ids).pooler_output[0]` per class name (networks/bbox_embedder.py:133-145).  `CLIPTextModel` below carries
transformers' parameter names, so SD-v1.5's `text_encoder/pytorch_model.bin` loads with `load_state_dict`.

A layer is seven launches on the C-ABI:
  LayerNorm1 -> Q|K|V as ONE [2304][768] GEMM with the fused bias -> causal attention (ops.causal_attention,
  dd_causal_attention: head_dim 64, the fused projection's column slices read in place) -> out_proj + residual ->
  LayerNorm2 -> fc1 -> fc2 + residual.
quick_gelu has no kernel of its own: g * sigmoid(1.702 g) = silu(1.702 g) / 1.702, and dd_gemm computes
act(alpha * (A W^T + bias) + res).  fc1 runs with alpha = 1.702 and the SiLU epilogue and stores 1.702 * quick_gelu(g)
(the same relative rounding as storing quick_gelu(g)); fc2 runs with alpha = 1 / 1.702, the residual and a bias
pre-multiplied by 1.702 (computed in fp32, rounded once, cached with the packed weights).
The embeddings and the pooling position are one launch (ops.clip_embed, dd_clip_embed); a forward is 1 + 12 * 7 + 1
library launches and one torch row gather for pooler_output — no host synchronisation.

There is no tokenizer here: the interface starts at token ids.
"""
import types

import torch
import torch.nn as nn

from .. import ops as O
from .layers import LayerNorm, Linear, _Cached, derived

QUICK_GELU = 1.702
MAX_TOKENS = 77


class _Embedding(nn.Module):
    """nn.Embedding's parameter (`weight` (num, dim)); the gather itself is ops.clip_embed."""

    def __init__(self, num_embeddings, embedding_dim):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(num_embeddings, embedding_dim))


class CLIPTextEmbeddings(nn.Module):
    def __init__(self, vocab_size, hidden_size, max_position_embeddings):
        super().__init__()
        self.token_embedding = _Embedding(vocab_size, hidden_size)
        self.position_embedding = _Embedding(max_position_embeddings, hidden_size)


class CLIPAttention(_Cached):
    """q_proj / k_proj / v_proj stay separate parameters under transformers' names; the kernels see one fused projection."""

    NAMES = ("q_proj", "k_proj", "v_proj")

    def __init__(self, hidden_size, heads):
        super().__init__()
        self.heads, self.head_dim = heads, hidden_size // heads
        self.q_proj = Linear(hidden_size, hidden_size)
        self.k_proj = Linear(hidden_size, hidden_size)
        self.v_proj = Linear(hidden_size, hidden_size)
        self.out_proj = Linear(hidden_size, hidden_size)

    def _fused(self):
        ps = [getattr(self, n) for n in self.NAMES]
        return derived(self, "qkv", [p.weight for p in ps] + [p.bias for p in ps], lambda: (
            torch.cat([p.weight.detach() for p in ps], dim=0).contiguous(),
            torch.cat([p.bias.detach() for p in ps]).contiguous()))

    def run(self, h, res, batch, l):
        c = self.heads * self.head_dim
        w, b = self._fused()
        qkv = O.gemm(h, w, b)
        a = O.causal_attention(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], batch, l, self.heads, self.head_dim)
        return self.out_proj.run(a, res=res)


class CLIPMLP(_Cached):
    def __init__(self, hidden_size, intermediate_size):
        super().__init__()
        self.fc1 = Linear(hidden_size, intermediate_size)
        self.fc2 = Linear(intermediate_size, hidden_size)

    def _bias2(self):
        """fc2's bias times 1.702 (fp32 product, one rounding): what alpha = 1 / 1.702 turns back into the bias."""
        b = self.fc2.bias
        return derived(self, "b2", [b], lambda: (b.detach().float() * QUICK_GELU).to(b.dtype).contiguous())

    def run(self, h, res):
        g = self.fc1.run(h, alpha=QUICK_GELU, epilogue=O.DD_EPI_SILU)          # 1.702 * quick_gelu(fc1(h))
        return O.gemm(g, self.fc2.w2d, self._bias2(), res=res, alpha=1.0 / QUICK_GELU)


class CLIPEncoderLayer(nn.Module):
    def __init__(self, hidden_size, heads, intermediate_size, eps):
        super().__init__()
        self.self_attn = CLIPAttention(hidden_size, heads)
        self.layer_norm1 = LayerNorm(hidden_size, eps)
        self.mlp = CLIPMLP(hidden_size, intermediate_size)
        self.layer_norm2 = LayerNorm(hidden_size, eps)

    def run(self, x, batch, l):
        x = self.self_attn.run(self.layer_norm1.run(x), x, batch, l)
        return self.mlp.run(self.layer_norm2.run(x), x)


class CLIPEncoder(nn.Module):
    def __init__(self, hidden_size, heads, intermediate_size, num_layers, eps):
        super().__init__()
        self.layers = nn.ModuleList([CLIPEncoderLayer(hidden_size, heads, intermediate_size, eps)
                                     for _ in range(num_layers)])


class CLIPTextTransformer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.embeddings = CLIPTextEmbeddings(cfg.vocab_size, cfg.hidden_size, cfg.max_position_embeddings)
        self.encoder = CLIPEncoder(cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size,
                                   cfg.num_hidden_layers, cfg.layer_norm_eps)
        self.final_layer_norm = LayerNorm(cfg.hidden_size, cfg.layer_norm_eps)


class CLIPTextOutput:
    """`.last_hidden_state` (b, l, c), `.pooler_output` (b, c); `[0]` / `[1]` and unpacking as transformers' ModelOutput."""

    def __init__(self, last_hidden_state, pooler_output):
        self.last_hidden_state, self.pooler_output = last_hidden_state, pooler_output

    def to_tuple(self):
        return (self.last_hidden_state, self.pooler_output)

    def __getitem__(self, i):
        return self.to_tuple()[i]

    def __iter__(self):
        return iter(self.to_tuple())

    def __len__(self):
        return 2


_PREFIX = "text_model."


class CLIPTextModel(nn.Module):
    """transformers.CLIPTextModel for inference; the defaults are SD-v1.5's text_encoder/config.json."""

    def __init__(self, vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12,
                 num_attention_heads=12, max_position_embeddings=77, layer_norm_eps=1e-5, eos_token_id=2):
        super().__init__()
        if hidden_size % num_attention_heads or hidden_size % 8:
            raise ValueError("hidden_size must be a multiple of the head count and of 8")
        # no `use_attention_mask` attribute: diffusers' _encode_prompt probes it with hasattr and then passes no mask
        self.config = types.SimpleNamespace(
            vocab_size=vocab_size, hidden_size=hidden_size, intermediate_size=intermediate_size,
            num_hidden_layers=num_hidden_layers, num_attention_heads=num_attention_heads,
            max_position_embeddings=max_position_embeddings, hidden_act="quick_gelu", layer_norm_eps=layer_norm_eps,
            eos_token_id=eos_token_id)
        self.text_model = CLIPTextTransformer(self.config)

    @property
    def dtype(self):
        return self.text_model.final_layer_norm.weight.dtype

    @property
    def device(self):
        return self.text_model.final_layer_norm.weight.device

    # ---- checkpoints: transformers 4.x keys ("text_model." prefix, an int64 position_ids buffer) and 5.x keys (neither) ----
    def load_state_dict(self, state_dict, strict=True, **kw):
        prefixed = any(k.startswith(_PREFIX) for k in state_dict)
        sd, back = {}, {}
        for k, v in state_dict.items():
            if k.endswith("embeddings.position_ids"):
                continue                                   # arange(77): the kernel indexes the position table itself
            nk = k if prefixed else _PREFIX + k
            sd[nk] = v
            back[nk] = k
        res = super().load_state_dict(sd, strict=False, **kw)
        missing = [k if prefixed else k[len(_PREFIX):] for k in res.missing_keys]
        unexpected = [back.get(k, k) for k in res.unexpected_keys]
        if strict and (missing or unexpected):
            raise RuntimeError("Error(s) in loading state_dict for CLIPTextModel: missing keys %s, unexpected keys %s"
                               % (missing, unexpected))
        res.missing_keys[:] = missing
        res.unexpected_keys[:] = unexpected
        return res

    @torch.no_grad()
    def forward(self, input_ids, attention_mask=None, position_ids=None, output_attentions=None,
                output_hidden_states=None, return_dict=None):
        if attention_mask is not None:
            raise NotImplementedError("attention_mask: the reference passes none (SD-v1.5's text encoder has no "
                                      "use_attention_mask; runner/base_runner.py:511-514 calls text_encoder(ids))")
        if position_ids is not None:
            raise NotImplementedError("position_ids: the reference passes none (positions are 0 .. l-1)")
        if output_attentions:
            raise NotImplementedError("output_attentions: the reference reads [0] and pooler_output only")
        if output_hidden_states:
            raise NotImplementedError("output_hidden_states: the reference reads [0] and pooler_output only "
                                      "(no clip_skip)")
        cfg = self.config
        if not torch.is_tensor(input_ids) or input_ids.dim() != 2 or input_ids.is_floating_point() \
                or input_ids.dtype in (torch.bool,) or input_ids.is_complex():
            raise ValueError("input_ids must be an integer tensor (b, l), got %s"
                             % ((tuple(input_ids.shape), input_ids.dtype) if torch.is_tensor(input_ids) else type(input_ids),))
        b, l = input_ids.shape
        if b < 1 or l < 1 or l > min(cfg.max_position_embeddings, O.CAUSAL_ATTN_MAX_L):
            raise ValueError("input_ids must be (b >= 1, 1 <= l <= %d), got %s"
                             % (min(cfg.max_position_embeddings, O.CAUSAL_ATTN_MAX_L), tuple(input_ids.shape)))
        if not input_ids.is_cuda:
            lo, hi = int(input_ids.min()), int(input_ids.max())
            if lo < 0 or hi >= cfg.vocab_size:
                raise ValueError("token ids must lie in [0, %d), got [%d, %d]" % (cfg.vocab_size, lo, hi))
        if not self.device.type == "cuda":
            raise RuntimeError("the CLIP text encoder runs on the GPU only (model on %s); there is no CPU fallback"
                               % self.device)
        ids = input_ids.to(device=self.device, dtype=torch.int64).contiguous()   # GPU ids: the kernel clamps
        tm = self.text_model
        x, pool = O.clip_embed(ids, tm.embeddings.token_embedding.weight.detach(),
                               tm.embeddings.position_embedding.weight.detach(), cfg.eos_token_id)
        for layer in tm.encoder.layers:
            x = layer.run(x, b, l)
        x = tm.final_layer_norm.run(x)
        last = x.view(b, l, cfg.hidden_size)
        rows = torch.arange(b, device=x.device, dtype=torch.int64) * l + pool.long()
        pooled = x.index_select(0, rows)
        if return_dict is not None and not return_dict:
            return (last, pooled)
        return CLIPTextOutput(last, pooled)


@torch.no_grad()
def encode_prompt_ids(text_encoder, input_ids, uncond_ids):
    """runner/base_runner.py:511-514 (`text_encoder(batch["input_ids"])[0]`, `text_encoder(batch["uncond_ids"])[0]`) as
    the `prompt_embeds` BEVDenoiser.set_inputs takes: (b_uncond + b, l, c) with the UNCONDITIONAL rows first.  The
    reference's collate function pads both to one length (dataset/utils.py:30-57, :515-518), and this is then ONE forward
    over cat([uncond_ids, input_ids]).  Ids of two different lengths would need two forwards whose results cannot share a
    tensor: that is a ValueError here, before anything runs."""
    if input_ids.dim() != 2 or uncond_ids.dim() != 2:
        raise ValueError("input_ids and uncond_ids must be (b, l) tensors")
    if input_ids.shape[1] != uncond_ids.shape[1]:
        raise ValueError("uncond_ids (l = %d) and input_ids (l = %d) give embeddings of different lengths, which cannot "
                         "be stacked into one prompt_embeds tensor: pad both to one length as the reference's collate "
                         "function does" % (uncond_ids.shape[1], input_ids.shape[1]))
    return text_encoder(torch.cat([uncond_ids.to(input_ids.device), input_ids], dim=0))[0]
