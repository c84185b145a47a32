"""CPU restatement of the SD-v1.5 text encoder (`transformers.CLIPTextModel`) — TEST INFRASTRUCTURE ONLY.

The reference calls it as `text_encoder(ids)[0]` (runner/base_runner.py:511-514, runner/multiview_runner.py:427-428,
diffusers' `_encode_prompt` at pipeline/pipeline_bev_controlnet.py:273) and `text_encoder(ids).pooler_output[0]`
(networks/bbox_embedder.py:133-145).  The model is not in the reference's tree: it comes from `transformers`.

PARITY PINNED — unlike the VAE restatements (oracle/vae_decoder.py, tests/vae_encoder_reference.py): tests/golden/
clip_text.npz holds what `transformers.CLIPTextModel` itself computes for this module's seeded weights and ids
(tests/golden/mint_clip_text.py), and tests/test_text_encoder_cpu.py requires this restatement to reproduce it.

Written from the model's formula, with transformers' module and parameter names (so `oracle.init_utils.seeded_state_dict`
gives the HIP model and this one the same weights):
    x = token_embedding[ids] + position_embedding[0:l]
    12 x:  h = LayerNorm1(x);  q, k, v = h Wq^T + bq, h Wk^T + bk, h Wv^T + bv  (12 heads x 64)
           x = x + softmax_{j <= i}(q_i . k_j / 8) v  Wo^T + bo
           g = fc1(LayerNorm2(x));  x = x + fc2(g * sigmoid(1.702 g))
    last_hidden_state = final_layer_norm(x);  pooler_output[b] = last_hidden_state[b, ids[b].argmax()]  (eos_token_id 2;
    any other eos_token_id: the first position holding it).
Padding is not masked (SD-v1.5 has no use_attention_mask).  Under `oracle.numerics.storage_emulation` the module
boundaries round to the storage dtype; `prob_round` (P before P.V) and `stor` (the embedding sum, the two residual adds,
the quick_gelu product) mark the functional results an fp16 run rounds as well, so the emulation is the storage floor.
"""
import torch
import torch.nn as nn

from oracle.numerics import prob_round, stor

SIZES = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
             max_position_embeddings=77, layer_norm_eps=1e-5, eos_token_id=2)
BOS, EOS = 49406, 49407


class CLIPTextEmbeddings(nn.Module):
    def __init__(self, vocab_size, hidden_size, max_position_embeddings):
        super().__init__()
        self.token_embedding = nn.Embedding(vocab_size, hidden_size)
        self.position_embedding = nn.Embedding(max_position_embeddings, hidden_size)

    def forward(self, ids):
        return stor(self.token_embedding(ids) + self.position_embedding.weight[:ids.shape[1]])


_FUTURE = {}


def future_mask(l, device):
    """(l, l) bool, True where key j > query i; built once per (l, device), as transformers builds its mask once per forward."""
    key = (l, str(device))
    if key not in _FUTURE:
        _FUTURE[key] = torch.ones((l, l), dtype=torch.bool, device=device).triu(1)
    return _FUTURE[key]


class CLIPAttention(nn.Module):
    def __init__(self, hidden_size, heads):
        super().__init__()
        self.heads = heads
        self.q_proj = nn.Linear(hidden_size, hidden_size)
        self.k_proj = nn.Linear(hidden_size, hidden_size)
        self.v_proj = nn.Linear(hidden_size, hidden_size)
        self.out_proj = nn.Linear(hidden_size, hidden_size)

    def forward(self, h):
        b, l, c = h.shape
        d = c // self.heads

        def split(t):
            return t.view(b, l, self.heads, d).transpose(1, 2)

        q, k, v = split(self.q_proj(h)), split(self.k_proj(h)), split(self.v_proj(h))
        scores = torch.matmul(q, k.transpose(-1, -2)).float() * d ** -0.5
        p = prob_round(scores.masked_fill(future_mask(l, h.device), float("-inf")).softmax(dim=-1)).to(v.dtype)
        return self.out_proj(torch.matmul(p, v).transpose(1, 2).reshape(b, l, c))


class CLIPMLP(nn.Module):
    def __init__(self, hidden_size, intermediate_size):
        super().__init__()
        self.fc1 = nn.Linear(hidden_size, intermediate_size)
        self.fc2 = nn.Linear(intermediate_size, hidden_size)

    def forward(self, h):
        g = self.fc1(h)
        return self.fc2(stor(g * torch.sigmoid(1.702 * g)))


class CLIPEncoderLayer(nn.Module):
    def __init__(self, hidden_size, heads, intermediate_size, eps):
        super().__init__()
        self.self_attn = CLIPAttention(hidden_size, heads)
        self.layer_norm1 = nn.LayerNorm(hidden_size, eps=eps)
        self.mlp = CLIPMLP(hidden_size, intermediate_size)
        self.layer_norm2 = nn.LayerNorm(hidden_size, eps=eps)

    def forward(self, x):
        x = stor(x + self.self_attn(self.layer_norm1(x)))
        return stor(x + self.mlp(self.layer_norm2(x)))


class CLIPEncoder(nn.Module):
    def __init__(self, hidden_size, heads, intermediate_size, num_layers, eps):
        super().__init__()
        self.layers = nn.ModuleList([CLIPEncoderLayer(hidden_size, heads, intermediate_size, eps)
                                     for _ in range(num_layers)])

    def forward(self, x):
        for layer in self.layers:
            x = layer(x)
        return x


class CLIPTextTransformer(nn.Module):
    def __init__(self, vocab_size, hidden_size, intermediate_size, num_hidden_layers, num_attention_heads,
                 max_position_embeddings, layer_norm_eps, eos_token_id):
        super().__init__()
        self.eos_token_id = eos_token_id
        self.embeddings = CLIPTextEmbeddings(vocab_size, hidden_size, max_position_embeddings)
        self.encoder = CLIPEncoder(hidden_size, num_attention_heads, intermediate_size, num_hidden_layers, layer_norm_eps)
        self.final_layer_norm = nn.LayerNorm(hidden_size, eps=layer_norm_eps)

    def forward(self, ids):
        last = self.final_layer_norm(self.encoder(self.embeddings(ids)))
        if self.eos_token_id == 2:
            at = ids.argmax(dim=-1)
        else:
            at = (ids == self.eos_token_id).int().argmax(dim=-1)
        return last, last[torch.arange(ids.shape[0], device=ids.device), at]


class CLIPTextModel(nn.Module):
    """forward(ids (b, l) int64) -> (last_hidden_state (b, l, c), pooler_output (b, c))."""

    def __init__(self, **sizes):
        super().__init__()
        self.text_model = CLIPTextTransformer(**{**SIZES, **sizes})

    def forward(self, ids):
        return self.text_model(ids)


def pool_position(ids, eos_token_id=2):
    """The position pooler_output reads from, per sequence."""
    if eos_token_id == 2:
        return ids.argmax(dim=-1)
    return (ids == eos_token_id).int().argmax(dim=-1)


def seeded_ids(b, l, seed):
    """(b, l) int64 prompts: BOS first, random ids in [0, 49406), EOS (49407, the largest id and the padding id) from a
    random position >= 1 to the end — so wherever that position is not the last one, argmax must take the FIRST of several
    equal maxima.  l = 1 is BOS alone."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, BOS, (b, l), generator=g, dtype=torch.int64)
    ids[:, 0] = BOS
    if l > 1:
        eos = torch.randint(1, l, (b,), generator=g)
        for i in range(b):
            ids[i, int(eos[i]):] = EOS
    return ids


# the seeded cases of tests/golden/clip_text.npz: (b, l, ids seed); weights: seeded_state_dict(CLIPTextModel(), GOLDEN_SEED)
GOLDEN_SEED = 7
GOLDEN_CASES = [(2, 77, 101), (3, 33, 102), (1, 4, 103)]
