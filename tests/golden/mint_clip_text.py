"""Mints tests/golden/clip_text.npz: what `transformers.CLIPTextModel` — the library the reference's `text_encoder` comes
from — computes for the seeded weights and ids of tests/clip_text_reference.py.  TEST INFRASTRUCTURE; runs only where
`transformers` is importable (CPU, fp32).  The weights are regenerated from the seed and never stored: the fixture holds
the ids and, per case, `last_hidden_state` and `pooler_output` in fp32.

    python tests/golden/mint_clip_text.py

This PINS the restatement's parity: tests/test_text_encoder_cpu.py requires tests/clip_text_reference.py to reproduce
these arrays (rel-L2 < 1e-4, the cross-host rule of parity_util.oracle_cache).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))

from oracle.init_utils import seeded_state_dict                # noqa: E402
from tests import clip_text_reference as RT                    # noqa: E402


def main():
    import transformers
    from transformers import CLIPTextConfig, CLIPTextModel
    torch.manual_seed(0)
    ours = RT.CLIPTextModel().eval()
    sd = seeded_state_dict(ours, RT.GOLDEN_SEED)
    cfg = CLIPTextConfig(vocab_size=RT.SIZES["vocab_size"], hidden_size=RT.SIZES["hidden_size"],
                         intermediate_size=RT.SIZES["intermediate_size"],
                         num_hidden_layers=RT.SIZES["num_hidden_layers"],
                         num_attention_heads=RT.SIZES["num_attention_heads"],
                         max_position_embeddings=RT.SIZES["max_position_embeddings"],
                         layer_norm_eps=RT.SIZES["layer_norm_eps"], hidden_act="quick_gelu", eos_token_id=2,
                         bos_token_id=0, pad_token_id=1)
    lib = CLIPTextModel(cfg).eval()
    want = lib.state_dict()
    # transformers 4.x names its parameters text_model.*, 5.x drops the prefix; position_ids is a buffer of the former
    load = {}
    for k, v in sd.items():
        name = k if k in want else k[len("text_model."):]
        assert name in want and want[name].shape == v.shape, k
        load[name] = v
    res = lib.load_state_dict(load, strict=False)
    assert not res.unexpected_keys and all(k.endswith("position_ids") for k in res.missing_keys), res
    out = {}
    with torch.no_grad():
        for b, l, seed in RT.GOLDEN_CASES:
            ids = RT.seeded_ids(b, l, seed)
            y = lib(input_ids=ids)
            tag = "%dx%d" % (b, l)
            out["ids_" + tag] = ids.numpy()
            out["last_hidden_state_" + tag] = y.last_hidden_state.float().numpy()
            out["pooler_output_" + tag] = y.pooler_output.float().numpy()
    path = os.path.join(HERE, "clip_text.npz")
    np.savez_compressed(path, **out)
    print("transformers %s -> %s (%d bytes)" % (transformers.__version__, path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
