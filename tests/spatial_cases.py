"""Spatial-module cases with a per-pixel and a per-channel error metric — a helper of tests/test_spatial_metric_cpu.py and
tests/test_spatial_blocks_gpu.py, not a test itself.  The block-switch work (tests/block_cases.py) restated for the modules
that own image borders, instance boundaries, strides, resizes and the never-materialised concat: the resnet, the down /
mid / up blocks of networks/layers.py and the VAE blocks of networks/vae_decoder.py and vae_encoder.py.

A case pairs an oracle module (oracle/diffusers_restated.py, oracle/vae_decoder.py, tests/vae_encoder_reference.py) with
the HIP module: seeded_state_dict rounded to bf16 loaded into both, inputs rounded to bf16, so that one CPU run is the
exact-weight reference of the fp16 and of the bf16 HIP run.  References, computed on the CPU once per case:
    ref[out]          the oracle module in float64;
    emul[dtype][out]  the same module under storage_emulation(dtype): ONE realisation of the storage dtype's rounding noise.
EVERY tensor a block returns is an output (`outputs_of`): each skip of a down block beside its result, a resnet with and
without extra_res, the encoder's moments beside its latents.  Outputs are (pixels, C) rows in NHWC order — the layout
run() returns; the two NCHW results (the decoder image, the encoder latents) are permuted to it.

The cases are the smallest shapes at which each path is still the one taken.  Unless noted m = 3, so that two instance
boundaries fall at row counts no tile divides; every instance has its own inputs and its own time vector.

Metrics of an output y (pixels, C) against ref, and the conditions on a HIP output (`conditions`):
    1. e(y)           <= max(1e-3, 1.02 e(emul))              whole tensor (parity_util.bound, unchanged)
    2. max_p e_pix(y) <= max(1e-3, M_pix max_p e_pix(emul))   worst pixel:   e_pix[p] = ||y_p - ref_p|| / ||ref_p||
    3. max_c e_ch(y)  <= max(1e-3, M_ch  max_c e_ch(emul))    worst channel: block_cases.e_ch
e_pix is block_cases.e_tok on pixel rows (pooled in groups of POOL[case] consecutive rows).  An output NARROWER than 32
channels — the decoder image (3) and the encoder's moments (8) and latents (4) — has pixels whose own norm is next to zero,
where a relative error says nothing; there e_pix[p] = ||y_p - ref_p|| / (sqrt(C) rms(ref)), rms over the whole output, so
that a pixel is measured against the typical pixel norm (`e_pix`).

Margins, as in block_cases: max_p e_pix(emul) is the largest of `pixels` noisy values of one realisation of rounding
noise.  emul is evaluated for N_SEEDS input seeds per case and dtype on ONE CPU thread; per output M = (largest over
seeds) / (smallest over seeds) x FLOOR_SLACK, rounded UP to two significant digits, and the case's margin is the largest
over its outputs.  `python -m tests.spatial_cases --margins` recomputes and prints the table below and exits non-zero when
it differs; no HIP code takes part.  A case whose pixel margin exceeds 2 pools its pixels in groups of 16 (POOL).
"""
import copy
import os
import sys

import torch
import torch.nn.functional as F

if __name__ == "__main__":                                 # `python tests/spatial_cases.py` as well as `-m tests.spatial_cases`
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import diffusers_restated as D  # noqa: E402
from oracle import vae_decoder as V  # noqa: E402
from oracle.init_utils import seeded_state_dict, seeded_tensor  # noqa: E402
from oracle.numerics import stor, storage_emulation  # noqa: E402
from tests import vae_encoder_reference as E  # noqa: E402
from tests.block_cases import DTYPES, bf16_round, e_ch, e_tok, round_up_2sig, tag  # noqa: E402
from tests.parity_util import FLOOR_SLACK, bound, rel_l2  # noqa: E402

LC, CTX_DIM, TEMB, HEADS = 13, 768, 1280, 8
N_SEEDS = 8                                # input seeds of the margin measurement; seed 0 is the one the tests run
NARROW = 32                                # outputs with fewer channels take the rms-normalised e_pix

# name: kind, instances, (h, w) of the input, weight seed, and what the kind needs:
#   R     cin = (c1, c2 or 0: the x2 source), cout                      -> out, out_res (extra_res added)
#   DB    cross, cin, cout, down                                        -> skip0, skip1[, skip2], out
#   MID   c                                                             -> out (with extra_res)
#   UB    cross, cin (skip of the last resnet), cout, prev, up_size     -> out
#   VR    cin, cout;  VMID c;  VUP cin, cout;  VDOWN cin, cout          -> out
#   VDEC  z (m, 4, h, w) -> image;  VENC  x (m, 3, h, w) -> moments, mode
CASES = {
    "R320":         dict(kind="R", m=3, hw=(5, 7), wseed=51, cin=(320, 0), cout=320),
    "R320_640":     dict(kind="R", m=3, hw=(5, 7), wseed=52, cin=(320, 0), cout=640),
    "Rcat960":      dict(kind="R", m=3, hw=(5, 7), wseed=53, cin=(640, 320), cout=320),
    "Rcat2560":     dict(kind="R", m=3, hw=(4, 7), wseed=54, cin=(1280, 1280), cout=1280),
    "DB640":        dict(kind="DB", m=2, hw=(7, 9), wseed=55, cross=True, cin=320, cout=640, down=True),
    "DB1280":       dict(kind="DB", m=3, hw=(4, 7), wseed=56, cross=False, cin=1280, cout=1280, down=False),
    "MID":          dict(kind="MID", m=2, hw=(4, 7), wseed=57, c=1280),
    "UB1280":       dict(kind="UB", m=2, hw=(4, 7), wseed=58, cross=False, cin=1280, cout=1280, prev=1280, up_size=(7, 13)),
    "CUB640":       dict(kind="UB", m=2, hw=(8, 8), wseed=59, cross=True, cin=320, cout=640, prev=1280, up_size=None),
    "VR256_128":    dict(kind="VR", m=3, hw=(6, 10), wseed=60, cin=256, cout=128),
    "VMID":         dict(kind="VMID", m=2, hw=(5, 8), wseed=61, c=512),
    "VMID5x7":      dict(kind="VMID", m=2, hw=(5, 7), wseed=61, c=512),          # 35 tokens: not a multiple of 8
    "VUP512_256":   dict(kind="VUP", m=2, hw=(3, 4), wseed=62, cin=512, cout=256),
    "VDOWN128_256": dict(kind="VDOWN", m=2, hw=(6, 10), wseed=63, cin=128, cout=256),
    "VDEC":         dict(kind="VDEC", m=2, hw=(3, 5), wseed=64),                  # 15 tokens in the mid block
    "VENC":         dict(kind="VENC", m=2, hw=(24, 40), wseed=65),
}

# ---- measured margins (python -m tests.spatial_cases --margins) --------------------------------------------------
# case: {dtype: (M_pix, M_ch)}; POOL[case] = pixel rows per group of e_pix (1: every pixel on its own).
#   worst-pixel / worst-channel floors behind them, max_p e_pix(emul) and max_c e_ch(emul), smallest .. largest over
#   the 8 seeds and the case's outputs (--margins --floors reprints them):
# R320          float16 pix 3.9e-04..4.4e-04 ch 4.1e-04..4.9e-04  bfloat16 pix 3.1e-03..3.6e-03 ch 3.5e-03..3.9e-03
# R320_640      float16 pix 4.0e-04..4.7e-04 ch 4.4e-04..5.6e-04  bfloat16 pix 3.4e-03..3.9e-03 ch 3.8e-03..4.6e-03
# Rcat960       float16 pix 4.1e-04..4.9e-04 ch 4.5e-04..5.3e-04  bfloat16 pix 3.4e-03..4.0e-03 ch 3.8e-03..4.4e-03
# Rcat2560      float16 pix 3.9e-04..4.5e-04 ch 4.8e-04..5.9e-04  bfloat16 pix 3.3e-03..3.7e-03 ch 4.0e-03..4.7e-03
# DB640         float16 pix 7.8e-04..1.1e-03 ch 9.1e-04..1.9e-03  bfloat16 pix 6.2e-03..8.4e-03 ch 7.3e-03..1.4e-02
# DB1280        float16 pix 4.0e-04..5.4e-04 ch 4.7e-04..7.4e-04  bfloat16 pix 3.2e-03..4.4e-03 ch 3.9e-03..5.9e-03
# MID           float16 pix 7.1e-04..7.3e-04 ch 9.5e-04..1.1e-03  bfloat16 pix 5.8e-03..6.1e-03 ch 8.1e-03..9.5e-03
# UB1280        float16 pix 6.2e-04..6.5e-04 ch 8.0e-04..9.1e-04  bfloat16 pix 5.0e-03..5.1e-03 ch 6.4e-03..7.4e-03
# CUB640        float16 pix 1.2e-03..1.3e-03 ch 1.4e-03..1.5e-03  bfloat16 pix 9.4e-03..9.8e-03 ch 1.1e-02..1.2e-02
# VR256_128     float16 pix 4.9e-04..5.2e-04 ch 4.5e-04..4.9e-04  bfloat16 pix 4.0e-03..4.3e-03 ch 3.7e-03..4.2e-03
# VMID          float16 pix 6.3e-04..6.8e-04 ch 7.5e-04..8.1e-04  bfloat16 pix 5.1e-03..5.6e-03 ch 6.1e-03..7.0e-03
# VMID5x7       float16 pix 6.2e-04..7.6e-04 ch 7.6e-04..8.7e-04  bfloat16 pix 5.0e-03..5.4e-03 ch 6.3e-03..6.7e-03
# VUP512_256    float16 pix 7.2e-04..7.9e-04 ch 8.6e-04..1.1e-03  bfloat16 pix 6.1e-03..6.5e-03 ch 7.6e-03..8.3e-03
# VDOWN128_256  float16 pix 6.3e-04..6.9e-04 ch 8.8e-04..1.2e-03  bfloat16 pix 4.9e-03..5.8e-03 ch 7.0e-03..9.2e-03
# VDEC          float16 pix 4.0e-03..5.2e-03 ch 1.4e-03..1.7e-03  bfloat16 pix 2.9e-02..3.7e-02 ch 1.1e-02..1.4e-02
# VENC          float16 pix 2.2e-03..3.5e-03 ch 1.5e-03..2.7e-03  bfloat16 pix 1.6e-02..2.5e-02 ch 1.2e-02..2.3e-02
MARGINS = {
    "R320":         {"float16": (1.1, 1.2), "bfloat16": (1.2, 1.1)},
    "R320_640":     {"float16": (1.1, 1.2), "bfloat16": (1.1, 1.2)},
    "Rcat960":      {"float16": (1.1, 1.2), "bfloat16": (1.2, 1.2)},
    "Rcat2560":     {"float16": (1.1, 1.2), "bfloat16": (1.1, 1.2)},
    "DB640":        {"float16": (1.2, 1.4), "bfloat16": (1.2, 1.3)},
    "DB1280":       {"float16": (1.1, 1.2), "bfloat16": (1.1, 1.2)},
    "MID":          {"float16": (1.1, 1.3), "bfloat16": (1.1, 1.2)},
    "UB1280":       {"float16": (1.1, 1.2), "bfloat16": (1.1, 1.2)},
    "CUB640":       {"float16": (1.2, 1.2), "bfloat16": (1.1, 1.2)},
    "VR256_128":    {"float16": (1.1, 1.1), "bfloat16": (1.2, 1.2)},
    "VMID":         {"float16": (1.2, 1.2), "bfloat16": (1.2, 1.2)},
    "VMID5x7":      {"float16": (1.3, 1.2), "bfloat16": (1.1, 1.1)},
    "VUP512_256":   {"float16": (1.2, 1.4), "bfloat16": (1.1, 1.2)},
    "VDOWN128_256": {"float16": (1.2, 1.5), "bfloat16": (1.3, 1.4)},
    "VDEC":         {"float16": (1.4, 1.3), "bfloat16": (1.3, 1.4)},
    "VENC":         {"float16": (1.4, 1.9), "bfloat16": (1.6, 1.9)},
}
POOL = {"R320": 1, "R320_640": 1, "Rcat960": 1, "Rcat2560": 1, "DB640": 1, "DB1280": 1, "MID": 1, "UB1280": 1, "CUB640": 1, "VR256_128": 1, "VMID": 1, "VMID5x7": 1, "VUP512_256": 1, "VDOWN128_256": 1, "VDEC": 1, "VENC": 1}


def outputs_of(name):
    c = CASES[name]
    if c["kind"] == "R":
        return ["out", "out_res"]
    if c["kind"] == "DB":
        return ["skip%d" % i for i in range(2 + c["down"])] + ["out"]
    if c["kind"] == "VENC":
        return ["moments", "mode"]
    return ["out"]


def rows_nhwc(t):
    """(m, C, h, w) -> (m * h * w, C) pixel rows."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def out_hw(name):
    """{output: (m, h, w)}: where a row of the output lies."""
    c = CASES[name]
    m, (h, w), k = c["m"], c["hw"], c["kind"]
    if k == "DB":
        d = {o: (m, h, w) for o in outputs_of(name)}
        if c["down"]:
            d["skip2"] = d["out"] = (m, (h - 1) // 2 + 1, (w - 1) // 2 + 1)
        return d
    if k == "UB":
        return {"out": (m,) + tuple(c["up_size"] or (2 * h, 2 * w))}
    if k == "VUP":
        return {"out": (m, 2 * h, 2 * w)}
    if k == "VDOWN":
        return {"out": (m, h // 2, w // 2)}
    if k == "VDEC":
        return {"out": (m, 8 * h, 8 * w)}
    if k == "VENC":
        return {o: (m, h // 8, w // 8) for o in outputs_of(name)}
    return {o: (m, h, w) for o in outputs_of(name)}


# ---- the oracle side ---------------------------------------------------------------------------------------------
def build_oracle(name):
    c = CASES[name]
    k = c["kind"]
    if k == "R":
        return D.ResnetBlock2D(in_channels=sum(c["cin"]), out_channels=c["cout"], temb_channels=TEMB, eps=1e-5)
    if k == "DB" and c["cross"]:
        return D.CrossAttnDownBlock2D(c["cin"], c["cout"], TEMB, num_layers=2, resnet_eps=1e-5, attn_num_head_channels=HEADS,
                                      cross_attention_dim=CTX_DIM, add_downsample=c["down"])
    if k == "DB":
        return D.DownBlock2D(c["cin"], c["cout"], TEMB, num_layers=2, resnet_eps=1e-5, add_downsample=c["down"])
    if k == "MID":
        return D.UNetMidBlock2DCrossAttn(c["c"], TEMB, resnet_eps=1e-5, attn_num_head_channels=HEADS, cross_attention_dim=CTX_DIM)
    if k == "UB" and c["cross"]:
        return D.CrossAttnUpBlock2D(c["cin"], c["cout"], c["prev"], TEMB, num_layers=3, resnet_eps=1e-5,
                                    attn_num_head_channels=HEADS, cross_attention_dim=CTX_DIM, add_upsample=True)
    if k == "UB":
        return D.UpBlock2D(c["cin"], c["prev"], c["cout"], TEMB, num_layers=3, resnet_eps=1e-5, add_upsample=True)
    if k == "VR":
        return D.ResnetBlock2D(in_channels=c["cin"], out_channels=c["cout"], temb_channels=None, eps=1e-6)
    if k == "VMID":
        return V.MidBlock(c["c"], 1e-6)
    if k == "VUP":
        return V.UpDecoderBlock(c["cin"], c["cout"], True, 1e-6)
    if k == "VDOWN":
        return E.DownEncoderBlock2D(c["cin"], c["cout"], True, 1e-6)
    if k == "VDEC":
        return V.AutoencoderKLDecoder()
    if k == "VENC":
        return E.AutoencoderKLEncoder()
    raise KeyError(k)


def make_oracle(name):
    """(oracle module in fp32 with its bf16-rounded seeded weights, that state dict)."""
    ora = build_oracle(name).eval()
    sd = {k: bf16_round(v) for k, v in seeded_state_dict(ora, CASES[name]["wseed"]).items()}
    ora.load_state_dict(sd)
    return ora, sd


def make_inputs(name, seed=0):
    """{key: bf16-rounded fp32 tensor, "skips": [..]}: NCHW activations, (m, 1280) time embedding, (m, LC, 768) context."""
    c = CASES[name]
    k, m, (h, w) = c["kind"], c["m"], c["hw"]
    base = [1000 * c["wseed"] + 20 * seed]

    def t(*shape, scale=1.0):
        base[0] += 1
        return bf16_round(seeded_tensor(shape, base[0], scale))
    if k == "R":
        c1, c2 = c["cin"]
        return {"x": t(m, c1, h, w), "x2": t(m, c2, h, w) if c2 else None, "emb": t(m, TEMB), "er": t(m, c["cout"], h, w)}
    if k == "DB":
        return {"x": t(m, c["cin"], h, w), "emb": t(m, TEMB), "ctx": t(m, LC, CTX_DIM)}
    if k == "MID":
        return {"x": t(m, c["c"], h, w), "emb": t(m, TEMB), "ctx": t(m, LC, CTX_DIM), "er": t(m, c["c"], h, w)}
    if k == "UB":                                  # skips in the order the down path pushed them: the LAST is popped first
        return {"x": t(m, c["prev"], h, w), "emb": t(m, TEMB), "ctx": t(m, LC, CTX_DIM),
                "skips": [t(m, ch, h, w) for ch in (c["cin"], c["cout"], c["cout"])]}
    if k in ("VR", "VUP", "VDOWN"):
        return {"x": t(m, c["cin"], h, w)}
    if k == "VMID":
        return {"x": t(m, c["c"], h, w)}
    if k == "VDEC":
        return {"x": t(m, 4, h, w, scale=3.0)}
    return {"x": bf16_round(t(m, 3, h, w, scale=0.5).clamp(-1.0, 1.0))}


def to_double(inp):
    return {k: (None if v is None else [s.double() for s in v] if isinstance(v, list) else v.double()) for k, v in inp.items()}


def run_oracle(name, ora, inp):
    """{output: (pixels, C) rows} of the oracle module (fp32, float64, or inside storage_emulation)."""
    c = CASES[name]
    k = c["kind"]
    with torch.no_grad():
        if k == "R":
            x = inp["x"] if inp["x2"] is None else torch.cat([inp["x"], inp["x2"]], dim=1)
            o = ora(x, inp["emb"])
            return {"out": rows_nhwc(o), "out_res": rows_nhwc(stor(o + inp["er"]))}
        if k == "DB":
            o, outs = ora(inp["x"], inp["emb"], encoder_hidden_states=inp["ctx"]) if c["cross"] else ora(inp["x"], inp["emb"])
            d = {"skip%d" % i: rows_nhwc(s) for i, s in enumerate(outs)}
            d["out"] = rows_nhwc(o)
            return d
        if k == "MID":
            return {"out": rows_nhwc(stor(ora(inp["x"], inp["emb"], encoder_hidden_states=inp["ctx"]) + inp["er"]))}
        if k == "UB":
            kw = {"encoder_hidden_states": inp["ctx"]} if c["cross"] else {}
            return {"out": rows_nhwc(ora(inp["x"], tuple(inp["skips"]), inp["emb"], upsample_size=c["up_size"], **kw))}
        if k == "VR":
            return {"out": rows_nhwc(ora(inp["x"], None))}
        if k in ("VMID", "VUP", "VDOWN"):
            return {"out": rows_nhwc(ora(inp["x"]))}
        if k == "VDEC":
            return {"out": rows_nhwc(ora.decode(inp["x"]))}
        mom = ora.encoder(inp["x"])                # conv_out's rows: what the HIP latent_dist holds as `moments`
        return {"moments": rows_nhwc(mom), "mode": rows_nhwc(E.posterior(ora.quant_conv(mom)))}


def run_emul(name, ora, inp, dtype):
    with storage_emulation(ora, dtype):
        return run_oracle(name, ora, inp)


def oracle_outputs(name, seed=0, ora_sd=None):
    """{"sd", "inp", "ref": {output: float64 rows}, "emul": {dtype: {output: fp32 rows}}} of one case."""
    ora, sd = ora_sd or make_oracle(name)
    inp = make_inputs(name, seed)
    ref = run_oracle(name, copy.deepcopy(ora).double(), to_double(inp))
    return {"sd": sd, "inp": inp, "ref": ref, "emul": {dt: run_emul(name, ora, inp, dt) for dt in DTYPES}}


# ---- the HIP side ------------------------------------------------------------------------------------------------
def build_hip(name):
    from dualdiff_amd.networks import layers as L, vae_decoder as VD, vae_encoder as VE
    c = CASES[name]
    k = c["kind"]
    if k == "R":
        return L.ResnetBlock2D(sum(c["cin"]), c["cout"], TEMB)
    if k == "DB" and c["cross"]:
        return L.CrossAttnDownBlock2D(c["cin"], c["cout"], TEMB, 2, HEADS, CTX_DIM, c["down"])
    if k == "DB":
        return L.DownBlock2D(c["cin"], c["cout"], TEMB, 2, c["down"])
    if k == "MID":
        return L.UNetMidBlock2DCrossAttn(c["c"], TEMB, HEADS, CTX_DIM)
    if k == "UB" and c["cross"]:
        return L.CrossAttnUpBlock2D(c["cin"], c["cout"], c["prev"], TEMB, 3, HEADS, CTX_DIM, True)
    if k == "UB":
        return L.UpBlock2D(c["cin"], c["prev"], c["cout"], TEMB, 3, True)
    if k == "VR":
        return VD.VaeResnetBlock2D(c["cin"], c["cout"])
    if k == "VMID":
        return VD.VaeMidBlock(c["c"], 1e-6)
    if k == "VUP":
        return VD.UpDecoderBlock2D(c["cin"], c["cout"], True, 1e-6)
    if k == "VDOWN":
        return VE.DownEncoderBlock2D(c["cin"], c["cout"], True, 1e-6)
    if k == "VDEC":
        return VD.AutoencoderKLDecoder()
    return VE.AutoencoderKLEncoder()


def make_hip(name, sd, dtype):
    blk = build_hip(name)
    blk.load_state_dict(sd, strict=True)
    return blk.to("cuda", dtype).eval()


def hip_inputs(name, inp, dtype):
    """Device tensors in the layout run() takes: (pixels, C) rows, (m, 1280) embedding, (m * LC, 768) context; the two
    whole networks take NCHW."""
    whole = CASES[name]["kind"] in ("VDEC", "VENC")

    def dev(key, v):
        if v is None:
            return None
        if isinstance(v, list):
            return [dev(key, s) for s in v]
        if key == "ctx":
            v = v.reshape(-1, CTX_DIM)
        elif v.dim() == 4 and not whole:
            v = rows_nhwc(v)
        return v.contiguous().cuda().to(dtype)
    return {k: dev(k, v) for k, v in inp.items()}


def run_hip(name, blk, d):
    """{output: (pixels, C) device rows} of one run of the HIP module on the device inputs `d` of hip_inputs."""
    from dualdiff_amd import ops as O
    from dualdiff_amd.networks import layers as L
    c = CASES[name]
    k, m, (h, w) = c["kind"], c["m"], c["hw"]
    with torch.no_grad():
        if k in ("R", "DB", "MID", "UB"):
            temb = L.TimeEmbProjBank(blk).run(O.silu(d["emb"]))
        if k == "R":
            return {"out": blk.run(d["x"], m, h, w, temb[id(blk)], x2=d["x2"]),
                    "out_res": blk.run(d["x"], m, h, w, temb[id(blk)], x2=d["x2"], extra_res=d["er"])}
        if k == "DB":
            x, _h, _w, skips = L.run_down_block(blk, d["x"], m, h, w, temb, d.get("ctx"), LC)
            o = {"skip%d" % i: s[0] for i, s in enumerate(skips)}
            o["out"] = x
            return o
        if k == "MID":
            return {"out": blk.run(d["x"], m, h, w, temb, d["ctx"], LC, extra_res=d["er"])}
        if k == "UB":
            skips = [(s, h, w) for s in d["skips"]]
            return {"out": L.run_up_block(blk, d["x"], m, h, w, skips, temb, d.get("ctx"), LC, c["up_size"])[0]}
        if k in ("VR", "VMID"):
            return {"out": blk.run(d["x"], m, h, w)}
        if k in ("VUP", "VDOWN"):
            return {"out": blk.run(d["x"], m, h, w)[0]}
        if k == "VDEC":
            return {"out": rows_nhwc(blk.decode(d["x"]))}
        dist = blk.encode(d["x"]).latent_dist
        return {"moments": dist.moments, "mode": rows_nhwc(dist.mode())}


# ---- metrics -----------------------------------------------------------------------------------------------------
def e_pix(y, ref, pool=1):
    """Relative L2 error of every pixel row (of every group of `pool` consecutive rows): block_cases.e_tok, and for an
    output narrower than NARROW channels the error of the row over sqrt(C) x rms(ref), i.e. over the typical row norm."""
    if ref.shape[1] >= NARROW:
        return e_tok(y, ref, pool)
    y, ref = y.detach().cpu().double(), ref.detach().cpu().double()
    d2 = ((y - ref) ** 2).sum(dim=1)
    n = torch.ones_like(d2)
    if pool > 1:
        pad = (-d2.numel()) % pool
        d2 = F.pad(d2, (0, pad)).reshape(-1, pool).sum(dim=1)
        n = F.pad(n, (0, pad)).reshape(-1, pool).sum(dim=1)
    return (d2 / (n * ref.shape[1] * (ref ** 2).mean() + 1e-300)).sqrt()


def conditions(name, dtype, y, ref, emul, margins=None, pool=None):
    """-> {"e": (value, bound), "pix": (value, bound), "ch": (value, bound)} of ONE output: conditions 1-3 above."""
    m_pix, m_ch = (MARGINS[name][tag(dtype)] if margins is None else margins)
    pool = POOL.get(name, 1) if pool is None else pool
    return {"e": (rel_l2(y, ref), bound(rel_l2(emul, ref))),
            "pix": (e_pix(y, ref, pool).max().item(), max(1e-3, m_pix * e_pix(emul, ref, pool).max().item())),
            "ch": (e_ch(y, ref).max().item(), max(1e-3, m_ch * e_ch(emul, ref).max().item()))}


def holds(cond):
    return {k: v <= b for k, (v, b) in cond.items()}


def where(name, out, row, pool=1):
    """(instance, y, x) of pixel row `row` (the first of its group) of output `out`."""
    _m, h, w = out_hw(name)[out]
    row *= pool
    return row // (h * w), row % (h * w) // w, row % w


# ---- margins -----------------------------------------------------------------------------------------------------
_SEEDS = {}


def seed_outputs(name):
    """[{"ref": .., "emul": ..} per input seed] of one case, on one CPU thread (the summation order of a threaded matmul
    is another realisation of the noise); computed once per process."""
    if name not in _SEEDS:
        threads = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            both = make_oracle(name)
            runs = []
            for seed in range(N_SEEDS):
                o = oracle_outputs(name, seed, both)
                runs.append({"ref": o["ref"], "emul": o["emul"]})
            _SEEDS[name] = runs
        finally:
            torch.set_num_threads(threads)
    return _SEEDS[name]


def seed_stats(name, pool=1):
    """{dtype tag: {output: ([max_p e_pix per seed], [max_c e_ch per seed])}} from the oracle alone."""
    stat = {tag(dt): {o: ([], []) for o in outputs_of(name)} for dt in DTYPES}
    for run in seed_outputs(name):
        for dt in DTYPES:
            for o, ref in run["ref"].items():
                em = run["emul"][dt][o]
                stat[tag(dt)][o][0].append(e_pix(em, ref, pool).max().item())
                stat[tag(dt)][o][1].append(e_ch(em, ref).max().item())
    return stat


def measure_case(name, pool=1):
    """{dtype tag: (M_pix, M_ch)}: per output largest / smallest over the seeds x FLOOR_SLACK, the largest over outputs."""
    return {t: tuple(max(round_up_2sig(max(v[i]) / min(v[i]) * FLOOR_SLACK) for v in per.values()) for i in (0, 1))
            for t, per in seed_stats(name, pool).items()}


def measure_margins(names=None):
    """-> (MARGINS, POOL) as the table above holds them."""
    margins, pools = {}, {}
    for name in (names or CASES):
        got, pool = measure_case(name, 1), 1
        if max(v[0] for v in got.values()) > 2.0:
            got, pool = measure_case(name, 16), 16
        margins[name], pools[name] = got, pool
    return margins, pools


def format_margins(margins, pools):
    lines = ["MARGINS = {"]
    for name, per in margins.items():
        lines.append("    %-15s {%s}," % ('"%s":' % name, ", ".join('"%s": (%s, %s)' % (t, v[0], v[1]) for t, v in per.items())))
    lines.append("}")
    lines.append("POOL = {%s}" % ", ".join('"%s": %d' % kv for kv in pools.items()))
    return "\n".join(lines)


def format_floors(names=None):
    """The floors behind the table: per case and dtype the range over seeds and outputs of the worst pixel and channel."""
    lines = []
    for name in (names or CASES):
        st = seed_stats(name, POOL.get(name, 1))
        lines.append("# %-13s %s" % (name, "  ".join(
            "%s pix %.1e..%.1e ch %.1e..%.1e" % (t, min(min(v[0]) for v in per.values()), max(max(v[0]) for v in per.values()),
                                                 min(min(v[1]) for v in per.values()), max(max(v[1]) for v in per.values()))
            for t, per in st.items())))
    return "\n".join(lines)


def main(argv):
    if "--margins" not in argv:
        print(__doc__)
        return 0
    margins, pools = measure_margins()
    print(format_margins(margins, pools))
    if "--floors" in argv:
        print(format_floors())
    same = margins == MARGINS and pools == POOL
    print("# %s the committed table" % ("reproduces" if same else "DIFFERS from"))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
