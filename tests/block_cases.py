"""Block-level cases with a per-token and a per-channel error metric — a helper of tests/test_block_metric_cpu.py and
tests/test_block_switches_gpu.py, not a test itself.

A case pairs an oracle block (oracle/diffusers_restated.py, oracle/dualdiff_restated.py) with the HIP block of
dualdiff_amd/networks: seeded_state_dict rounded to bf16 loaded into both, inputs rounded to bf16, so that one CPU run is
the exact-weight reference of the fp16 and of the bf16 HIP run.  References, computed on the CPU once per case:
    ref          the oracle block in float64;
    emul[dtype]  the same block under storage_emulation(dtype): ONE realisation of the storage dtype's rounding noise.

The cases are the smallest shapes at which each path is still the one taken: the LayerNorm fold takes K in {320, 640,
1280}; dd_xattn320 takes 320 channels, 8 heads x 40 and <= 128 keys, and 100 tokens per instance are one 80-row tile of
it plus a ragged 20.

Metrics of an output y (rows, C) against ref:
    e_tok(y)[r] = ||y_r - ref_r||_2 / ||ref_r||_2     per token row r (rows pooled in groups of POOL[case], see below)
    e_ch(y)[c]  = the same per channel c, over the rows
    e(y)        = the whole-tensor relative L2 error of tests/parity_util.py
Conditions on a HIP output (`conditions`):
    1. e(y)          <= max(1e-3, 1.02 e(emul))                      (parity_util.bound, unchanged)
    2. max_r e_tok(y) <= max(1e-3, M_tok max_r e_tok(emul))
    3. max_c e_ch(y)  <= max(1e-3, M_ch  max_c e_ch(emul))
The whole-tensor number averages over rows x C values and cannot see a 5 % error in one token of a workload-sized
output (0.05 / sqrt(8400) = 5.5e-4); 2 and 3 bound the WORST row and the WORST channel.

Margins.  max_r e_tok(emul) is the largest of `rows` noisy values of one realisation of rounding noise; how far it sits
from the same statistic of another realisation is measured from the reference alone: emul is evaluated for N_SEEDS input
seeds per case and dtype, M = (largest over seeds) / (smallest over seeds) x FLOOR_SLACK (1.02), rounded UP to two
significant digits.  `python -m tests.block_cases --margins` recomputes and prints the table below; no HIP code takes part.
The measurement runs on one CPU thread, so that it gives the same table wherever it is run.
A margin above 2 would mean the statistic is too noisy to localise anything: such a case pools its rows in groups of 16
(POOL) — none needs it, see the table.
"""
import copy
import math
import os
import sys

import torch

if __name__ == "__main__":                                   # `python tests/block_cases.py` as well as `-m tests.block_cases`
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import diffusers_restated as D  # noqa: E402
from oracle import dualdiff_restated as R  # noqa: E402
from oracle.init_utils import seeded_state_dict, seeded_tensor  # noqa: E402
from oracle.numerics import storage_emulation  # noqa: E402
from tests.parity_util import FLOOR_SLACK, bound, rel_l2  # noqa: E402

PAIR = {0: [5, 1], 1: [0, 2], 2: [1, 3], 3: [2, 4], 4: [3, 5], 5: [4, 0]}
DTYPES = [torch.float16, torch.bfloat16]
LC, CTX_DIM = 13, 768                      # context tokens per instance, their width
N_SEEDS = 8                                # input seeds of the margin measurement; seed 0 is the one the tests run

# name: (kind, channels, heads, head_dim, instances, (h, w) of a T case / tokens per view of an MV case, weight seed)
CASES = {
    "T320": ("T", 320, 8, 40, 2, (10, 10), 31),
    "T640": ("T", 640, 8, 80, 2, (7, 10), 32),
    "T1280": ("T", 1280, 8, 160, 2, (4, 7), 33),
    "MV320": ("MV", 320, 8, 40, 6, 100, 34),
    "MV640": ("MV", 640, 8, 80, 6, 70, 35),
}

# ---- measured margins (python -m tests.block_cases --margins) ----------------------------------------------------
# case: {dtype: (M_tok, M_ch)}; POOL[case] = rows per group of e_tok (1: every token row on its own).
#   worst-row / worst-channel floors behind them, max_r e_tok(emul) and max_c e_ch(emul) over the 8 seeds:
#     fp16: 6.3e-4 .. 8.2e-4 per row, 6.7e-4 .. 9.8e-4 per channel — below the 1e-3 of conditions 2 and 3, which then is the bound;
#     bf16: 5.1e-3 .. 6.4e-3 per row, 5.6e-3 .. 7.8e-3 per channel.
MARGINS = {
    "T320":   {"float16": (1.1, 1.2), "bfloat16": (1.1, 1.2)},
    "T640":   {"float16": (1.1, 1.2), "bfloat16": (1.1, 1.2)},
    "T1280":  {"float16": (1.1, 1.2), "bfloat16": (1.1, 1.2)},
    "MV320":  {"float16": (1.2, 1.1), "bfloat16": (1.1, 1.1)},
    "MV640":  {"float16": (1.1, 1.1), "bfloat16": (1.1, 1.1)},
}
POOL = {"T320": 1, "T640": 1, "T1280": 1, "MV320": 1, "MV640": 1}


def tag(dtype):
    return str(dtype).split(".")[-1]


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def make_oracle(name):
    """(oracle block in fp32 with its bf16-rounded seeded weights, that state dict)."""
    kind, c, heads, hd, _m, _sp, wseed = CASES[name]
    if kind == "T":
        ora = D.Transformer2DModel(heads, hd, c, cross_attention_dim=CTX_DIM)
    else:
        ora = R.BasicMultiviewTransformerBlock(c, heads, hd, cross_attention_dim=CTX_DIM, neighboring_view_pair=PAIR)
    ora = ora.eval()
    sd = {k: bf16_round(v) for k, v in seeded_state_dict(ora, wseed).items()}
    ora.load_state_dict(sd)
    return ora, sd


def make_inputs(name, seed=0):
    """(x, ctx), bf16-rounded fp32: x is (m, C, h, w) for a T case and (views, tokens, C) for an MV case."""
    kind, c, _heads, _hd, m, sp, wseed = CASES[name]
    shape = (m, c) + sp if kind == "T" else (m, sp, c)
    base = 1000 * wseed + 2 * seed
    return bf16_round(seeded_tensor(shape, base + 1)), bf16_round(seeded_tensor((m, LC, CTX_DIM), base + 2))


def rows_of(name, out):
    """The block's output as (rows, C): token-major, the layout the HIP block hands back."""
    kind, c = CASES[name][:2]
    if kind == "T":
        out = out[0] if isinstance(out, tuple) else out
        return out.permute(0, 2, 3, 1).reshape(-1, c)
    return out.reshape(-1, c)


def run_oracle(name, ora, x, ctx):
    with torch.no_grad():
        return rows_of(name, ora(x, encoder_hidden_states=ctx)).contiguous()


def run_emul(name, ora, x, ctx, dtype):
    with storage_emulation(ora, dtype):
        return run_oracle(name, ora, x, ctx)


def oracle_outputs(name, seed=0):
    """{"sd", "x", "ctx", "ref": float64 (rows, C), "emul": {dtype: fp32 (rows, C)}} of one case."""
    ora, sd = make_oracle(name)
    x, ctx = make_inputs(name, seed)
    ref = run_oracle(name, copy.deepcopy(ora).double(), x.double(), ctx.double())
    return {"sd": sd, "x": x, "ctx": ctx, "ref": ref, "emul": {dt: run_emul(name, ora, x, ctx, dt) for dt in DTYPES}}


# ---- the HIP side ------------------------------------------------------------------------------------------------
def make_hip(name, sd, dtype):
    from dualdiff_amd.networks import blocks, layers
    kind, c, heads, hd = CASES[name][:4]
    if kind == "T":
        blk = layers.Transformer2DModel(heads, hd, c, CTX_DIM)
    else:
        blk = blocks.BasicMultiviewTransformerBlock(c, heads, hd, cross_attention_dim=CTX_DIM, neighboring_view_pair=PAIR)
    blk.load_state_dict(sd, strict=True)
    return blk.to("cuda", dtype).eval()


def hip_inputs(name, x, ctx, dtype):
    """Device tensors in the layout the block's run() takes: (rows, C) token-major activations, (m * LC, 768) context."""
    kind, c = CASES[name][:2]
    x2d = x.permute(0, 2, 3, 1).reshape(-1, c) if kind == "T" else x.reshape(-1, c)
    return x2d.contiguous().cuda().to(dtype), ctx.reshape(-1, CTX_DIM).contiguous().cuda().to(dtype)


def run_hip(name, blk, x2d, ctx2d):
    kind, _c, _heads, _hd, m, sp = CASES[name][:6]
    with torch.no_grad():
        if kind == "T":
            return blk.run(x2d, m, sp[0], sp[1], ctx2d, LC)
        return blk.run(x2d, m, sp, ctx2d, LC)


# ---- metrics -----------------------------------------------------------------------------------------------------
def _f64(t):
    return t.detach().cpu().double()


def e_tok(y, ref, pool=1):
    """Relative L2 error of every token row (of every group of `pool` consecutive rows; a ragged last group stays)."""
    y, ref = _f64(y), _f64(ref)
    d2, r2 = ((y - ref) ** 2).sum(dim=1), (ref ** 2).sum(dim=1)
    if pool > 1:
        pad = (-d2.numel()) % pool
        d2 = torch.nn.functional.pad(d2, (0, pad)).reshape(-1, pool).sum(dim=1)
        r2 = torch.nn.functional.pad(r2, (0, pad)).reshape(-1, pool).sum(dim=1)
    return (d2 / (r2 + 1e-300)).sqrt()


def e_ch(y, ref):
    y, ref = _f64(y), _f64(ref)
    return (((y - ref) ** 2).sum(dim=0) / ((ref ** 2).sum(dim=0) + 1e-300)).sqrt()


def conditions(name, dtype, y, ref, emul, margins=None, pool=None):
    """-> {"e": (value, bound), "tok": (value, bound), "ch": (value, bound)}: conditions 1-3 of the module docstring."""
    m_tok, m_ch = (MARGINS[name][tag(dtype)] if margins is None else margins)
    pool = POOL.get(name, 1) if pool is None else pool
    return {"e": (rel_l2(y, ref), bound(rel_l2(emul, ref))),
            "tok": (e_tok(y, ref, pool).max().item(), max(1e-3, m_tok * e_tok(emul, ref, pool).max().item())),
            "ch": (e_ch(y, ref).max().item(), max(1e-3, m_ch * e_ch(emul, ref).max().item()))}


def holds(cond):
    return {k: v <= b for k, (v, b) in cond.items()}


# ---- margins -----------------------------------------------------------------------------------------------------
def round_up_2sig(v):
    if v <= 0:
        return 0.0
    q = 10.0 ** (math.floor(math.log10(v)) - 1)
    return round(math.ceil(v / q - 1e-9) * q, 10)


def measure_case(name, pool=1):
    """{dtype tag: (M_tok, M_ch, [max_r e_tok per seed], [max_c e_ch per seed])} from the oracle alone."""
    ora, _sd = make_oracle(name)
    ora64 = copy.deepcopy(ora).double()
    stat = {tag(dt): ([], []) for dt in DTYPES}
    for seed in range(N_SEEDS):
        x, ctx = make_inputs(name, seed)
        ref = run_oracle(name, ora64, x.double(), ctx.double())
        for dt in DTYPES:
            em = run_emul(name, ora, x, ctx, dt)
            stat[tag(dt)][0].append(e_tok(em, ref, pool).max().item())
            stat[tag(dt)][1].append(e_ch(em, ref).max().item())
    return {t: (round_up_2sig(max(a) / min(a) * FLOOR_SLACK), round_up_2sig(max(b) / min(b) * FLOOR_SLACK), a, b)
            for t, (a, b) in stat.items()}


def measure_margins(names=None):
    """-> (MARGINS, POOL) as the table above holds them: a case whose per-row margin exceeds 2 is measured again with
    its rows pooled in groups of 16."""
    margins, pools = {}, {}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)          # the summation order of a threaded matmul is another realisation of the noise
    try:
        for name in (names or CASES):
            got, pool = measure_case(name, 1), 1
            if max(v[0] for v in got.values()) > 2.0:
                got, pool = measure_case(name, 16), 16
            margins[name] = {t: (v[0], v[1]) for t, v in got.items()}
            pools[name] = pool
    finally:
        torch.set_num_threads(threads)
    return margins, pools


def format_margins(margins, pools):
    lines = ["MARGINS = {"]
    for name, per in margins.items():
        lines.append("    %-9s {%s}," % ('"%s":' % name, ", ".join('"%s": (%s, %s)' % (t, v[0], v[1]) for t, v in per.items())))
    lines.append("}")
    lines.append("POOL = {%s}" % ", ".join('"%s": %d' % kv for kv in pools.items()))
    return "\n".join(lines)


def main(argv):
    if "--margins" not in argv:
        print(__doc__)
        return 0
    margins, pools = measure_margins()
    print(format_margins(margins, pools))
    same = margins == MARGINS and pools == POOL
    print("# %s the committed table" % ("reproduces" if same else "DIFFERS from"))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
