"""Every layer fusion switch of networks/layers.py and blocks.py, through a whole block, per token and per channel against
the float64 oracle (tests/block_cases.py: cases, metrics, measured margins).

The switches decide which kernels a block launches and how a producer hands its LayerNorm on (`_ln_cache` / `_ln_out` /
`_ln_stats` attributes, consumed once).  Each test sets one row of SETTINGS with monkeypatch.setattr on the module or
class attribute (every switch is first pinned to its documented default, so `default` means the defaults whatever the
environment of the session says), runs the block on ONE shared HIP instance per (case, dtype), and checks
  1. conditions 1-3 of block_cases against the float64 reference, and that the output is finite everywhere;
  2. that the setting reached the code: counting spies around ops.layernorm / xattn320 / gemm / attention see the launches
     and keyword arguments `expected()` derives from the structure of the block;
  3. (default only) that a second run on the same input tensors gives the same bits: the hand-off attributes leave
     nothing behind.
One line per test: [block switch] <case> <dtype> <setting> e=.. floor=.. tok=<max e_tok>/<bound> ch=<max e_ch>/<bound> calls=..
"""
import pytest
import torch

from tests import block_cases as B
from tests.parity_util import rel_l2, report

pytestmark = pytest.mark.gpu

# The documented defaults (DD_XATTN_FUSED, DD_LN_PRODUCER, DD_ATTN_HEAD_MAJOR, DD_LN_FOLD, DD_FOLD_PROJ_OUT unset).
DEFAULTS = {"XATTN_FUSED": True, "LN_PRODUCER": True, "HEAD_MAJOR": True, "LN_FOLD": "0", "fold_proj_out": True}
SETTINGS = {
    "default": {},
    "no_xattn": {"XATTN_FUSED": False},
    "no_ln_producer": {"LN_PRODUCER": False},
    "no_xattn_no_producer": {"XATTN_FUSED": False, "LN_PRODUCER": False},
    "row_major": {"HEAD_MAJOR": False},
    "fold_q": {"LN_FOLD": "q"},
    "fold_all": {"LN_FOLD": "all"},
    "fold_stats": {"LN_FOLD": "stats"},
    "no_proj_fold": {"fold_proj_out": False},                 # Transformer2DModel cases only
    "plain": {"XATTN_FUSED": False, "LN_PRODUCER": False, "HEAD_MAJOR": False, "fold_proj_out": False, "LN_FOLD": "0"},
}
MATRIX = [(c, dt, s) for c in B.CASES for dt in B.DTYPES for s in SETTINGS
          if not (s == "no_proj_fold" and B.CASES[c][0] == "MV")]


def expected(name, s):
    """The launches and keyword arguments one run of the block makes under the switches `s`, from the code:

    Transformer2DModel.run:  GroupNorm, proj_in [emits norm1], block, then ONE GEMM over [g | h] (a2) for ff.net.2 +
        proj_out where fold_proj_out, else the two GEMMs.
    BasicTransformerBlock.run:  attn1 = fused Q|K|V GEMM (reads norm1), attention, to_out GEMM [emits norm2];
        attn2 = K|V GEMM of the context, then dd_xattn320 (reads norm2, emits the next norm) or to_q GEMM (reads norm2),
        attention, to_out GEMM [emits the next norm];  feed-forward = GEGLU GEMM (reads norm3) and ff.net.2.
    BasicMultiviewTransformerBlock.run (driven directly: nothing emits norm1):  between attn2 and the feed-forward,
        attn4 = fused Q|K|V GEMM (reads norm4), ONE attention launch for both neighbours (ATTN4_PAIR),
        connector(to_out) as one GEMM [emits norm3].

    A LayerNorm is FOLDED into its consumer GEMM (ln=) when ln_fold_ok says so: "all" always, "q" where the consumer is
    no wider than C (attn2.to_q alone), "stats" where a producer left row statistics (every norm but a directly driven
    block's norm1).  It is EMITTED by its producer (ln_out=) at the 320-channel level with LN_PRODUCER on and no fold
    (ln_producer_ok, run_cross, _cross_view).  Otherwise it is LAUNCHED.  dd_xattn320 runs at 320 channels with no fold
    on (run_cross: a fold would take the q-projection's LayerNorm away from it)."""
    kind, c = B.CASES[name][:2]
    mv, fold = kind == "MV", s["LN_FOLD"]
    xattn = s["XATTN_FUSED"] and c == 320 and fold == "0"
    emit = s["LN_PRODUCER"] and c == 320 and fold == "0"
    cross_out = "xattn320" if xattn else "gemm"
    # (producer of the norm's input, width of its consumer in units of C)
    norms = [(None if mv else "gemm", 3), ("gemm", 1)] + ([(cross_out, 3), ("gemm", 8)] if mv else [(cross_out, 8)])
    exp = dict.fromkeys(("gemm.ln", "gemm.stats_in", "gemm.ln_out", "xattn320.ln_out", "gemm.ln_stats", "layernorm"), 0)
    for prod, width in norms:
        if fold == "all" or (fold == "q" and width <= 1) or (fold == "stats" and prod is not None):
            exp["gemm.ln"] += 1
            exp["gemm.stats_in"] += fold == "stats"           # the consumer finds the producer's statistics on its input
        elif emit and prod is not None:
            exp[prod + ".ln_out"] += 1
        else:
            exp["layernorm"] += 1
        exp["gemm.ln_stats"] += fold == "stats" and prod is not None       # want_ln_stats(): every producer leaves them
    cross = 0 if xattn else 1
    exp["xattn320"] = 1 - cross
    exp["attention"] = 1 + cross + mv
    exp["attention.q_prescaled"] = exp["attention"] if s["HEAD_MAJOR"] else 0
    exp["gemm.head_major"] = (1 + cross + mv) if s["HEAD_MAJOR"] else 0         # Q|K|V, to_q, attn4's Q|K|V
    if mv:                       # Q|K|V, to_out, K|V, [to_q, to_out], attn4 Q|K|V, connector, GEGLU, ff.net.2
        exp["gemm"], exp["gemm.a2"] = 7 + 2 * cross, 0
    else:                        # proj_in, Q|K|V, to_out, K|V, [to_q, to_out], GEGLU, then 1 folded or 2 plain GEMMs
        exp["gemm"], exp["gemm.a2"] = 5 + 2 * cross + (1 if s["fold_proj_out"] else 2), int(s["fold_proj_out"])
    return {k: int(v) for k, v in exp.items()}


class Spies:
    """Counting wrappers around the launch wrappers `layers` and `blocks` call through the ops module; a call counts
    when it returns (a refused launch, _native.Unsupported, made none)."""

    def __init__(self, monkeypatch, ops):
        self.n = dict.fromkeys(expected("T320", DEFAULTS), 0)
        for fn in ("layernorm", "xattn320", "gemm", "attention"):
            monkeypatch.setattr(ops, fn, self._wrap(fn, getattr(ops, fn)))

    def _wrap(self, fn, real):
        def spy(*a, **kw):
            out = real(*a, **kw)
            self.n[fn] += 1
            if fn == "gemm":
                for k in ("ln", "ln_out", "head_major", "a2"):
                    self.n["gemm." + k] += kw.get(k) is not None
                self.n["gemm.ln_stats"] += bool(kw.get("ln_stats"))
                self.n["gemm.stats_in"] += kw.get("ln") is not None and getattr(a[0], "_ln_stats", None) is not None
                assert (kw.get("ln_out") is not None) == (getattr(out, "_ln_out", None) is not None)
                assert bool(kw.get("ln_stats")) == (getattr(out, "_ln_stats", None) is not None)
            elif fn == "xattn320":
                self.n["xattn320.ln_out"] += kw.get("ln_out") is not None
            elif fn == "attention":
                self.n["attention.q_prescaled"] += bool(kw.get("q_prescaled"))
            return out
        return spy


@pytest.fixture(scope="module")
def shared(gpu):
    """name -> oracle outputs (CPU, once per case); (name, dtype) -> the ONE HIP block and its device inputs."""
    cache = {}

    def get(name, dtype):
        if name not in cache:
            cache[name] = B.oracle_outputs(name)
        o = cache[name]
        if (name, dtype) not in cache:
            cache[name, dtype] = (B.make_hip(name, o["sd"], dtype),) + B.hip_inputs(name, o["x"], o["ctx"], dtype)
        return (o,) + cache[name, dtype]
    return get


@pytest.mark.parametrize("name,dtype,setting", MATRIX, ids=["%s-%s-%s" % (c, B.tag(dt), s) for c, dt, s in MATRIX])
def test_block_switch(shared, monkeypatch, name, dtype, setting):
    from dualdiff_amd import ops
    from dualdiff_amd.networks import blocks, layers
    o, blk, x2d, ctx2d = shared(name, dtype)
    s = dict(DEFAULTS, **SETTINGS[setting])
    for k, v in s.items():
        monkeypatch.setattr(layers.Transformer2DModel if k == "fold_proj_out" else layers, k, v)
    monkeypatch.setattr(blocks, "ATTN4_PAIR", True)
    spies = Spies(monkeypatch, ops)

    y = B.run_hip(name, blk, x2d, ctx2d)
    torch.cuda.synchronize()
    calls = dict(spies.n)
    ref, emul = o["ref"], o["emul"][dtype]
    assert y.shape == ref.shape and y.dtype == dtype
    assert torch.isfinite(y).all()
    cond = B.conditions(name, dtype, y, ref, emul)
    print("[block switch] %s %s %s e=%.3e floor=%.3e tok=%.3e/%.3e ch=%.3e/%.3e calls=%s"
          % (name, B.tag(dtype), setting, cond["e"][0], rel_l2(emul, ref), cond["tok"][0], cond["tok"][1],
             cond["ch"][0], cond["ch"][1], " ".join("%s=%d" % kv for kv in sorted(calls.items()) if kv[1])))
    assert calls == expected(name, s)
    rec = []
    assert report("block switch %s %s" % (name, setting), y, ref, dtype, rec, emul) <= 1.0, rec
    assert cond["tok"][0] <= cond["tok"][1], "worst token row %d" % int(B.e_tok(y, ref, B.POOL[name]).argmax())
    assert cond["ch"][0] <= cond["ch"][1], "worst channel %d" % int(B.e_ch(y, ref).argmax())
    for t in (x2d, ctx2d):                       # nothing is left hanging on the caller's tensors
        assert not [a for a in ("_ln_cache", "_ln_out", "_ln_stats", "_gn_cache") if hasattr(t, a)]
    if setting == "default":
        y2 = B.run_hip(name, blk, x2d, ctx2d)
        assert torch.equal(y, y2), "a second run on the same input tensors changes the result"
        assert spies.n == {k: 2 * v for k, v in calls.items()}
