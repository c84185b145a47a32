"""model_base.sibling_overlap where its readiness proof cannot see (the rule is restated in tests/sibling_cases.py).

A forward() is moved onto the model's side stream, behind an event recorded at the PREVIOUS model's entry, when every
tensor argument is vouched for by its storage, view and version.  That proof covers what torch wrote.  Tested here is
what it does not cover by itself:
  H1  the model's own weights, changed on the caller's stream between the two calls (load_state_dict, an in-place
      update + _invalidate, a sub-module's .to() / load_state_dict, fold_lora_, enable_fp8_weights);
  H2  this package's raw-pointer writers (out=, x_out=, x_dup=, in-place targets), which must count a version;
  H3  two models that hold the same sub-module object or the same Parameter;
  H4  keys that are not recorded yet (first sight, capture), and an exception on the side stream.
Every scenario runs twice from cloned inputs, once with the overlap switched off and once with it on: the outputs must
be the same bits and the number of overlapped calls the expected one.  Where a scenario changes something between two
calls, a 50 ms sleep sits on the caller's stream in front of the change: a call that is wrongly moved to the side
stream then certainly runs ahead of the change and returns the numbers of the old weights / old latents.

Models: three two-level UNets (320 / 640 channels, one layer per block), 12 instances of 8 x 10 latents, 83 context
tokens (capacity 110) — the smallest that take the graph path with both cross-attention forms."""
import types

import pytest
import torch

from tests import block_cases as BC
from tests import gemm_reference as G
from tests import sibling_cases as C

pytestmark = pytest.mark.gpu

SLEEP = 5_000_000                 # torch.cuda._sleep: 50 ms at the 100 MHz of the constant counter (test_device_consts_gpu.py)
M, REAL, LONG = 12, 83, 120       # instances; context tokens (bucket capacity 110); a length of the next bucket
F16 = torch.float16


def _unet(seed, gpu):
    from dualdiff_amd.networks import layers as L
    from dualdiff_amd.networks.unet_2d_condition_multiview import UNet2DConditionModelMultiview
    unet = UNet2DConditionModelMultiview(
        down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"),
        block_out_channels=(320, 640), layers_per_block=1, cross_attention_dim=768, neighboring_view_pair=BC.PAIR)
    return L.seeded_init_(unet, seed).to(gpu, F16).eval()


@pytest.fixture(scope="module")
def env(gpu):
    from dualdiff_amd.networks import model_base as MB
    e = types.SimpleNamespace(MB=MB, dev=gpu)
    e.A, e.B = _unet(5, gpu), _unet(6, gpu)
    e.S = _unet(7, gpu)                                  # shares a sub-module OBJECT with A
    e.S.time_embedding = e.A.time_embedding
    e.P = _unet(7, gpu)                                  # shares one PARAMETER with A
    e.P.conv_norm_out.weight = e.A.conv_norm_out.weight
    e.sd_b = {k: v.clone() for k, v in e.B.state_dict().items()}
    e.sd_other = {k: v.clone() for k, v in _unet(8, gpu).state_dict().items()}       # other weights for B, on the GPU
    e.x0 = G.rand((M, 4, 8, 10), F16, 7200, device=gpu)
    e.ctx0 = G.rand((M, REAL, 768), F16, 7201, device=gpu)
    e.ctx_long = G.rand((M, LONG, 768), F16, 7202, device=gpu)
    e.t = torch.tensor(481, device=gpu)
    yield e
    torch.cuda.synchronize()


def call(e, model, x, ctx, **kw):
    with torch.no_grad():
        return model(x, e.t, encoder_hidden_states=ctx, **kw).sample


def count(model):
    return model.__dict__.get("_sib_overlapped", 0)


def serial(e, fn):
    was, e.MB.SIBLING_OVERLAP = e.MB.SIBLING_OVERLAP, False
    try:
        return fn()
    finally:
        e.MB.SIBLING_OVERLAP = was


def warm(e, models, x, ctx):
    """eager, record, replay — with the overlap off, so that no call of it counts"""
    serial(e, lambda: [call(e, m, x, ctx) for _ in range(3) for m in models])


def both(e, scenario):
    """scenario(x, ctx) -> (outputs, overlapped counts) from cloned inputs: switched off, then on.  -> the counts of
    the second run, after the outputs of the two were found equal bit for bit."""
    want, zeros = serial(e, lambda: scenario(e.x0.clone(), e.ctx0.clone()))
    got, counts = scenario(e.x0.clone(), e.ctx0.clone())
    torch.cuda.synchronize()
    assert not any(zeros)
    assert len(want) == len(got)
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), "output %d differs from the run without overlap" % i
    return got, counts


def restore_b(e):
    from dualdiff_amd.networks.layers import enable_fp8_weights
    enable_fp8_weights(e.B, on=False)
    e.B.load_state_dict(e.sd_b)
    torch.cuda.synchronize()


# ---- the overlap exists --------------------------------------------------------------------------------------------------------

def test_baseline_overlaps(env):
    """Guards every "not overlapped" below against a rule that never overlaps."""
    e = env

    def scenario(x, ctx):
        warm(e, [e.A, e.B], x, ctx)
        outs, counts, n0 = [], [], count(e.B)
        for _ in range(3):
            outs += [call(e, e.A, x, ctx), call(e, e.B, x, ctx)]
            counts.append(count(e.B) - n0)
        return outs, counts
    _, counts = both(e, scenario)
    assert counts == [1, 2, 3]


# ---- H1: the model's own weights -----------------------------------------------------------------------------------------------

def _weights_scenario(e, mutate, changes=True, drops_graphs=True):
    """A(x); sleep; change B's weights; B(x) [not overlapped, new weights]; A(x); B(x); A(x); B(x).  drops_graphs: the
    change goes through B._invalidate(), so B's key is unknown again — the call after the change is its first sight, the
    next one records (neither is overlapped), the third replays on the side stream.  Without it (a packed-weight drop
    below B: the epoch alone is over) the key is known, the call after the change records again on the caller's
    stream, and the two pairs behind it overlap."""
    def scenario(x, ctx):
        try:
            warm(e, [e.A, e.B], x, ctx)
            n0 = count(e.B)
            outs = [call(e, e.B, x, ctx)]
            # B's recorded graphs stay alive over the change (a caller may hold them through views of their outputs as
            # well): destroying a graph can wait for the device, and a wait between the sleep and B's call would let a
            # wrongly overlapped call see the new weights by accident
            keep = list(e.B.__dict__["_fwd_graphs"].entries.values())
            assert keep
            call(e, e.A, x, ctx)
            torch.cuda._sleep(SLEEP)
            mutate()
            outs.append(call(e, e.B, x, ctx))
            counts = [count(e.B) - n0]
            for _ in range(2):
                call(e, e.A, x, ctx)
                outs.append(call(e, e.B, x, ctx))
                counts.append(count(e.B) - n0)
            torch.cuda.synchronize()
            del keep
            return outs, counts
        finally:
            restore_b(e)
    outs, counts = both(e, scenario)
    if changes:
        assert not torch.equal(outs[0], outs[1]), "the change of the weights did not reach the output"
    assert torch.equal(outs[1], outs[2]) and torch.equal(outs[1], outs[3])
    assert counts == ([0, 0, 1] if drops_graphs else [0, 1, 2])


@pytest.mark.parametrize("how", ["load_state_dict", "mul_"])
def test_weight_change_between_calls_is_ordered(env, how):
    e = env

    def load():
        e.B.load_state_dict(e.sd_other)

    def mul():
        with torch.no_grad():
            e.B.conv_in.weight.mul_(1.5)
        e.B._invalidate()
    _weights_scenario(e, load if how == "load_state_dict" else mul)


@pytest.mark.parametrize("how", ["to", "load_state_dict"])
def test_sub_module_cache_drop_is_ordered(env, how):
    """A sub-module's .to() / load_state_dict drops its packed weights (layers.CACHE_EPOCH) without B._invalidate()."""
    e = env
    sub = {k[len("down_blocks.0."):]: v for k, v in e.sd_other.items() if k.startswith("down_blocks.0.")}
    assert sub

    def to():
        e.B.down_blocks[0].to(F16)                       # same dtype: the values stay, the packed copies are rebuilt

    def load():
        e.B.down_blocks[0].load_state_dict(sub)
    _weights_scenario(e, to if how == "to" else load, changes=how != "to", drops_graphs=False)


@pytest.mark.parametrize("how", ["fold_lora_", "enable_fp8_weights"])
def test_lora_and_fp8_conversions_are_ordered(env, how):
    """fold_lora_ rewrites the attention projections in place; enable_fp8_weights switches the 640-wide GEGLU projection
    of the mid block to W8A8 (the only fp8-eligible projection of this model: layers.fp8_mfma_ok)."""
    from dualdiff_amd.lora import fold_lora_, lora_keys
    from dualdiff_amd.networks.layers import enable_fp8_weights
    e = env
    lora = {k: G.rand(shape, torch.float32, 900 + i, 0.05, device=e.dev)
            for i, (k, shape) in enumerate(sorted(lora_keys(e.B, 4).items()))}
    torch.cuda.synchronize()

    def fold():
        assert fold_lora_(e.B, lora, 0.8) == len(lora) // 2

    def fp8():
        assert enable_fp8_weights(e.B) > 0
    _weights_scenario(e, fold if how == "fold_lora_" else fp8, drops_graphs=how == "fold_lora_")


# ---- H2: raw-pointer writers ---------------------------------------------------------------------------------------------------

def _given(e, n):
    from dualdiff_amd import ops
    mask = torch.zeros(M, dtype=torch.uint8)
    mask[::2] = 1
    return ops.GivenViews(mask.to(e.dev), G.rand((n,), torch.float32, 7301, device=e.dev),
                          G.rand((n,), F16, 7302, device=e.dev), torch.tensor([0.9, 0.4, 0.1], device=e.dev), 1)


WRITES = ["scale", "add", "cfg_ddim_step", "cfg_unipc_step", "given_views_noise", "gemm"]


@pytest.mark.parametrize("what", WRITES)
def test_raw_writes_between_calls_are_seen(env, what):
    """A(x); sleep; a raw write into x (or the context); B(x) — not overlapped, and computed from what was written."""
    from dualdiff_amd import ops
    from dualdiff_amd.pipeline.pipeline_bev_controlnet import ddim_schedule
    from dualdiff_amd.pipeline.schedulers import unipc_schedule
    e = env
    n = e.x0.numel()
    src = G.rand(tuple(e.x0.shape), F16, 7310, device=e.dev)
    eps = G.rand((2,) + tuple(e.x0.shape), F16, 7311, device=e.dev)
    ddim, unipc = ddim_schedule(50)[1][25].to(e.dev), unipc_schedule(8)[1][3].to(e.dev)
    given = _given(e, n)
    a, w = G.rand((M * REAL, 64), F16, 7312, device=e.dev), G.rand((768, 64), F16, 7313, 0.125, device=e.dev)
    torch.cuda.synchronize()

    def scenario(x, ctx):
        dup = x.clone()                                  # the ddim case hands B the step's second output
        lat = dup if what == "cfg_ddim_step" else x
        hist = torch.zeros((3, n), dtype=torch.float32, device=e.dev)
        warm(e, [e.A, e.B], lat, ctx)
        n0 = count(e.B)
        outs = [call(e, e.B, lat, ctx)]
        call(e, e.A, lat, ctx)
        torch.cuda._sleep(SLEEP)
        if what == "scale":
            ops.scale(src, 0.5, out=x)
        elif what == "add":
            ops.add(x, src, out=x)
        elif what == "cfg_ddim_step":
            ops.cfg_ddim_step(eps, x, ddim, 2.0, x_out=x, x_dup=dup)
        elif what == "cfg_unipc_step":
            ops.cfg_unipc_step(eps, x, hist, unipc, 2.0, x_out=x)
        elif what == "given_views_noise":
            ops.given_views_noise(x, given, torch.tensor([0.8, 0.6]))
        else:
            ops.gemm(a, w, out=ctx.view(M * REAL, 768))
        outs.append(call(e, e.B, lat, ctx))
        counts = [count(e.B) - n0]
        call(e, e.A, lat, ctx)                           # nothing written since: the pair overlaps again
        outs.append(call(e, e.B, lat, ctx))
        counts.append(count(e.B) - n0)
        return outs, counts
    outs, counts = both(e, scenario)
    assert not torch.equal(outs[0], outs[1]), "the write did not reach the output"
    assert torch.equal(outs[1], outs[2])
    assert counts == [0, 1]


@pytest.mark.parametrize("name", sorted(C.RAW_WRITERS))
def test_every_raw_writer_bumps_the_version(env, name):
    """Each tensor a wrapper writes through its data pointer counts one version more after the call: the version is
    what sibling_overlap's readiness proof reads."""
    row = C.RAW_WRITERS[name]
    run, written = row["make"](env.dev)
    flat = {}
    for arg, ts in written.items():
        for i, t in enumerate(ts if isinstance(ts, (tuple, list)) else (ts,)):
            if t is not None:
                flat["%s[%d]" % (arg, i)] = t
    assert set(written) == set(row["writes"]) and flat
    before = {k: t._version for k, t in flat.items()}
    run()
    torch.cuda.synchronize()
    stale = [k for k, t in flat.items() if t._version <= before[k]]
    assert not stale, "%s wrote %s without counting a version" % (name, stale)


# ---- H3: shared sub-modules and parameters -------------------------------------------------------------------------------------

@pytest.mark.parametrize("sharing", ["module", "parameter"])
@pytest.mark.parametrize("order", ["A-S", "S-A"])
def test_shared_sub_module_or_parameter_never_overlaps(env, sharing, order):
    e = env
    s = e.S if sharing == "module" else e.P
    first, second = (e.A, s) if order == "A-S" else (s, e.A)

    def scenario(x, ctx):
        n0 = count(first), count(second), count(e.B)
        warm(e, [first, second, e.B], x, ctx)
        outs = []
        for _ in range(3):
            outs += [call(e, first, x, ctx), call(e, second, x, ctx)]
        shared = [count(first) - n0[0], count(second) - n0[1]]
        outs += [call(e, e.A, x, ctx), call(e, e.B, x, ctx)]          # A and B share nothing
        return outs, shared + [count(e.B) - n0[2]]
    _, counts = both(e, scenario)
    assert counts == [0, 0, 1]


# ---- H4: keys that are not recorded, exceptions --------------------------------------------------------------------------------

def test_no_overlap_until_the_key_is_recorded(env):
    e = env

    def scenario(x, ctx):
        e.A._invalidate()                                # the long context is new to both models in both runs
        e.B._invalidate()
        warm(e, [e.A, e.B], x, ctx)
        outs, counts = [], []
        e.B._invalidate()
        for c in (ctx, e.ctx_long):                      # B's graphs dropped; then a context length of another bucket
            e.MB.sibling_barrier()
            for _ in range(3):
                n0 = count(e.A), count(e.B)
                outs += [call(e, e.A, x, c), call(e, e.B, x, c)]
                counts += [count(e.A) - n0[0], count(e.B) - n0[1]]
        return outs, counts
    _, counts = both(e, scenario)
    # (A, B) per pair.  83 tokens: A is recorded (its first call has no window); B is seen, recorded, replayed.
    # 120 tokens: both are seen, recorded, replayed.
    assert counts == [0, 0, 1, 0, 1, 1] + [0, 0, 0, 0, 1, 1]


def test_exception_on_the_side_stream(env):
    e = env

    def scenario(x, ctx):
        warm(e, [e.A, e.B], x, ctx)
        call(e, e.A, x, ctx)
        call(e, e.B, x, ctx)
        cur = torch.cuda.current_stream()
        n0 = count(e.B)
        call(e, e.A, x, ctx)
        with pytest.raises(NotImplementedError):
            call(e, e.B, x, ctx, cross_attention_kwargs={"k": 1})
        assert getattr(e.MB._SIB, "window", None) is None
        assert torch.cuda.current_stream() == cur
        outs = [call(e, e.B, x, ctx)]
        counts = [count(e.B) - n0]
        outs += [call(e, e.A, x, ctx), call(e, e.B, x, ctx)]
        counts.append(count(e.B) - n0)
        return outs, counts
    _, counts = both(e, scenario)
    assert counts == [0, 1]


# ---- everything together -------------------------------------------------------------------------------------------------------

def test_random_interleavings_equal_serial(env):
    """SEQS seeded sequences of LENGTH actions (tests/sibling_cases.py); the decisions must be those of the pure-Python
    rule, call by call, and every output the bits of the run without overlap.  No sleeps."""
    from dualdiff_amd import ops
    e = env
    seqs = C.sequences()
    models = {"A": e.A, "B": e.B, "S": e.S}
    other = torch.cuda.Stream()

    def run():
        for m in models.values():
            m._invalidate()
        outs, decisions = [], []
        for seq in seqs:
            x, ctx = e.x0.clone(), e.ctx0
            row = []
            for action in seq:
                if action.startswith("call_"):
                    m = models[action[5]]
                    n0 = count(m)
                    if action.endswith("other_stream"):
                        cur = torch.cuda.current_stream()
                        other.wait_stream(cur)
                        with torch.cuda.stream(other):
                            outs.append(call(e, m, x, ctx))
                        cur.wait_stream(other)
                    else:
                        outs.append(call(e, m, x, ctx))
                    row.append((action[5], count(m) - n0 == 1))
                    continue
                row.append(None)
                if action == "new_x":
                    x = x * 1.01
                elif action == "mul_x":
                    x.mul_(0.99)
                elif action == "raw_x":
                    ops.scale(x, 0.99, out=x)
                else:
                    assert action == "invalidate_B"
                    e.B._invalidate()
            decisions.append(row)
        torch.cuda.synchronize()
        return outs, decisions
    want, none = serial(e, run)
    got, decisions = run()
    assert not any(r[1] for row in none for r in row if r)
    predicted = C.predict(seqs)
    wrong = [(i, j, seqs[i][j], d, p) for i, (drow, prow) in enumerate(zip(decisions, predicted))
             for j, (d, p) in enumerate(zip(drow, prow)) if d != p]
    assert not wrong, "decisions that differ from the rule (sequence, action, name, got, predicted): %s" % wrong[:8]
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if not torch.equal(g, w)]
    assert not bad, "calls %s of %d differ from the run without overlap" % (bad[:8], len(got))
