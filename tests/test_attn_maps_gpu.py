"""networks/attn_maps.CrossAttnMapCapture: the probe in Attention.run_cross, the forward graphs, BEVDenoiser.cross_attn_map.

Blocks: a Transformer2DModel at 320 channels (the dd_xattn320 path, where q never reaches memory) and one at 640 (the
unfused path), built by tests/block_cases.py, on 4 instances (cond = the last 2) with a context laid out at the capacity
110 holding 83 real tokens.  A capture must change NO bit of the block output; a spy around ops.attention_probs records
the operands the probe passed, and the maps are held to the fp64 reference OF THOSE OPERANDS with the kernel bound
(attn_probs_reference.py), the q among them to the fp64 projection with gemm_reference.check."""
import functools

import pytest
import torch

from dualdiff_amd import ops
from tests import attn_probs_reference as AR
from tests import block_cases as B
from tests import gemm_reference as G
from tests.test_parity_r02_gpu import _denoiser, _to_dev, step_models  # noqa: F401  (fixture: state dicts, no oracle run)

pytestmark = pytest.mark.gpu

CAP, REAL, INST = 110, 83, 4


@functools.lru_cache(maxsize=None)
def _state_dict(name):
    return B.make_oracle(name)[1]


def _attn2_names(model):
    from dualdiff_amd.networks.layers import Attention
    return {n for n, m in model.named_modules() if isinstance(m, Attention) and "attn2" in n}


def _no_leftovers(*models):
    return not any("_attn_probe" in m.__dict__ for model in models for m in model.modules())


class Spy:
    """Around ops.attention_probs: records every call's operands and passes it on."""

    def __init__(self, monkeypatch):
        self.calls, self.real = [], ops.attention_probs
        monkeypatch.setattr(ops, "attention_probs", self)

    def __call__(self, q, k, batch, lq, lk, heads, head_dim, scale=None, **kw):
        self.calls.append(dict(q=q, k=k, batch=batch, lq=lq, lk=lk, heads=heads, d=head_dim, scale=scale, **kw))
        return self.real(q, k, batch, lq, lk, heads, head_dim, scale, **kw)


def _canonical(call):
    """The canonical [batch, heads, rows, d] views of a recorded call's q and k."""
    b, h, d = call["batch"], call["heads"], call["d"]
    q, k = call["q"], call["k"]
    qv = AR.head_major_view(q, b, call["lq"], h, d) if q.dim() == 3 else AR.rows_view(q, b, call["lq"], h, d)
    kv = AR.head_major_view(k, b, call["lk"], h, d) if k.dim() == 3 else AR.rows_view(k, b, call["lk"], h, d)
    return qv, kv


# ---- blocks ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", B.DTYPES, ids=B.tag)
@pytest.mark.parametrize("name", ["T320", "T640"])
@pytest.mark.parametrize("heads_mode", ["mean", "all"])
def test_block_probe_observes_and_changes_nothing(gpu, monkeypatch, name, dtype, heads_mode):
    from dualdiff_amd.networks import layers as L
    from dualdiff_amd.networks.attn_maps import CrossAttnMapCapture
    _kind, c, heads, hd, _m, (h, w), seed = B.CASES[name]
    blk = B.make_hip(name, _state_dict(name), dtype)
    lq = h * w
    x2d = G.rand((INST * lq, c), dtype, 7000 + seed, device=gpu)
    ctx2d = G.rand((INST * CAP, B.CTX_DIM), dtype, 7001 + seed, device=gpu)
    lk_dev = torch.tensor([REAL], dtype=torch.int32, device=gpu)
    attn = blk.transformer_blocks[0].attn2

    def run():
        with torch.no_grad(), L.context_keys(ctx2d, CAP, lk_dev):
            return blk.run(x2d, INST, h, w, ctx2d, CAP).clone()

    y0 = run()
    spy = Spy(monkeypatch)
    proj = []                                            # (input, kwargs, output) of attn2.to_q

    def to_q_run(x, **kw):
        out = L.Linear.run(attn.to_q, x, **kw)
        proj.append((x, kw, out))
        return out
    cap = CrossAttnMapCapture(blk, heads=heads_mode, select="cond")
    with cap:
        attn.to_q.run = to_q_run
        try:
            y1 = run()
        finally:
            del attn.to_q.run
        assert torch.equal(y1, y0)                       # observed, not rerouted: not one bit moves
        assert len(spy.calls) == 1                       # one attn2 layer, one probe launch
        maps = cap.collect()
    call = spy.calls[0]
    fused = name == "T320"
    assert L.XATTN_FUSED and ops.xattn320_ok(c, heads, CAP, INST * lq) == fused
    assert list(maps) == ["transformer_blocks.0.attn2"]
    got = maps["transformer_blocks.0.attn2"]
    nb = INST // 2
    assert call["batch"] == nb and call["lk"] == CAP and call["lk_dev"] is lk_dev and call["heads"] == heads
    assert got.dtype == torch.float32 and got.shape == ((nb * heads if heads_mode == "all" else nb), lq, REAL)
    # the maps against fp64 of the operands the probe handed over
    qv, kv = _canonical(call)
    pre = bool(call.get("q_prescaled"))
    ref, e = AR.reference(qv, kv, call["scale"], n_keys=REAL, prescaled=pre, per_head=heads_mode == "all")
    if heads_mode == "all":                              # head_to_batch_dim order: row b * heads + h
        ref, e = ref.reshape(nb * heads, lq, REAL), e.reshape(nb * heads, lq, REAL)
    ratio = AR.check(got, ref, e, "%s %s maps" % (name, B.tag(dtype)), torch.float32)
    print("%s %s %s: maps max err/bound %.3f" % (name, B.tag(dtype), heads_mode, ratio))
    # the cond half, by pointer offset: the probe's q is the second half of the projection's output, not a copy
    x_in, kw, q_full = proj[-1]
    assert len(proj) == 1
    hm = kw.get("head_major")
    half = q_full[:, nb * lq:] if hm else q_full[nb * lq:]
    assert call["q"].data_ptr() == half.data_ptr() and call["q"].shape == half.shape and pre == bool(hm)
    # ... and that output against the fp64 projection of its input
    acc, e_acc = G.dense_acc(x_in, attn.to_q.w2d)
    qref, qe = G.epilogue(acc, e_acc)
    if hm:
        qref, qe = G.head_major(qref, qe, hm[0], hm[1], hm[2])
    G.check(q_full, qref, qe, "%s %s probe q" % (name, B.tag(dtype)))
    # removed: no probe launch, the same bits, nothing left behind
    y2 = run()
    assert len(spy.calls) == 1 and torch.equal(y2, y0) and _no_leftovers(blk)


def test_accumulate_and_select_all(gpu):
    """accumulate(1 / 2) over two forwards = the mean of the two stored maps: the halvings are exact, each call rounds its
    add once (2 u relative in all, values under the fp32 normal range apart); select="all" keeps every instance, and its
    second half is the cond capture."""
    from dualdiff_amd.networks import layers as L
    from dualdiff_amd.networks.attn_maps import CrossAttnMapCapture
    name, dtype = "T640", torch.float16
    _kind, c, heads, hd, _m, (h, w), seed = B.CASES[name]
    blk = B.make_hip(name, _state_dict(name), dtype)
    lq = h * w
    xs = [G.rand((INST * lq, c), dtype, 7100 + i, device=gpu) for i in range(2)]
    ctx2d = G.rand((INST * CAP, B.CTX_DIM), dtype, 7102, device=gpu)
    lk_dev = torch.tensor([REAL], dtype=torch.int32, device=gpu)

    def run(x):
        with torch.no_grad(), L.context_keys(ctx2d, CAP, lk_dev):
            blk.run(x, INST, h, w, ctx2d, CAP)
    with CrossAttnMapCapture(blk, select="all") as cap:
        stored = []
        for x in xs:
            run(x)
            stored.append(cap.collect()["transformer_blocks.0.attn2"])
        assert stored[0].shape == (INST, lq, REAL)
        epoch = L.CACHE_EPOCH[0]
        cap.accumulate(0.5)
        assert L.CACHE_EPOCH[0] > epoch                  # the weight is an argument of recorded launches
        cap.zero_()
        for x in xs:
            run(x)
        acc = cap.collect()["transformer_blocks.0.attn2"]
    want = (stored[0].double() + stored[1].double()) / 2
    assert bool(((acc.double() - want).abs() <= 2 * AR.U32 * want + AR.FLUSH32).all())
    with CrossAttnMapCapture(blk, select="cond") as cap:
        run(xs[1])
        assert torch.equal(cap.collect()["transformer_blocks.0.attn2"], stored[1][INST // 2:])
    assert _no_leftovers(blk)


# ---- forward graphs ---------------------------------------------------------------------------------------------------------

def test_forward_graph_replay_writes_the_maps_of_an_eager_forward(gpu):
    """A two-level UNet (320: dd_xattn320, 640: unfused) through the PUBLIC forward(): the context (83 tokens) is laid out
    at its capacity (110) and the forward replays a recorded graph; with a capture installed the graph is recorded again,
    ONCE, with the probe launches inside, a replay fills the maps with the bits of an eager forward, and the noise
    prediction keeps its bits before, during and after."""
    from dualdiff_amd.networks import layers as L
    from dualdiff_amd.networks.attn_maps import CrossAttnMapCapture
    from dualdiff_amd.networks.unet_2d_condition_multiview import UNet2DConditionModelMultiview
    dtype = torch.float16
    unet = UNet2DConditionModelMultiview(
        down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"),
        block_out_channels=(320, 640), layers_per_block=1, cross_attention_dim=768, neighboring_view_pair=B.PAIR)
    unet = L.seeded_init_(unet, 5).to(gpu, dtype).eval()
    m = 12
    x = G.rand((m, 4, 8, 10), dtype, 7200, device=gpu)
    ctx = G.rand((m, REAL, 768), dtype, 7201, device=gpu)
    t = torch.tensor(481, device=gpu)

    def fwd():
        with torch.no_grad():
            return unet(x, t, encoder_hidden_states=ctx).sample.clone()
    y_pre = [fwd() for _ in range(3)]                    # eager, recorded, replayed
    graphs = unet.__dict__["_fwd_graphs"]
    assert graphs.captures == 1 and torch.equal(y_pre[0], y_pre[2])
    names = _attn2_names(unet)
    assert len(names) == 4
    cap = CrossAttnMapCapture(unet).install()            # heads="mean", select="cond": the defaults
    unet.graph_forward = False
    y_eager = fwd()
    eager = cap.collect()
    unet.graph_forward = True
    y_rec = fwd()                                        # the key is known: recorded again, with the probes, and replayed
    assert graphs.captures == 2
    for found in cap.probes:
        for _, probe in found.values():
            for buf in probe.buffers.values():
                buf.fill_(float("nan"))
    y_rep = fwd()                                        # a pure replay
    assert graphs.captures == 2
    replay = cap.collect()
    assert torch.equal(y_eager, y_pre[0]) and torch.equal(y_rec, y_pre[0]) and torch.equal(y_rep, y_pre[0])
    assert set(eager) == names and set(replay) == names
    for n in sorted(names):
        lq = 80 if "mid" not in n else 20
        assert eager[n].shape == (m // 2, lq, REAL), (n, eager[n].shape)
        assert torch.equal(replay[n], eager[n]), n
        assert float((eager[n].double().sum(-1) - 1).abs().max()) <= (REAL + 8 + 12) * AR.U32
    cap.remove()
    y_after = [fwd() for _ in range(2)]
    assert torch.equal(y_after[0], y_pre[0]) and torch.equal(y_after[1], y_pre[0]) and _no_leftovers(unet)


# ---- BEVDenoiser ------------------------------------------------------------------------------------------------------------

def test_denoiser_cross_attn_map(gpu, step_models):
    """Two steps of the two-branch step case (the configuration the denoiser tests build): latents keep their bits with a
    capture, cross_attn_map has the reference's layout, the running mean equals the mean of the per-step maps, and
    mean_map is explore_attn.py's gather_layer."""
    from dualdiff_amd.networks.attn_maps import CrossAttnMapCapture
    from dualdiff_amd.pipeline.pipeline_bev_controlnet import BEVDenoiser
    from tests.golden import cases as C
    dtype, steps = torch.float16, 2
    base = _denoiser(step_models, dtype)
    unet, cns = base.unet, base.controlnets
    inp = C.step_inputs(2)
    args = (C.step_latents().cuda().to(dtype), _to_dev(inp["text"], dtype), _to_dev(inp["camera_param"], dtype),
            [_to_dev(inp["boxes_bg"], dtype), _to_dev(inp["boxes_fg"], dtype)],
            [_to_dev(inp["cond_bg"], dtype), _to_dev(inp["cond_fg"], dtype)])
    with torch.no_grad():
        base.run(steps)
    lat0 = base.latents.clone()

    def run(cap, reduce=None):
        den = BEVDenoiser(unet, cns, guidance_scale=2.0, num_inference_steps=50, attn_maps=cap, attn_maps_reduce=reduce)
        with torch.no_grad():
            den.set_inputs(*args)
            den.run(steps)
        assert torch.equal(den.latents, lat0)            # bit-identical latents, whatever is captured
        return den

    ts = [int(base.timesteps[i]) for i in range(steps)]
    lc = 1 + C.STEP_LTXT + C.STEP_NBOX
    inst = C.N_CAM                                       # the cond half of 2 x 6 instances
    u_names = _attn2_names(unet)
    c_names = {"nets.%d.%s" % (i, n) for i, cn in enumerate(cns) for n in _attn2_names(cn)}
    # heads="all": the reference's own tensors
    with CrossAttnMapCapture(unet, *cns, heads="all") as cap:
        cam = run(cap).cross_attn_map
    assert set(cam) == {"cnet", "unet"} and len(cam["cnet"]) == 2 and cam["cnet"][1] == {}
    assert list(cam["unet"]) == ts and list(cam["cnet"][0]) == ts and all(type(k) is int for k in cam["unet"])
    mods = dict(unet.named_modules())
    for tt in ts:
        assert set(cam["unet"][tt]) == u_names and set(cam["cnet"][0][tt]) == c_names
        for n, mp in cam["unet"][tt].items():
            assert mp.dtype == torch.float32 and mp.shape[0] == inst * mods[n].heads and mp.shape[2] == lc, (n, mp.shape)
            assert mp.shape[1] in (28 * 50, 14 * 25, 7 * 13, 4 * 7)
    assert not torch.equal(cam["unet"][ts[0]]["mid_block.attentions.0.transformer_blocks.0.attn2"],
                           cam["unet"][ts[1]]["mid_block.attentions.0.transformer_blocks.0.attn2"])
    # heads="mean": per step, then the running mean of the same sample
    cap = CrossAttnMapCapture(unet, *cns)
    with cap:
        per_step = run(cap).cross_attn_map
        mean = run(cap, reduce="mean").cross_attn_map
        gathered = cap.mean_map(hw=(28, 50), model=unet)                   # from the accumulated buffers
        from_steps = cap.mean_map(hw=(28, 50), model=unet, maps=[per_step["unet"][tt] for tt in ts])
    assert list(mean["unet"]) == ["mean"] and set(mean["unet"]["mean"]) == u_names
    assert set(mean["cnet"][0]["mean"]) == c_names and mean["cnet"][1] == {}
    for slot_mean, slot_steps in ((mean["unet"]["mean"], per_step["unet"]), (mean["cnet"][0]["mean"], per_step["cnet"][0])):
        for n, mp in slot_mean.items():
            want = sum(slot_steps[tt][n].double() for tt in ts) / steps
            assert mp.shape == want.shape and mp.shape[0] == inst
            assert bool(((mp.double() - want).abs() <= (steps + 2) * AR.U32 * want).all()), n
    # gather_layer (explore_attn.py:97-105) in float64 on the collected maps: mean over steps, then over the 28 x 50
    # layers whose name contains "up" and does not start with "mid"
    layers = [n for n in per_step["unet"][ts[0]] if "up" in n and not n.startswith("mid")
              and per_step["unet"][ts[0]][n].shape[1] == 28 * 50]
    assert len(layers) == 3
    want = torch.stack([torch.stack([per_step["unet"][tt][n].double() for tt in ts]).mean(0) for n in layers]).mean(0)
    assert from_steps.shape == (inst, 28 * 50, lc) and gathered.shape == from_steps.shape
    tol = (steps + len(layers) + 4) * AR.U32             # two fp32 means of positive numbers, on top of the buffers' own
    assert bool(((from_steps.double() - want).abs() <= tol * want).all())
    assert bool(((gathered.double() - want).abs() <= (tol + (steps + 2) * AR.U32) * want).all())
    assert _no_leftovers(unet, *cns)
