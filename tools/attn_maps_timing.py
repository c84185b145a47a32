"""Cross-attention maps (networks/attn_maps.CrossAttnMapCapture): what capturing them costs the fused sampler, against
the route that needs no kernel of its own.

    python tools/attn_maps_timing.py                 # steps/s of the bench workload, three alternating rounds -> stdout

The workload is bench.py's (config 2: two ControlNet branches, 12 instances of 28 x 50 latents, 98 context tokens, fp16).
Per round, each after a warm-up run of its own, wall clock around `BEVDenoiser.run(steps)` + a device synchronise:
  plain     no capture (the step graph bench.py's headline replays);
  capture   CrossAttnMapCapture(unet, both ControlNets), heads="mean", attn_maps_reduce="mean": the probes are recorded
            into the step graph and add 1 / steps of every map into the capture's buffers;
  per-step  the same capture with the per-step maps kept (device-to-device copies after every replay);
  foreign   the route available without dd_attn_probs: a processor of the diffusers protocol on every attn2 layer that
            calls `attn.get_attention_scores` (plain torch), keeps the cond half of the probabilities on the module and
            is read out to the host after every step — the reference's way (tools/unet_modify.py:7-57,
            pipeline/explore_pipeline_bev_controlnet.py:437-453,494-500).  Foreign processors run eagerly (no graphs).
Then one eager step on ONE stream under ops.KernelTimer with and without the capture: the summed device time of
dd_attn_probs_kernel when nothing runs beside it (inside the step graph it shares the machine with the other branches'
streams), and how many other launches the capture adds (the to_q GEMMs of the dd_xattn320 layers), next to what the
capture adds to the step."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from dualdiff_amd import ops  # noqa: E402
from dualdiff_amd.networks.attn_maps import CrossAttnMapCapture  # noqa: E402
from dualdiff_amd.networks.layers import Attention, HIPAttnProcessor  # noqa: E402
from dualdiff_amd.pipeline.pipeline_bev_controlnet import BEVDenoiser  # noqa: E402


class KeepProbsProcessor:
    """Cross-attention through the module's diffusers surface, keeping softmax(scale q k^T) of the cond half."""

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, **kw):
        ctx = hidden_states if encoder_hidden_states is None else encoder_hidden_states
        q = attn.head_to_batch_dim(attn.to_q(hidden_states))
        k = attn.head_to_batch_dim(attn.to_k(ctx))
        v = attn.head_to_batch_dim(attn.to_v(ctx))
        probs = attn.get_attention_scores(q, k)
        attn.attn_probs_original = probs.chunk(2)[1]
        return attn.to_out[0](attn.batch_to_head_dim(torch.bmm(probs, v)))


def attn2_layers(models):
    return [m for net in models for n, m in net.named_modules() if isinstance(m, Attention) and "attn2" in n]


def timed(den, inputs, steps):
    with torch.no_grad():
        den.set_inputs(*inputs)
        lat0 = den.lat2.clone()
        den.run(steps)                                   # warm-up: packs, tunes, records the step graph
        den.lat2.copy_(lat0)                             # the same sample again (set_inputs would drop the graph)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        den.run(steps)
        torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU")
    dev, dtype = torch.device("cuda:0"), torch.float16
    print("# %s, torch %s, %d steps per run, %d rounds" % (torch.cuda.get_device_name(0), torch.__version__, args.steps, args.rounds))
    unet, cns = bench.build_models(dtype, dev)
    inputs = bench.synthetic_inputs(1, dtype, dev, seed=11)
    models = [unet] + cns
    layers = attn2_layers(models)

    def plain():
        return timed(BEVDenoiser(unet, cns, num_inference_steps=50), inputs, args.steps)

    def capture(reduce):
        with CrossAttnMapCapture(*models) as cap:
            return timed(BEVDenoiser(unet, cns, num_inference_steps=50, attn_maps=cap, attn_maps_reduce=reduce), inputs,
                         args.steps)

    def foreign():
        for m in layers:
            m.set_processor(KeepProbsProcessor())
        den = BEVDenoiser(unet, cns, num_inference_steps=50, use_graph=False)
        step = den.step
        kept = {}

        def step_and_read(i):
            step(i)
            for j, m in enumerate(layers):               # to the host after every step, as the reference does
                kept[j] = m.attn_probs_original.detach().cpu()
        den.step = step_and_read
        try:
            return timed(den, inputs, args.steps)
        finally:
            for m in layers:
                m.set_processor(HIPAttnProcessor())
                m.__dict__.pop("attn_probs_original", None)

    legs = (("plain", plain), ("capture", lambda: capture("mean")), ("per-step", lambda: capture(None)), ("foreign", foreign))
    rates = {name: [] for name, _ in legs}
    for r in range(args.rounds):
        for name, fn in legs:
            rates[name].append(fn())
            print("round %d %-9s %8.2f steps/s" % (r, name, rates[name][-1]), flush=True)
    for name, _ in legs:
        v = rates[name]
        print("%-9s median %8.2f steps/s   (min %.2f, max %.2f)   %.3f of plain"
              % (name, statistics.median(v), min(v), max(v), statistics.median(v) / statistics.median(rates["plain"])))

    # where the capture's time goes: one eager step under the per-launch timer, with and without the probes
    def eager_step(cap):
        # one stream: with the branches side by side an event pair also times whatever runs beside its launch
        den = BEVDenoiser(unet, cns, num_inference_steps=50, use_graph=False, parallel_branches=False, attn_maps=cap)
        with torch.no_grad():
            den.set_inputs(*inputs)
            den.step(0)
            torch.cuda.synchronize()
            timer = ops.KernelTimer()
            timer.calibrate()
            ops.set_timer(timer)
            try:
                den.step(1)
                return timer.summary()
            finally:
                ops.set_timer(None)
    base = eager_step(None)
    with CrossAttnMapCapture(*models) as cap:
        probed = eager_step(cap)
    cnt = lambda s: sum(d["count"] for d in s.values())
    pk = [d for n, d in probed.items() if n.startswith("dd_attn_probs_kernel")]
    n_pk, ms_pk = sum(d["count"] for d in pk), sum(d["ms"] for d in pk)
    per_step = 1e3 / statistics.median(rates["capture"]) - 1e3 / statistics.median(rates["plain"])
    print("the capture adds %.3f ms to the %.3f ms step" % (per_step, 1e3 / statistics.median(rates["plain"])))
    print("  dd_attn_probs_kernel, one stream, eager: %d launches, %.3f ms in all (%.1f us each), %.1f MB read and written"
          % (n_pk, ms_pk, 1e3 * ms_pk / max(1, n_pk), sum(d["bytes"] for d in pk) / 1e6))
    print("  other timed launches added (the to_q GEMMs of the dd_xattn320 layers): %d of %d" % (cnt(probed) - cnt(base) - n_pk, cnt(probed)))


if __name__ == "__main__":
    main()
