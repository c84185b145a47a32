"""Cross-attention maps of the text / camera / box context — the `cross_attn_map` of the reference's explore pipeline
(pipeline/explore_pipeline_bev_controlnet.py:352-354,437-453,494-500,576; saved by tools/explore_unet.py:224-232 and
turned into per-token heat maps by tools/explore_attn.py:97-151: `mean_map` below is its `gather_layer`, and
pipeline/attn_output.py's `AttnMapRender` makes its pictures, `view_images_{view}.png` / `view_images_{view}box.png`, on
the device from this capture).

The reference gets them by installing a processor that calls `attn.get_attention_scores` on every `attn2` layer
(tools/unet_modify.py:7-57) and keeps the conditional CFG half (`chunk(2)[1]`).  Here a `CrossAttnMapCapture` OBSERVES
the built-in path instead: `Attention.run_cross` hands the q and k it already has (or, on the dd_xattn320 path where q
never reaches memory, the q of one extra to_q GEMM) to `ops.attention_probs`, which writes float32 probabilities into a
buffer owned by the capture.  Nothing the step computes is rerouted: hidden states and latents keep their bits, and the
probe launches are recorded into the forward graphs like any other launch.

Not captured: the extra box / class attentions of `Adapter_XFormersAttnProcessor` (the reference's
`cross_attn_viz_c_adapter`, which its own analysis script notes is empty, tools/explore_attn.py:62) and the SFA
attention (txt_con_fusion.py) — neither goes through `Attention.run_cross`.  A layer whose probe never fired is simply
absent from `collect()`."""
import torch

from .. import ops as O
from . import layers as L

_ATTR = "_attn_probe"


class _Probe:
    """What `Attention.run_cross` calls while a capture is installed on its module."""

    def __init__(self, owner, name):
        self.owner, self.name = owner, name
        self.buffers = {}              # (instances, heads, lq, capacity) -> float32 buffer: one address per shape, for good
        self.last = None               # (key, lk_dev) of the most recent python-level call

    def __call__(self, attn, q, k, batch, lq, lk, q_prescaled, lk_dev):
        own = self.owner
        b0 = batch // 2 if own.select == "cond" and batch > 1 else 0       # the CFG batch is [uncond ; cond]
        nb = batch - b0
        if b0:
            q = q[:, b0 * lq:] if q.dim() == 3 else q[b0 * lq:]
            k = k[b0 * lk:]
        key = (nb, attn.heads, lq, lk)
        buf = self.buffers.get(key)
        if buf is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("attn_maps: layer %s first seen inside a graph capture; run the shape eagerly once" % self.name)
            shape = (nb, attn.heads, lq) if own.heads == "all" else (nb, lq)
            # rows at a pitch of whole float4 groups; zeros, so that an accumulation starts from nothing
            buf = self.buffers[key] = torch.zeros(shape + ((lk + 3) // 4 * 4,), dtype=torch.float32, device=q.device)[..., :lk]
        w = own.weight
        O.attention_probs(q, k, nb, lq, lk, attn.heads, attn.dim_head, attn.scale, q_prescaled=q_prescaled,
                          per_head=own.heads == "all", out=buf, accumulate=w is not None, weight=1.0 if w is None else w,
                          lk_dev=lk_dev)
        self.last = (key, lk_dev)

    def current(self):
        """(buffer trimmed to the real key count, instances, heads) of the most recent call, or None."""
        if self.last is None:
            return None
        key, lk_dev = self.last
        n = key[3] if lk_dev is None else max(1, min(int(lk_dev[0].item()), key[3]))
        return self.buffers[key][..., :n], key[0], key[1]


class CrossAttnMapCapture:
    """`CrossAttnMapCapture(unet, cnet, ..., heads="mean" | "all", select="cond" | "all", layers=None)`.

    heads:  "mean" (default) keeps the mean over the heads, (instances, lq, n) per layer — what every use in the
            reference's analysis reduces to first; "all" keeps the reference's own tensor, (instances * heads, lq, n) in
            `head_to_batch_dim` order (row b * heads + h), `heads` times the memory.
    select: "cond" keeps the second half of the batch (the conditional CFG half, the reference's `chunk(2)[1]`);
            "all" every batch entry.
    layers: optional predicate on the module name.

    install() attaches a probe to every `Attention` module whose qualified name contains "attn2" (the reference's rule)
    and starts a new cache epoch, so that forward graphs are recorded again with the probe launches inside; remove()
    detaches them.  Usable as a context manager.  Buffers are allocated at the first (eager) call of a shape, at the
    context CAPACITY, and never move: a recorded graph keeps writing to them."""

    def __init__(self, *models, heads="mean", select="cond", layers=None):
        if heads not in ("mean", "all"):
            raise ValueError("heads is 'mean' or 'all'")
        if select not in ("cond", "all"):
            raise ValueError("select is 'cond' or 'all'")
        if not models:
            raise ValueError("CrossAttnMapCapture needs at least one model")
        self.models = list(models)
        self.heads, self.select, self.layers = heads, select, layers
        self.weight = None             # None: every forward STORES its maps; a float: it ADDS weight * map
        self.probes = []               # per model: {name: (module, probe)}
        self.installed = False

    # ------------------------------------------------------------------------ install ----
    def install(self):
        if self.installed:
            return self
        self.probes = []
        for model in self.models:
            found = {}
            for name, mod in model.named_modules():
                if isinstance(mod, L.Attention) and "attn2" in name and (self.layers is None or self.layers(name)):
                    if _ATTR in mod.__dict__:
                        raise RuntimeError("attn_maps: %s already carries a capture" % name)
                    found[name] = (mod, _Probe(self, name))
            self.probes.append(found)
        for found in self.probes:
            for mod, probe in found.values():
                mod.__dict__[_ATTR] = probe
        self.installed = True
        self._new_epoch()
        return self

    def remove(self):
        if not self.installed:
            return
        for found in self.probes:
            for mod, _ in found.values():
                mod.__dict__.pop(_ATTR, None)
        self.installed = False
        self.probes = []
        self._new_epoch()

    @staticmethod
    def _new_epoch():
        # graphs recorded with another set of probe launches are over (model_base.ForwardGraphs).  The epoch only ever
        # grows: graphs recorded under an old value hold addresses of that time and must never match again.
        L.CACHE_EPOCH[0] += 1

    def __enter__(self):
        return self.install()

    def __exit__(self, *exc):
        self.remove()
        return False

    # ----------------------------------------------------------------------- the maps ----
    def accumulate(self, weight=1.0):
        """Subsequent forwards ADD weight * map into the buffers (weight = 1 / steps: the buffers end up holding the mean
        over the steps); None goes back to storing.  A new cache epoch: the weight is an argument of recorded launches."""
        weight = None if weight is None else float(weight)
        if weight != self.weight:
            self.weight = weight
            self._new_epoch()

    def zero_(self):
        for found in self.probes:
            for _, probe in found.values():
                for buf in probe.buffers.values():
                    buf.zero_()

    def collect(self, model=None, copy=True):
        """{name: map} of the most recent forward of `model` (index or module; default: the only one), trimmed to the real
        key count: (instances, lq, n), or (instances * heads, lq, n) for heads="all".  Device-to-device copies unless
        copy=False (then views of the live buffers where the layout allows)."""
        out = {}
        for name, (_, probe) in self._of(model).items():
            cur = probe.current()
            if cur is None:
                continue
            buf, nb, hd = cur
            if copy:
                buf = buf.clone(memory_format=torch.contiguous_format)
            if self.heads == "all":
                buf = buf.reshape(nb * hd, buf.shape[2], buf.shape[3])         # head_to_batch_dim order
            out[name] = buf
        return out

    def _of(self, model):
        if model is None:
            if len(self.probes) != 1:
                raise ValueError("collect(model=...): this capture observes %d models" % len(self.probes))
            return self.probes[0]
        if isinstance(model, int):
            return self.probes[model]
        for m, found in zip(self.models, self.probes):
            if m is model:
                return found
        raise ValueError("that model is not observed by this capture")

    def mean_map(self, hw=(28, 50), layer_filter=None, model=None, maps=None):
        """`gather_layer` of tools/explore_attn.py:97-105: the mean over heads, over steps and over the layers whose
        lq == h * w, whose name contains "up" and does not start with "mid" -> (instances, h * w, n) float32.
        maps: a list of per-step {name: map} dicts (what collect() returned after each step); None: the buffers as they
        stand — after accumulate(1 / steps) they hold the mean over the steps already."""
        keep = layer_filter or (lambda name: "up" in name and not name.startswith("mid"))
        steps = [self.collect(model, copy=False)] if maps is None else list(maps)
        per_layer = []
        for name in steps[0]:
            if not keep(name) or steps[0][name].shape[-2] != hw[0] * hw[1]:
                continue
            per_step = []
            for s in steps:
                t = s[name].float()
                if self.heads == "all":
                    hd = self._heads_of(name, model)
                    t = t.reshape(t.shape[0] // hd, hd, t.shape[1], t.shape[2]).mean(1)
                per_step.append(t)
            per_layer.append(torch.stack(per_step).mean(0))
        if not per_layer:
            raise ValueError("no captured layer has %d x %d queries" % tuple(hw))
        return torch.stack(per_layer).mean(0)

    def _heads_of(self, name, model):
        return self._of(model)[name][0].heads
