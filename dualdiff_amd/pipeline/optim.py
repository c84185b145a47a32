"""The optimizer step of the reference's training loop on the GPU: `FusedAdamW`.

runner/multiview_runner.py:512-521 ends a training step with `accelerator.clip_grad_norm_(params, max_grad_norm)`,
`optimizer.step()` (torch.optim.AdamW, :256-276, under the GradScaler that `mixed_precision: fp16` installs) and
`lr_scheduler.step()`.  `FusedAdamW.step()` is those three lines as ONE call of `ops.adamw_step`: three launches over a
descriptor table of the parameters, the step count, the learning rate of the schedule and the skip decision in device
memory, nothing read back, so a step can be captured into a graph.  The 16-bit tensors the HIP modules read (`shadows`)
are refreshed in the same pass and count a version, which is what `layers.derived` keys the packed weights on.

Differences from the torch chain, all deliberate:
  * the gradients are not rewritten: after step() they still hold the scaled, unclipped values;
  * the schedule is a device table indexed by the number of steps TAKEN (a skipped step does not advance it, as
    accelerate's scheduler wrapper arranges), not a scheduler object;
  * one step count for all parameters, where torch keeps one per parameter: a parameter whose gradient is None is left
    alone, but its bias correction, once it gets a gradient, is that of the common count.
"""
import math

import torch

from .. import ops

_REFUSED = ("amsgrad", "maximize", "use_8bit_adam")


# ---- the schedule ------------------------------------------------------------------------------------------------------
# The lambdas of diffusers.optimization.get_scheduler that the reference's configs name (configs/runner/default.yaml:35:
# cosine), restated; diffusers is not a dependency, so their parity is unpinned.

def constant():
    return lambda step: 1.0


def constant_with_warmup(lr_warmup_steps):
    def f(step):
        if step < lr_warmup_steps:
            return float(step) / float(max(1.0, lr_warmup_steps))
        return 1.0
    return f


def cosine(lr_warmup_steps, max_train_steps, lr_num_cycles=0.5):
    def f(step):
        if step < lr_warmup_steps:
            return float(step) / float(max(1, lr_warmup_steps))
        progress = float(step - lr_warmup_steps) / float(max(1, max_train_steps - lr_warmup_steps))
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(lr_num_cycles) * 2.0 * progress)))
    return f


def lr_table(base_lr, lr_lambda, n, device=None):
    """base_lr * lr_lambda(k) for k = 0 .. n - 1, evaluated in float64 and rounded to fp32 once: entry k is the learning
    rate of the step taken after k steps (torch's LambdaLR sets base_lr * lr_lambda(0) before the first step)."""
    if n < 1:
        raise ValueError("lr_table: at least one entry, got n = %r" % (n,))
    return torch.tensor([float(base_lr) * float(lr_lambda(k)) for k in range(int(n))], dtype=torch.float64).to(
        torch.float32).to(device)


# ---- the optimizer -----------------------------------------------------------------------------------------------------

class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW + clip_grad_norm_ + GradScaler's unscale and skip + the learning-rate schedule, fused
    (ops.adamw_step).  params: fp32 tensors of one GPU, contiguous.  shadows: {parameter: fp16 / bf16 tensor of its shape}
    to refresh with every taken step — typically the HIP module's own Parameter.  lr_table: 1-D fp32 device tensor indexed
    by the number of steps taken so far (its last entry for every later step); default: the one entry `lr`.

    step() honours the `grad_scale` / `found_inf` attributes a torch.amp.GradScaler sets (_step_supports_amp_scaling) and
    a `grad_scale` argument; `found_inf`, `grad_norm`, `clip_coef`, `steps_taken`, `skipped` are device tensors, views of
    the state block.  state_dict() / load_state_dict() use torch.optim.AdamW's layout."""
    _step_supports_amp_scaling = True

    def __init__(self, params, lr=8e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None, shadows=None,
                 lr_table=None, **refused):
        for name, value in refused.items():
            if name not in _REFUSED:
                raise TypeError("FusedAdamW: unknown argument %r" % name)
            if value:
                raise ValueError("FusedAdamW: %s is not supported" % name)
        if not lr >= 0.0 or not eps >= 0.0 or not weight_decay >= 0.0 or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError("FusedAdamW: lr >= 0, betas in [0, 1), eps >= 0, weight_decay >= 0, got %r, %r, %r, %r"
                             % (lr, betas, eps, weight_decay))
        if max_grad_norm is not None and not max_grad_norm >= 0.0:
            raise ValueError("FusedAdamW: max_grad_norm must be None or >= 0, got %r" % (max_grad_norm,))
        # the keys of torch.optim.AdamW's param_groups, so that either optimizer loads the other's state
        defaults = dict(torch.optim.AdamW([torch.zeros(1)]).defaults)
        defaults.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self._check_groups()
        self.max_grad_norm = max_grad_norm
        ps = self._params()
        if not ps:
            raise ValueError("FusedAdamW: no parameters")
        self._device = ps[0].device
        shadows = dict(shadows or {})
        known = {id(p) for p in ps}
        for p in shadows:
            if id(p) not in known:
                raise ValueError("FusedAdamW: a shadow is given for a tensor that is not a parameter")
        self._shadows = [shadows.get(p) for p in ps]
        for p in ps:
            self.state[p] = {"step": torch.tensor(0.0), "exp_avg": torch.zeros_like(p, memory_format=torch.preserve_format),
                             "exp_avg_sq": torch.zeros_like(p, memory_format=torch.preserve_format)}
        self._user_lr_table = lr_table is not None
        if lr_table is None:
            lr_table = torch.full((1,), float(lr), dtype=torch.float32, device=self._device)
        elif not isinstance(lr_table, torch.Tensor) or lr_table.dtype != torch.float32 or lr_table.dim() != 1 \
                or lr_table.numel() < 1 or lr_table.device != self._device:
            raise ValueError("FusedAdamW: lr_table must be a 1-D fp32 tensor on %s with at least one entry" % self._device)
        self._lr_table = lr_table.contiguous()
        self._lr_filled = float(lr)
        self._scale_value, self._scale_tensor = None, None
        self._grad_ptrs = None
        self._table = None
        self._chunks = ops.adamw_chunks([p.numel() for p in ps]).to(self._device)
        self._workspace = torch.empty((ops.adamw_workspace_bytes(self._chunks.shape[0]),), dtype=torch.uint8,
                                      device=self._device)
        self._state_block = None
        self._set_state_block(0, 0)
        self._upload_table(ps, now=False)          # validates every row before the first launch

    # -- layout --------------------------------------------------------------------------------------------------------
    def _params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _check_groups(self):
        first = self.param_groups[0]
        for name in _REFUSED[:2]:
            if any(g.get(name) for g in self.param_groups):
                raise ValueError("FusedAdamW: %s is not supported" % name)
        for g in self.param_groups[1:]:
            for key in ("lr", "betas", "eps", "weight_decay"):
                if g[key] != first[key]:
                    raise ValueError("FusedAdamW: parameter groups with different hyper-parameters are not supported "
                                     "(%s: %r and %r)" % (key, first[key], g[key]))

    def _set_state_block(self, step, skipped):
        block = ops.adamw_state(step, self.param_groups[0]["betas"], skipped).to(self._device)
        if self._state_block is None:
            self._state_block = block
        else:
            self._state_block.copy_(block)         # keep the address: the views below, and a captured graph, hold it

    def _field(self, name):
        return ops.adamw_state_field(self._state_block, name)

    # `found_inf` is both: what a GradScaler sets (and deletes) around step() is kept aside as the incoming mark; what is
    # read is the step's own decision, the int32 of the state block.
    def _get_found_inf(self):
        return self._field("found_inf")

    def _set_found_inf(self, value):
        self._found_inf_in = value

    def _del_found_inf(self):
        self._found_inf_in = None

    found_inf = property(_get_found_inf, _set_found_inf, _del_found_inf)
    _found_inf_in = None
    grad_norm = property(lambda self: self._field("grad_norm"))
    clip_coef = property(lambda self: self._field("clip_coef"))
    steps_taken = property(lambda self: self._field("step"))
    skipped = property(lambda self: self._field("skipped"))

    def _rows(self, ps):
        return [(p, p.grad, self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"], s) for p, s in zip(ps, self._shadows)]

    def _upload_table(self, ps, now=True):
        if not now and self._device.type != "cuda":
            # parameters on the host: the state can be kept, saved and loaded; the first step() raises (no CPU fallback)
            self._grad_ptrs = None
            return
        rows = self._rows(ps)
        host, shadow_dtype = ops.adamw_table(rows)
        self._shadow_dtype = shadow_dtype or torch.float16
        # one pinned block per upload: the host allocator keeps it until the asynchronous copy has read it
        host = host.pin_memory()
        if self._table is None:
            self._table = torch.empty_like(host, device=self._device)
        self._table.copy_(host, non_blocking=True)
        self._grad_ptrs = [0 if r[1] is None else r[1].data_ptr() for r in rows]
        self._touched = [t for r in rows if r[1] is not None for t in (r[0], r[2], r[3], r[4])
                         if t is not None and not t.is_inference()]

    # -- the step ------------------------------------------------------------------------------------------------------
    def _scale(self, grad_scale):
        if grad_scale is None:
            return None
        if isinstance(grad_scale, torch.Tensor):
            return grad_scale.reshape(1)
        if self._scale_value != float(grad_scale):
            self._scale_tensor = torch.full((1,), float(grad_scale), dtype=torch.float32, device=self._device)
            self._scale_value = float(grad_scale)
        return self._scale_tensor

    @torch.no_grad()
    def step(self, closure=None, *, grad_scale=None):
        """One step.  grad_scale: a number or a one-element fp32 device tensor by which the gradients are divided (as the
        scaler does it: times fp32(1 / float64(scale))); default: the `grad_scale` attribute a GradScaler set, else 1.
        Reads nothing back: whether the step was taken is `found_inf` / `steps_taken` / `skipped`, on the device."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._device.type != "cuda":
            raise RuntimeError("FusedAdamW runs on the GPU only (the parameters are on %s); there is no CPU fallback"
                               % self._device)
        self._check_groups()
        group = self.param_groups[0]
        ps = self._params()
        ptrs = [0 if p.grad is None else p.grad.data_ptr() for p in ps]
        if ptrs != self._grad_ptrs:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FusedAdamW: a gradient moved (or appeared, or went) during a stream capture: the captured "
                                   "step reads the addresses of its table; keep the gradient buffers (set_to_none=False)")
            self._upload_table(ps)
        if not self._user_lr_table and float(group["lr"]) != self._lr_filled:
            self._lr_table.fill_(float(group["lr"]))
            self._lr_filled = float(group["lr"])
        scale = self._scale(grad_scale if grad_scale is not None else getattr(self, "grad_scale", None))
        found_inf = self._found_inf_in
        ops.adamw_step(self._table, self._chunks, self._state_block, self._lr_table, betas=group["betas"], eps=group["eps"],
                       weight_decay=group["weight_decay"], max_grad_norm=self.max_grad_norm, grad_scale=scale,
                       found_inf=None if found_inf is None else found_inf.reshape(1), shadow_dtype=self._shadow_dtype,
                       workspace=self._workspace, written=self._touched)
        return loss

    # -- state ---------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """torch.optim.AdamW's layout.  Reads the step count back (the one place that does)."""
        step = float(int(self.steps_taken.item()))
        for p in self._params():
            self.state[p]["step"] = torch.tensor(step)
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """Loads a state in torch.optim.AdamW's layout (ours, or one a torch.optim.AdamW wrote).  The parameters' step
        counts must agree; the running beta products restart from Python's beta ** step."""
        for g in state_dict["param_groups"]:
            for name in _REFUSED[:2]:
                if g.get(name):
                    raise ValueError("FusedAdamW: a state with %s cannot be loaded" % name)
        steps = {int(float(s["step"])) for s in state_dict["state"].values() if "step" in s}
        if len(steps) > 1:
            raise ValueError("FusedAdamW: the parameters of this state have taken different numbers of steps (%s); "
                             "one count is kept for all" % sorted(steps))
        super().load_state_dict(state_dict)
        self._check_groups()
        for p in self._params():
            st = self.state[p]
            for key in ("exp_avg", "exp_avg_sq"):
                t = st.get(key)
                st[key] = torch.zeros_like(p, memory_format=torch.preserve_format) if t is None else \
                    t.to(device=p.device, dtype=torch.float32).contiguous()
        self._set_state_block(steps.pop() if steps else 0, 0)
        if not self._user_lr_table:
            self._lr_table.fill_(float(self.param_groups[0]["lr"]))
            self._lr_filled = float(self.param_groups[0]["lr"])
        self._upload_table(self._params(), now=False)
