"""fp64 restatements for the given-view sampling tests — TEST INFRASTRUCTURE ONLY.

`reference_loop` restates the loop of the reference's StableDiffusionBEVControlNetGivenViewPipeline
(pipeline/pipeline_bev_controlnet_given_view.py) procedurally: the pre-loop noising of :263-276, the per-step
overwrite of :283-295 at the TOP of every step, and the noise replacement of :380-389 after guidance, with the
per-(i, j) Python loops of the reference (its shadowing of the step index by the inner `for i` loops is not
reproduced: it only touched the progress bar).  The scheduler is oracle.unipc.UniPCRestated or `DDIMRestated`
below (DDIMScheduler.step with eta = 0, steps_offset 1, set_alpha_to_one False, the SD-v1.5 table).

`fused_loop` emulates the product's per-element rule on the host: the pre-loop noising with the `t0` row of
schedulers.given_view_table, then per step the scheduler update with the given views' store replaced by
row[0] c + row[1] n0 when row[2] != 0 (mode 1: the NEXT step's overwrite fused into this step's store) or their
guided noise replaced by n0 (mode 2).

Both are driven by a callable `model(x, t) -> eps2` ((2, b*n, ...) noise predictions, uncond first) and take
`dtype`: None (fp64 throughout) or the storage type, in which case the latents, the guided noise and n0 are rounded
to it where the fused sampler stores them.
"""
import numpy as np
import torch

from oracle.unipc import UniPCRestated


def alphas_cumprod(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012):
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float64) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def add_noise(acp, c, noise, t):
    """scheduler.add_noise(original_samples, noise, timesteps) for one timestep."""
    return acp[int(t)].sqrt() * c + (1.0 - acp[int(t)]).sqrt() * noise


class DDIMRestated:
    """diffusers DDIMScheduler.set_timesteps / .step (eta = 0, epsilon prediction) for SD-v1.5."""

    def __init__(self, num_train_timesteps=1000, steps_offset=1):
        self.acp = alphas_cumprod(num_train_timesteps)
        self.num_train_timesteps = num_train_timesteps
        self.steps_offset = steps_offset

    def set_timesteps(self, num_inference_steps):
        self.ratio = self.num_train_timesteps // num_inference_steps
        self.timesteps = (np.arange(0, num_inference_steps) * self.ratio)[::-1].copy().astype(np.int64) + self.steps_offset
        return self.timesteps

    def step(self, eps, t, sample):
        a_t = self.acp[int(t)]
        prev = int(t) - self.ratio
        a_p = self.acp[prev] if prev >= 0 else self.acp[0]                # set_alpha_to_one = False
        x0 = (sample - (1 - a_t).sqrt() * eps) / a_t.sqrt()
        return a_p.sqrt() * x0 + (1 - a_p).sqrt() * eps


def make_scheduler(sampler):
    return DDIMRestated() if sampler == "ddim" else UniPCRestated()


def _round(x, dtype):
    return x if dtype is None else x.to(dtype).double()


def _guided(eps2, guidance, dtype):
    eps2 = eps2.double()
    return _round(eps2[0] + guidance * (eps2[1] - eps2[0]), dtype)


def reference_loop(sampler, steps, latents, conditional_latents, change_every_input, model, guidance=2.0, dtype=None,
                   run=None, after_step=None):
    """The reference's given-view loop.  latents (b, n, c, h, w); conditional_latents: b x n list of lists of
    (c, h, w) tensors or None.  Runs the first `run` steps (default all); after_step(k, latents) is called after
    each.  Returns the latents (fp64) — after a truncated run (run < steps) as step `run` would start from them
    (with its overwrite of :283-295 applied), which is what the fused sampler holds between steps."""
    sch = make_scheduler(sampler)
    timesteps = sch.set_timesteps(steps)
    acp = alphas_cumprod()
    b, n = latents.shape[:2]
    latents = _round(latents.double(), dtype).clone()
    original_noise = latents.clone()                                        # :264
    if not change_every_input:                                              # :265-276
        for i in range(b):
            for j in range(n):
                if conditional_latents[i][j] is not None:
                    latents[i, j] = _round(add_noise(acp, conditional_latents[i][j].double(), latents[i, j],
                                                     timesteps[0]), dtype)
    for k, t in enumerate(timesteps[:run]):
        if change_every_input:                                              # :283-295
            for i in range(b):
                for j in range(n):
                    if conditional_latents[i][j] is not None:
                        latents[i, j] = _round(add_noise(acp, conditional_latents[i][j].double(),
                                                         original_noise[i, j], t), dtype)
        eps2 = model(latents.reshape(b * n, *latents.shape[2:]), int(t))
        noise_pred = _guided(eps2, guidance, dtype).reshape(latents.shape)
        if not change_every_input:                                          # :380-389
            for i in range(b):
                for j in range(n):
                    if conditional_latents[i][j] is not None:
                        noise_pred[i, j] = original_noise[i, j]
        latents = _round(sch.step(noise_pred, int(t), latents), dtype)
        if after_step is not None:
            after_step(k, latents)
    if change_every_input and run is not None and run < len(timesteps):
        for i in range(b):
            for j in range(n):
                if conditional_latents[i][j] is not None:
                    latents[i, j] = _round(add_noise(acp, conditional_latents[i][j].double(), original_noise[i, j],
                                                     timesteps[run]), dtype)
    return latents


def fused_loop(sampler, steps, latents, clean, given, mode, model, t0, gcoef, guidance=2.0, dtype=None):
    """The fused per-element rule: clean (b, n, c, h, w), given bool (b, n), mode 1 / 2, (t0, gcoef) =
    schedulers.given_view_table(timesteps, dtype=torch.float64)."""
    sch = make_scheduler(sampler)
    timesteps = sch.set_timesteps(steps)
    b, n = latents.shape[:2]
    x = _round(latents.double(), dtype).clone()
    n0 = x.clone()
    clean = clean.double()
    g = given.reshape(b, n, *([1] * (x.dim() - 2))).expand_as(x)
    x = torch.where(g, _round(float(t0[0]) * clean + float(t0[1]) * n0, dtype), x)          # dd_given_views_noise
    for k, t in enumerate(timesteps):
        e = _guided(model(x.reshape(b * n, *x.shape[2:]), int(t)), guidance, dtype).reshape(x.shape)
        if mode == 2:
            e = torch.where(g, n0, e)
        r = _round(sch.step(e, int(t), x), dtype)
        row = gcoef[k].tolist()
        if mode == 1 and row[2] != 0:
            r = torch.where(g, _round(row[0] * clean + row[1] * n0, dtype), r)
        x = r
    return x


def linear_model(seed, scale=0.3):
    """A toy eps model, linear in the latents with a per-half, per-timestep offset: eps_h = a_h x + s(t) z_h."""
    gen = torch.Generator().manual_seed(seed)
    a = (0.4, 0.7)

    def model(x, t):
        z = torch.randn((2,) + tuple(x.shape), generator=gen, dtype=torch.float64)
        s = scale * (1.0 + t / 1000.0)
        return torch.stack([a[0] * x + s * z[0], a[1] * x + s * z[1]])
    return model
