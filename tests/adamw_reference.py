"""The fused optimizer step (include/dualdiff_hip.h: dd_adamw_step) restated in numpy, in two forms:

  * the fp32 form, operation by operation as csrc/adamw_core.h states it (numpy's float32 array arithmetic is one IEEE
    operation per call: no fused multiply-add, division and square root correctly rounded), with the norm summed in the
    kernels' chunk order, so that it gives the kernels' bits;
  * the float64 form: the same formula with every scalar and every operation in float64 ("exact" beside fp32).

and `bounds`, the per-element bound on |fp32 form - float64 form| after one step from the same state, derived below from
the roundings of each line — not from what any kernel gives.  Shared by tests/test_adamw_cpu.py and tests/test_adamw_gpu.py.

The rule (torch/optim/adamw.py, _single_tensor_adamw with amsgrad=False, maximize=False, behind GradScaler's unscale and
torch.nn.utils.clip_grad_norm_):
    gu = g * inv_scale;  norm = sqrt(sum gu^2);  clip = min(max_norm / (norm + 1e-6), 1);  gc = gu * clip
    p *= 1 - lr wd;  m += (1 - beta1)(gc - m);  v = v beta2 + (1 - beta2) gc gc
    p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
"""
import math

import numpy as np

U = 2.0 ** -24                    # unit roundoff of fp32
ETA = 2.0 ** -149                 # the smallest fp32 subnormal: the absolute error of an operation that underflows
THREADS, WAVE = 256, 64

DEFAULTS = dict(lr=8e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=1.0)   # configs/runner/default.yaml
LOUD = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.1, max_grad_norm=1.0)
HYPERS = {"defaults": DEFAULTS, "loud": LOUD}
FAULTS = ("no_bias_correction", "coupled_decay", "eps_in_sqrt", "unclamped", "beta1_weight", "skip_counts", "tail_untouched")


# ---- the fixture -------------------------------------------------------------------------------------------------------

def numels(chunk):
    """the eleven rows of the issue's table: the last but one is empty, the last has no gradient"""
    return [1, 3, 255, 256, 257, chunk - 1, chunk, chunk + 1, 3 * chunk + 5, 0, 37]


def fixture(chunk, seed=0):
    """-> (state, [grads of step 1..4]): fp32 rows; gradients alternate between a set of norm 200 (the clip bites) and
    one of norm 0.5 (the coefficient clamps to 1); the last row's gradient is None."""
    rng = np.random.default_rng(seed)
    ns = numels(chunk)
    state = new_state([rng.normal(0.0, 0.05, n).astype(np.float32) for n in ns])
    grads = []
    for k in range(4):
        g = [rng.normal(0.0, 1.0, n) for n in ns[:-1]]
        norm = math.sqrt(sum(float((x * x).sum()) for x in g))
        target = 200.0 if k % 2 == 0 else 0.5
        grads.append([(x * (target / norm)).astype(np.float32) for x in g] + [None])
    return state, grads


def new_state(p, step=0, betas=(0.9, 0.999)):
    return dict(p=[x.copy() for x in p], m=[np.zeros_like(x) for x in p], v=[np.zeros_like(x) for x in p], step=step,
                b1p=betas[0] ** step, b2p=betas[1] ** step, skipped=0, found_inf=0)


def copy_state(s):
    return dict(s, p=[x.copy() for x in s["p"]], m=[x.copy() for x in s["m"]], v=[x.copy() for x in s["v"]])


# ---- the norm ----------------------------------------------------------------------------------------------------------

def inv_scale_of(grad_scale):
    """GradScaler: scale.double().reciprocal().float()"""
    return np.float32(1.0) if grad_scale is None else np.float32(1.0 / float(np.float32(grad_scale)))


def _group_sum(lanes):
    """256 float64 lane sums -> the workgroup's sum: the butterfly of each wave, then waves 0..3 in order"""
    w = lanes.reshape(THREADS // WAVE, WAVE).copy()
    idx = np.arange(WAVE)
    o = WAVE // 2
    while o:
        w = w + w[:, idx ^ o]
        o //= 2
    out = w[0, 0]
    for k in range(1, THREADS // WAVE):
        out = out + w[k, 0]
    return out


def sumsq_kernel_order(grads, inv_scale, chunk, sizes=None):
    """The float64 sum of fl32(g * inv_scale)^2 in the kernels' order, bit for bit: per chunk, lane l sums elements
    4 (256 i + l) + c in rising i, c; the group sum; then the partials, lane l summing partials l + 256 i.
    sizes: the rows' element counts, needed where a gradient is None (its chunks hold a zero partial each, which moves
    the later partials to other lanes).  -> (sum, a non-finite value was seen)"""
    partials, bad = [], False
    with np.errstate(all="ignore"):
        for i, g in enumerate(grads):
            if g is None:
                partials += [np.float64(0.0)] * ((sizes[i] + chunk - 1) // chunk)
                continue
            gu = (g.astype(np.float32) * np.float32(inv_scale)).astype(np.float32)
            bad = bad or not bool(np.isfinite(gu).all())
            for at in range(0, g.size, chunk):
                x = np.zeros(chunk, np.float64)
                part = gu[at:at + chunk].astype(np.float64)
                x[:part.size] = part * part
                x = x.reshape(chunk // (4 * THREADS), THREADS, 4)
                lanes = np.zeros(THREADS, np.float64)
                for k in range(x.shape[0]):
                    for c in range(4):
                        lanes = lanes + x[k, :, c]
                partials.append(_group_sum(lanes))
        n = len(partials)
        padded = np.zeros((n + THREADS - 1) // THREADS * THREADS if n else THREADS, np.float64)
        padded[:n] = partials
        lanes = np.zeros(THREADS, np.float64)
        for row in padded.reshape(-1, THREADS):
            lanes = lanes + row
        return _group_sum(lanes), bad


def sumsq_exact(grads, inv_scale):
    """the same sum with no rounding but the last (math.fsum over exact float64 squares)"""
    with np.errstate(all="ignore"):
        sq = [((g.astype(np.float32) * np.float32(inv_scale)).astype(np.float64)) ** 2 for g in grads if g is not None]
    flat = np.concatenate(sq) if sq else np.zeros(0)
    return math.fsum(flat.tolist()) if np.isfinite(flat).all() else float("nan")


# ---- the scalars -------------------------------------------------------------------------------------------------------

def scalars64(sumsq, b1p, b2p, lr, hyper, unclamped=False, no_bias_correction=False, beta1_weight=False):
    """the step's scalars in float64, from the sum of squares, the ADVANCED beta products and the fp32 table entry lr"""
    beta1, beta2 = hyper["betas"]
    norm = math.sqrt(sumsq)
    clip = 1.0
    if hyper.get("max_grad_norm") is not None:
        clip = hyper["max_grad_norm"] / (norm + 1e-6)
        if not unclamped and not clip < 1.0:
            clip = 1.0
    lr = float(np.float32(lr))
    return dict(grad_norm=norm, clip_coef=clip, lr=lr, decay=1.0 - lr * hyper["weight_decay"],
                w1=beta1 if beta1_weight else 1.0 - beta1, b2=beta2, w2=1.0 - beta2,
                step_size=lr if no_bias_correction else lr / (1.0 - b1p),
                bc2_sqrt=1.0 if no_bias_correction else math.sqrt(1.0 - b2p), eps=hyper["eps"])


def scalars32(s64):
    """each rounded to fp32 once"""
    return {k: np.float32(v) for k, v in s64.items()}


SCALAR_NAMES = ("clip_coef", "decay", "w1", "b2", "w2", "step_size", "bc2_sqrt", "eps")


# ---- the update --------------------------------------------------------------------------------------------------------

def update32(p, g, m, v, s, inv_scale, coupled_decay=None, eps_in_sqrt=False):
    """one row, the fp32 form: every line one float32 operation.  s: fp32 scalars.  -> (p, m, v)"""
    f = np.float32
    with np.errstate(all="ignore"):
        gc = (g * f(inv_scale)) * s["clip_coef"]
        if coupled_decay is not None:                     # planted fault: weight decay added to the gradient (Adam's L2)
            gc = gc + f(coupled_decay) * p
            pd = p
        else:
            pd = p * s["decay"]
        mn = m + s["w1"] * (gc - m)
        vn = v * s["b2"] + (s["w2"] * gc) * gc
        if eps_in_sqrt:                                   # planted fault
            den = np.sqrt(vn + s["eps"]) / s["bc2_sqrt"]
        else:
            den = np.sqrt(vn) / s["bc2_sqrt"] + s["eps"]
        pn = pd - s["step_size"] * (mn / den)
    assert pn.dtype == mn.dtype == vn.dtype == np.float32
    return pn, mn, vn


def update64(p, g, m, v, s, inv_scale):
    """one row, the float64 form.  s: float64 scalars"""
    p, g, m, v = (x.astype(np.float64) for x in (p, g, m, v))
    with np.errstate(all="ignore"):
        gc = g * float(inv_scale) * s["clip_coef"]
        pd = p * s["decay"]
        mn = m + s["w1"] * (gc - m)
        vn = v * s["b2"] + s["w2"] * gc * gc
        den = np.sqrt(vn) / s["bc2_sqrt"] + s["eps"]
        pn = pd - s["step_size"] * (mn / den)
    return pn, mn, vn


def shadow_bits(p, dtype):
    """fp32 -> the uint16 bits of the nearest fp16 / bf16, ties to even"""
    if dtype == "fp16":
        with np.errstate(over="ignore"):
            return p.astype(np.float16).view(np.uint16)
    u = p.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(p), np.uint16(0x7FC0), r)


def step(state, grads, hyper, lr_table, form="fp32", chunk=8192, grad_scale=None, found_inf_in=False, scalars=None, fault=None):
    """One whole step from `state` -> (new state, scalars used).  form "fp32": the kernels' arithmetic (the norm in chunk
    order, the scalars rounded to fp32 — or `scalars`, fp32 values read from a device, in their place); form "float64": the
    exact one (the norm by math.fsum, float64 scalars).  fault: one of FAULTS, planted into the fp32 form."""
    assert fault is None or (fault in FAULTS and form == "fp32")
    inv = inv_scale_of(grad_scale)
    if form == "fp32":
        sumsq, bad = sumsq_kernel_order(grads, inv, chunk, [x.size for x in state["p"]])
    else:
        sumsq = sumsq_exact(grads, inv)
        bad = not math.isfinite(sumsq)
    new = copy_state(state)
    beta1, beta2 = hyper["betas"]
    if bad or found_inf_in:
        new["found_inf"], new["skipped"] = 1, state["skipped"] + 1
        if fault == "skip_counts":
            new["step"], new["b1p"], new["b2p"] = state["step"] + 1, state["b1p"] * beta1, state["b2p"] * beta2
        return new, None
    new["found_inf"] = 0
    new["step"], new["b1p"], new["b2p"] = state["step"] + 1, state["b1p"] * beta1, state["b2p"] * beta2
    lr = lr_table[min(new["step"] - 1, len(lr_table) - 1)]
    s = scalars64(sumsq, new["b1p"], new["b2p"], lr, hyper, unclamped=fault == "unclamped",
                  no_bias_correction=fault == "no_bias_correction", beta1_weight=fault == "beta1_weight")
    if form == "fp32":
        s = scalars32(s)
        if scalars is not None:
            s.update({k: np.float32(scalars[k]) for k in SCALAR_NAMES})
    for i, g in enumerate(grads):
        if g is None:
            continue
        if form == "fp32":
            pn, mn, vn = update32(state["p"][i], g, state["m"][i], state["v"][i], s, inv,
                                  coupled_decay=hyper["weight_decay"] if fault == "coupled_decay" else None,
                                  eps_in_sqrt=fault == "eps_in_sqrt")
            if fault == "tail_untouched":
                full = g.size - g.size % 4
                pn[full:], mn[full:], vn[full:] = state["p"][i][full:], state["m"][i][full:], state["v"][i][full:]
        else:
            pn, mn, vn = update64(state["p"][i], g, state["m"][i], state["v"][i], s, inv)
        new["p"][i], new["m"][i], new["v"][i] = pn, mn, vn
    return new, s


# ---- the bounds --------------------------------------------------------------------------------------------------------

def bounds(state_row, g, scalars, inv_scale=1.0, clip_rel=U):
    """Per-element bounds (Em, Ev, Ep) on |fp32 form - float64 form| of m, v and p after ONE step of one row from the same
    fp32 state (p, m, v) and gradient g.  scalars: the float64 scalars (scalars64); the fp32 form uses each rounded to
    fp32, i.e. within a relative U = 2^-24 of it — clip_coef within clip_rel, which also carries the error of the norm
    under it (scalar_bounds).

    Derivation.  Every fp32 operation returns x (1 + d) with |d| <= U, or x + e with |e| <= ETA where the result is
    subnormal; a scalar rounded to fp32 is s (1 + d).  Write E(x) for the bound on the absolute error of the computed x,
    and r2 = (1 + U)^2 - 1 for "a rounded scalar times a value, rounded".
      gu = fl(g inv):              inv is the same fp32 number in both forms; one rounding.
      gc = fl(gu clip~):           relative error e_g = (1 + U)^2 (1 + clip_rel) - 1;      E(gc) = |gc| e_g + ETA
      d  = fl(gc - m):             E(d)  = E(gc) + U (|gc - m| + E(gc)) + ETA              (m is exact: the shared state)
      t  = fl(w1~ d):              E(t)  = w1 (E(d) + (|gc - m| + E(d)) r2) + ETA
      m' = fl(m + t):              E(m') = E(t) + U (|m'| + E(t)) + ETA
      a  = fl(v b2~):              E(a)  = v b2 r2 + ETA
      b  = fl(fl(w2~ gc) gc):      relative e_b = (1 + U)^3 (1 + e_g)^2 - 1;               E(b) = w2 gc^2 e_b + 2 ETA (1 + |gc|)
      v' = fl(a + b):              E(v') = E(a) + E(b) + U (v' + E(a) + E(b)) + ETA        (both terms >= 0: no cancellation)
      s  = fl(sqrt(v')):           |sqrt(x) - sqrt(y)| <= |x - y| / sqrt(y) for y > 0 (and <= sqrt(|x - y|) always):
                                   E0 = min(E(v') / sqrt(v'), sqrt(E(v')));  E(s) = E0 + U (sqrt(v') + E0)
      q  = fl(s / bc~):            r3 = (1 + U) / (1 - U) - 1;  E(q) = (E(s) + (sqrt(v') + E(s)) r3) / bc + ETA
      den = fl(q + eps~):          E(den) = E(q) + U eps + U (den + E(q) + U eps) + ETA
      r  = fl(m' / den):           the quotient's conditioning: |m~/den~ - m'/den| <= (E(m') + |r| E(den)) / (den - E(den)),
                                   =: E1 (den >= eps > E(den));  E(r) = E1 + U (|r| + E1) + ETA
      k  = fl(step_size~ r):       E(k)  = step_size (E(r) + (|r| + E(r)) r2) + ETA
      pd = fl(p decay~):           E(pd) = |p decay| r2 + ETA
      p' = fl(pd - k):             E(p') = E(pd) + E(k) + U (|p'| + E(pd) + E(k)) + ETA
    The bound on p is therefore about 3 U |p| — an fp32 parameter cannot hold less — plus the step's own error."""
    p, m, v = (state_row[k].astype(np.float64) for k in ("p", "m", "v"))
    s = scalars
    r2 = (1.0 + U) ** 2 - 1.0
    r3 = (1.0 + U) / (1.0 - U) - 1.0
    with np.errstate(all="ignore"):
        gc = g.astype(np.float64) * float(inv_scale) * s["clip_coef"]
        e_g = (1.0 + U) ** 2 * (1.0 + clip_rel) - 1.0
        Eg = np.abs(gc) * e_g + ETA
        D = np.abs(gc - m)
        Ed = Eg + U * (D + Eg) + ETA
        Et = s["w1"] * (Ed + (D + Ed) * r2) + ETA
        mn = m + s["w1"] * (gc - m)
        Em = Et + U * (np.abs(mn) + Et) + ETA
        Ea = v * s["b2"] * r2 + ETA
        e_b = (1.0 + U) ** 3 * (1.0 + e_g) ** 2 - 1.0
        Eb = s["w2"] * gc * gc * e_b + 2.0 * ETA * (1.0 + np.abs(gc))
        vn = v * s["b2"] + s["w2"] * gc * gc
        Ev = Ea + Eb + U * (vn + Ea + Eb) + ETA
        root = np.sqrt(vn)
        E0 = np.minimum(np.where(root > 0.0, Ev / np.where(root > 0.0, root, 1.0), np.inf), np.sqrt(Ev))
        Es = E0 + U * (root + E0)
        Eq = (Es + (root + Es) * r3) / s["bc2_sqrt"] + ETA
        den = root / s["bc2_sqrt"] + s["eps"]
        Eden = Eq + U * s["eps"] + U * (den + Eq + U * s["eps"]) + ETA
        r = mn / den
        E1 = (Em + np.abs(r) * Eden) / (den - Eden)
        Er = E1 + U * (np.abs(r) + E1) + ETA
        Ek = s["step_size"] * (Er + (np.abs(r) + Er) * r2) + ETA
        pd = p * s["decay"]
        Epd = np.abs(pd) * r2 + ETA
        pn = pd - s["step_size"] * r
        Ep = Epd + Ek + U * (np.abs(pn) + Epd + Ek) + ETA
    return Em, Ev, Ep


def scalar_bounds(n, norm, clip, max_grad_norm):
    """Bounds on |device value - float64 value| of grad_norm and clip_coef, and the relative bound on clip_coef that
    `bounds` takes as clip_rel.  The device sums n exact float64 squares in some fixed order: relative error below
    (n - 1) 2^-53 (1 + ...) for non-negative terms, taken as n 2^-52; the square root halves it and adds 2^-53; + 1e-6, the
    division and the comparison add two more; then ONE fp32 rounding each (relative U).  The reference value itself
    (math.fsum, math.sqrt) is within 2^-52 of the truth."""
    rel64 = (n + 8) * 2.0 ** -52
    rel = U + rel64 * (1.0 + U)
    return norm * rel, (clip * rel if max_grad_norm is not None else 0.0), rel


def worst_ratio(got, want, bound):
    """max |got - want| / bound over one row (0 for an empty row); a NaN anywhere counts as infinite"""
    if got.size == 0:
        return 0.0
    with np.errstate(all="ignore"):
        r = np.abs(got.astype(np.float64) - want) / bound
    return float("inf") if not np.isfinite(r).all() else float(r.max())
