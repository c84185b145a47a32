"""Building blocks of the denoising UNet / ControlNet on the HIP C-ABI (NHWC, fused epilogues).

The classes carry the *parameter names and constructor arguments* of the diffusers-0.17.1
modules the reference instantiates (so diffusers-layout checkpoints load with
`load_state_dict`), but the arithmetic is dispatched to the gfx950
kernels in libdualdiff_hip.so through `dualdiff_amd.ops` — there is no torch.nn.functional
compute on this path and no CPU fallback.

Activations travel as token-major 2-D tensors (m*h*w, c) plus the (m, h, w) triple; NCHW exists
only at the 4-channel latent boundary and when a caller hands in NCHW residuals.
"""
import math
import os

import torch
import torch.nn as nn

from .. import ops as O
from .. import upfold
from .._consts import device_const


# ----------------------------------------------------------------------------- helpers ----
# Bumped whenever ANY module drops its packed weights (.to() / load_state_dict / device_init_, also on a sub-module
# alone): HIP graphs captured behind the public forward() surfaces (model_base.ForwardGraphs) hold raw pointers to
# the packed copies and are re-captured when the epoch they were recorded in is over.
CACHE_EPOCH = [0]


class _Cached(nn.Module):
    """Module with lazily derived kernel-layout weights (`derived`); its entries drop on .to()/load_state_dict."""

    def _drop_cache(self):
        CACHE_EPOCH[0] += 1
        for k in [k for k in self.__dict__ if k.startswith("_pk_")]:
            del self.__dict__[k]

    def _apply(self, fn, *a, **k):
        self._drop_cache()
        return super()._apply(fn, *a, **k)

    def _load_from_state_dict(self, *a, **k):
        self._drop_cache()
        return super()._load_from_state_dict(*a, **k)


def _weight(mod, name=None):
    """mod.weight, or mod.<name>.weight: the parameter itself, not through nn.Module.__getattr__ (1 us a look, and the
    eager forward asks several hundred times)."""
    return (mod if name is None else mod._modules[name])._parameters["weight"]


def _capturing():
    try:
        return torch.cuda.is_current_stream_capturing()
    except RuntimeError:               # a build of torch with GPU support on a machine without one (CPU modules)
        return False


def derived(holder, name, params, build, slot=None):
    """holder.__dict__["_pk_" + name] (per `slot` where one name holds several entries): the value build() returns,
    cached against the address and version of every tensor in `params` (None entries allowed).  THE rule for every
    kernel-layout copy of a parameter: an in-place update or a new storage rebuilds it at the next eager call; inside a
    stream capture a stale entry is kept as it is (every caller warms up eagerly before it captures: a rebuild would
    record the packing kernels into the graph and redo them on every replay) and only a missing one is built.
    `_Cached._drop_cache` of the holder forgets it.  Recorded graphs do not follow: see CACHE_EPOCH."""
    try:
        key = [t if t is None else (t.data_ptr(), t._version) for t in params]
    except RuntimeError:               # inference tensors do not count versions
        key = [t if t is None else (t.data_ptr(), 0 if t.is_inference() else t._version) for t in params]
    entries, k = holder.__dict__, "_pk_" + name
    if slot is not None:
        entries, k = entries.setdefault(k, {}), slot
    hit = entries.get(k)
    if hit is None or (hit[0] != key and not _capturing()):
        with torch.no_grad():
            hit = entries[k] = (key, build())
    return hit[1]


# ---- context length in device memory (round 6) ----------------------------------------------------------------
# The context a cross-attention reads is [camera token | 77 text tokens | N_box box tokens] per view-instance
# (unet_addon_rawbox.py:337-361,1065-1068), and N_box changes from sample to sample: the reference's collate function pads
# the boxes of a batch to that batch's maximum (dataset/utils.py:165-244) and the pipeline forwards that length
# (pipeline_bev_controlnet.py:349-375).  The public forward()s therefore lay the context out at a CAPACITY — the box
# count rounded up to CTX_BUCKET — and hand the real length to the attention kernels through one int32 in device memory
# (dd_attn_desc.lk_dev), so that ONE recorded HIP graph per capacity serves every length (model_base.ForwardGraphs).
# Keys past the real length are never read: they are not "masked null boxes" (null box tokens DO attend in the
# reference, unet_addon_rawbox.py:852-896), they do not exist.
CTX_BASE = 78          # camera token + the 77 CLIP text tokens: the box-free context of every DualDiff config
CTX_BUCKET = 32        # box-token capacities are multiples of this


def box_capacity(n_box):
    """Capacity (in box tokens) of the bucket that holds `n_box` boxes: 0 -> 32, 1..32 -> 32, 33..64 -> 64, ..."""
    return max(CTX_BUCKET, -(-int(n_box) // CTX_BUCKET) * CTX_BUCKET)


def ctx_capacity(lc):
    """Context capacity for a context of `lc` tokens handed to the UNet: contexts shorter than CTX_BASE (plain SD use:
    text only) keep their exact length, longer ones are [CTX_BASE | boxes] and get the box bucket's capacity."""
    return int(lc) if lc < CTX_BASE else CTX_BASE + box_capacity(lc - CTX_BASE)


_CTX_KEYS = __import__("threading").local()


class context_keys:
    """`with context_keys(ctx, capacity, lk_dev):` — inside, every cross-attention whose context lies in `ctx`'s memory
    and is `capacity` tokens long reads only the first lk_dev[0] of them (Attention.run_cross).  Matched by address
    range, not identity: the processor protocol reshapes and SPLIT_SIZE chunks the context on its way down."""

    def __init__(self, ctx, capacity, lk_dev):
        self.new = None if lk_dev is None else (ctx.data_ptr(), ctx.data_ptr() + ctx.numel() * ctx.element_size(),
                                                int(capacity), lk_dev)

    def __enter__(self):
        self.old = getattr(_CTX_KEYS, "cur", None)
        _CTX_KEYS.cur = self.new
        return self

    def __exit__(self, *exc):
        _CTX_KEYS.cur = self.old
        return False


def lk_dev_for(ctx2d, lk):
    cur = getattr(_CTX_KEYS, "cur", None)
    if cur is None or lk != cur[2] or not (cur[0] <= ctx2d.data_ptr() < cur[1]):
        return None
    return cur[3]


def lk_const(value, device):
    """int32 device tensor [1] holding `value` — a device constant (_consts.device_const: one per device and value,
    first asked for outside any capture; a forward graph copies it into its own static word, an eager call reads it in
    place)."""
    value = int(value)
    return device_const(("lk", value), device, lambda: torch.tensor([value], dtype=torch.int32))


def _pad_cols(w, mult=8):
    k = w.shape[1]
    kp = (k + mult - 1) // mult * mult
    if kp == k:
        return w.contiguous()
    out = w.new_zeros((w.shape[0], kp))
    out[:, :k] = w
    return out


def to_nhwc(x):
    """(m, c, h, w) tensor -> ((m*h*w, c) view/copy, m, h, w); zero-copy for channels_last."""
    m, c, h, w = x.shape
    p = x.permute(0, 2, 3, 1)
    if not p.is_contiguous():
        if not x.is_cuda or x.dtype not in (torch.float16, torch.bfloat16):
            p = p.contiguous()
        else:                # LDS-tiled layout kernel (torch's strided copy moves the 320-channel ORS-3D condition at 0.3 TB/s)
            return O.nchw_to_nhwc(x), m, h, w
    return p.reshape(m * h * w, c), m, h, w


def as_nchw_view(x2d, m, h, w):
    """Zero-copy logical-NCHW (channels_last strides) view of an NHWC activation."""
    return x2d.view(m, h, w, x2d.shape[1]).permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------ linear ----
class Linear(_Cached):
    """nn.Linear / 1x1 nn.Conv2d.  `conv` only changes the stored weight shape ([n,k,1,1])."""

    def __init__(self, in_features, out_features, bias=True, conv=False):
        super().__init__()
        self.in_features, self.out_features, self.conv = in_features, out_features, conv
        shape = (out_features, in_features, 1, 1) if conv else (out_features, in_features)
        self.weight = nn.Parameter(torch.empty(shape))
        self.bias = nn.Parameter(torch.empty(out_features)) if bias else None

    @property
    def w2d(self):
        """(out, K padded to a multiple of 8); a view of the live parameter where nothing is padded."""
        w = _weight(self)
        return derived(self, "w", [w], lambda: _pad_cols(w.detach().reshape(self.out_features, -1)))

    @property
    def wx(self):
        """The (320, 320) weight in the layout dd_xattn320 streams (ops.xattn_pack_weight), packed lazily like w2d and
        owned by this module."""
        return derived(self, "wx", [_weight(self)], lambda: O.xattn_pack_weight(self.w2d))

    fp8_mfma = False   # extension (BASELINE configs[4]): W8A8 on the fp8 matrix path (dd_gemm8) where it pays: K >= 640, wide output

    @property
    def w8p(self):
        """(float8_e4m3fn [n, K padded to 128], fp32 scale [n]): the W8 operand of ops.gemm8, packed lazily."""
        return derived(self, "w8p", [_weight(self)], lambda: O.quantize_fp8_padded(self.w2d))

    def run(self, x2d, ln_next=None, **kw):
        """x2d: (rows, K) — fused-epilogue GEMM (see ops.gemm kwargs).  ln_next: the LayerNorm module that will
        read the result next; where the 80x320 tile applies (out_features == 320) the epilogue emits its output
        too and `ln_next.run(result)` becomes a cache hit (no launch)."""
        if ln_next is not None and ln_producer_ok(self, ln_next, kw):
            w = self.w2d
            out = O.gemm(x2d, w, self.bias, ln_out=(ln_next.weight, ln_next.bias, ln_next.eps), **kw)
            out._ln_cache = (ln_next, out._ln_out)
            return out
        w = self.w2d
        if w.shape[1] != self.in_features:   # K padded to a multiple of 8 (e.g. cam2token 189 -> 192)
            x2d = torch.nn.functional.pad(x2d, (0, w.shape[1] - x2d.shape[1]))
        return O.gemm(x2d, w, self.bias, **kw)

    def run_ln(self, x2d, norm, **kw):
        """LayerNorm(norm) + this Linear: the algebraic fold when enabled, else two launches.  (The row-panel GEMM with
        the LayerNorm as its prologue — round 2, 9 % slower on the step — went with its family in round 5.)"""
        if self.fp8_mfma and fp8_mfma_ok(norm, self.in_features, self.out_features, x2d) \
                and set(kw) <= {"epilogue"} and kw.get("epilogue", O.DD_EPI_NONE) in (O.DD_EPI_NONE, O.DD_EPI_GEGLU):
            # the LayerNorm launch quantises its output rows to e4m3; the projection runs on the fp8 matrix path
            a8, sa = O.rowquant_fp8(x2d, (norm.weight, norm.bias, norm.eps))
            w8, sw = self.w8p
            return O.gemm8(a8, sa, w8, sw, self.bias, dtype=x2d.dtype, geglu=kw.get("epilogue") == O.DD_EPI_GEGLU)
        if not ln_fold_ok(norm, self.in_features, self.out_features, x2d):
            return self.run(norm.run(x2d), **kw)
        w, ln = fold_layernorm(self, "ln", norm, [self.weight], [self.bias])
        return O.gemm(x2d, w, None, ln=ln, **kw)

    def forward(self, x):
        """Tensor-in / tensor-out form used by foreign attention processors:
        (..., K) tokens, or (m, K, h, w) NCHW for the 1x1-conv flavour."""
        if self.conv and x.dim() == 4:
            x2d, m, h, w = to_nhwc(x)
            return as_nchw_view(self.run(x2d), m, h, w)
        lead = x.shape[:-1]
        y = self.run(x.reshape(-1, x.shape[-1]) if x.is_contiguous() else x.contiguous().reshape(-1, x.shape[-1]))
        return y.reshape(*lead, self.out_features)


class Conv3x3(_Cached):
    """nn.Conv2d(k=3, padding=1, stride) as implicit GEMM; weight kept in torch layout
    [cout, cin, 3, 3] for checkpoints, packed to [cout][ky][kx][cin_pad] for the kernel."""

    def __init__(self, in_channels, out_channels, stride=1):
        super().__init__()
        self.in_channels, self.out_channels, self.stride = in_channels, out_channels, stride
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, 3, 3))
        self.bias = nn.Parameter(torch.empty(out_channels))

    @property
    def cin_pad(self):
        return (self.in_channels + 7) // 8 * 8

    @property
    def packed(self):
        def build():
            w = _weight(self).detach().permute(0, 2, 3, 1)            # [cout, 3, 3, cin]
            if self.cin_pad != self.in_channels:
                wp = w.new_zeros((self.out_channels, 3, 3, self.cin_pad))
                wp[..., :self.in_channels] = w
                w = wp
            return w.reshape(self.out_channels, 9 * self.cin_pad).contiguous()
        return derived(self, "w", [_weight(self)], build)

    # Nearest upsample + conv: the three taps of an axis read at most two source pixels, so the tap slices that read the
    # same pixel are summed ahead of time (fp32, rounded once) and the launch is a 2 x 2-tap conv with K = 4 Cin instead
    # of 9 Cin (upfold.py; dd_gemm2u_kernel).  The layer folds only where the tracked table
    # (tuned/gfx950_upfold.json) records the folded launch as measured faster than the 9-tap one for this very shape:
    # many classes over few rows lose (each class streams its own weight matrix).  DD_UPFOLD=0 turns it off.
    fold_upsample = os.environ.get("DD_UPFOLD", "1") != "0"

    def folded_up(self, h, w, up_size, m=None):
        """The weights folded for the nearest map (h, w) -> up_size, or None where the 9-tap form is kept: a map the fold
        does not cover, or (m given: the model's path) a shape without a winning row in the tracked table."""
        if not self.fold_upsample or up_size is None:
            return None
        size = (h, w, int(up_size[0]), int(up_size[1]))
        if m is not None:
            row = O.tuning.upfold_tuned(O.tuning.conv_upfold_key(m, h, w, self.cin_pad, self.out_channels, size[2], size[3],
                                                                O._dtype_code(self.weight.dtype)))
            if row is None or row[0] == 0:
                return None
        if not upfold.ok(*size, self.cin_pad, self.stride):
            return None
        return derived(self, "upfold", [_weight(self)], lambda: upfold.fold_weight(self.packed, *size), slot=size)

    def run(self, x2d, m, h, w, up_size=None, **kw):
        """kw gn_next = (GroupNorm module, silu, want_x): see ops.conv3x3 (split-K reduce folded into that norm)."""
        return O.conv3x3(x2d, self.packed, self.bias, m, h, w, stride=self.stride, up_size=up_size,
                         upfold=self.folded_up(h, w, up_size, m), **kw)

    def out_hw(self, h, w, up_size=None):
        hv, wv = (h, w) if up_size is None else up_size
        return (hv - 1) // self.stride + 1, (wv - 1) // self.stride + 1

    def forward(self, x):
        x2d, m, h, w = to_nhwc(x)
        if x2d.shape[1] != self.cin_pad:
            x2d = torch.nn.functional.pad(x2d, (0, self.cin_pad - x2d.shape[1]))
        ho, wo = self.out_hw(h, w)
        return as_nchw_view(self.run(x2d, m, h, w), m, ho, wo)


class GroupNorm(nn.Module):
    def __init__(self, num_groups, num_channels, eps=1e-5):
        super().__init__()
        self.num_groups, self.num_channels, self.eps = num_groups, num_channels, eps
        self.weight = nn.Parameter(torch.empty(num_channels))
        self.bias = nn.Parameter(torch.empty(num_channels))

    def run(self, x2d, m, hw, silu, x2=None):
        hit = getattr(x2d, "_gn_cache", None)          # already computed by the producing conv's fused reduce + norm
        if hit is not None:
            del x2d._gn_cache                          # consumed once (see LayerNorm.run)
            if hit[0] is self and hit[1] == bool(silu) and x2 is None:
                return hit[2]
        if getattr(x2d, "_unwritten", False):
            raise RuntimeError("this conv output was folded into its GroupNorm and never written")
        return O.groupnorm(x2d, self.weight, self.bias, m, hw, self.num_groups, self.eps, silu, x2=x2)


class LayerNorm(nn.Module):
    def __init__(self, dim, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.empty(dim))
        self.bias = nn.Parameter(torch.empty(dim))

    def run(self, x2d):
        hit = getattr(x2d, "_ln_cache", None)          # LayerNorm already emitted by the producer's epilogue
        if hit is not None:
            # consumed ONCE: the kernels write through data_ptr (out=, accumulate), so tensor._version cannot
            # tell whether x2d was rewritten later — a second LayerNorm of the same Python tensor recomputes
            del x2d._ln_cache
            if hit[0] is self:
                return hit[1]
        return O.layernorm(x2d, self.weight, self.bias, self.eps)

    def forward(self, x):
        return self.run(x.reshape(-1, x.shape[-1])).reshape(x.shape)


# LayerNorm fold policy (dd_gemm's ln_colsum path).  Every column tile of the consumer GEMM recomputes
# the statistics of its rows, and that costs more than the LayerNorm launch it removes: measured on
# config 2, folding all four norms (QKV is 3C wide, the GEGLU projection 8C) LOSES 5 % (72.8 -> 68.9
# steps/s), folding only the C-wide to_q of attn2 is neutral (73.1 vs 73.1-75).  Off by default;
# DD_LN_FOLD=all / q turn it on.
#
# DD_LN_FOLD=stats: fold wherever the producer of the input left its row statistics behind
# (`O.gemm(..., ln_stats=True)`: proj_in and the to_out + residual GEMMs have every output value in
# registers), so that the consumer reads k/32 partial sums per row instead of the rows themselves and the
# LayerNorm launch disappears.  Measured on config 2: 81.1-81.3 vs 82.0 steps/s with the fold off — the
# extra epilogue work of the wide consumers (QKV 3C, GEGLU 8C: two FMAs and two table loads per output
# value) and the producers' shuffles cost more than 106 small LayerNorm launches that mostly overlap
# with other streams.  Kept behind the switch, with kernel tests.
LN_FOLD = __import__("os").environ.get("DD_LN_FOLD", "0")


def ln_fold_ok(norm, k, n=None, x=None):
    """The kernel-side fold covers the transformer widths of this network."""
    if LN_FOLD == "0" or not isinstance(norm, LayerNorm) or k not in (320, 640, 1280):
        return False
    if LN_FOLD == "stats":
        return x is not None and getattr(x, "_ln_stats", None) is not None
    return LN_FOLD == "all" or (n is not None and n <= k)


def want_ln_stats():
    return LN_FOLD == "stats"


# LayerNorm emitted by the PRODUCER's epilogue (dd_gemm_desc.ln_out): the GEMM that writes the residual stream at
# the 320-channel level runs on a tile owning whole rows (80 x 320) and writes LayerNorm(out) next to out, so the
# next sub-layer's norm needs no launch and does not re-read the stream.  DD_LN_PRODUCER=0 turns it off.
LN_PRODUCER = __import__("os").environ.get("DD_LN_PRODUCER", "1") != "0"


def ln_producer_ok(lin, norm, kw):
    if not LN_PRODUCER or not isinstance(norm, LayerNorm) or lin.out_features != 320:
        return False
    if LN_FOLD != "0":                         # the consumer would fold the LayerNorm and ignore ln_out
        return False
    if lin.w2d.shape[1] % 64 or kw.get("a2") is not None and kw["a2"].shape[1] % 64:
        return False
    bad = ("ln", "ln_stats", "head_major", "out_f32", "accumulate", "rowvec", "out", "tile", "split_k")
    return not any(kw.get(k) for k in bad) and kw.get("epilogue", O.DD_EPI_NONE) == O.DD_EPI_NONE \
        and kw.get("alpha", 1.0) == 1.0


def fp8_mfma_ok(norm, k, n, x2d):
    """Where the W8A8 projection beats LayerNorm + 16-bit GEMM on MI355X (tools/gemm8_bench.py): K = 640 / 1280 and an
    output at least 3 K wide (fused Q|K|V, the GEGLU projection); the C x C projections and the 320-channel level
    (K padded 320 -> 384, three K steps) do not gain and stay 16-bit."""
    return isinstance(norm, LayerNorm) and k in (640, 1280) and n >= 3 * k and x2d.is_contiguous() \
        and getattr(x2d, "_ln_cache", None) is None


# Fused cross-attention kernel of the 320-channel level (dd_xattn320: to_q -> SDPA over <= 128 context keys -> to_out +
# residual + next LayerNorm in one launch; SFA and attn2 of the 28x50 blocks).  DD_XATTN_FUSED=0: the three launches.
XATTN_FUSED = __import__("os").environ.get("DD_XATTN_FUSED", "1") != "0"


# Head-major Q / K / V planes + softmax scale folded into Q by the projection epilogue (dd_gemm_desc.
# out_headmajor_d, dd_attn_desc.q_prescaled).  DD_ATTN_HEAD_MAJOR=0 restores the fused row-major layout.
HEAD_MAJOR = __import__("os").environ.get("DD_ATTN_HEAD_MAJOR", "1") != "0"


def fold_layernorm(holder, name, norm, weights, biases):
    """LayerNorm(x) @ W^T + b  ==  rstd * (x @ W'^T - mean * colsum) + b'   with
    W' = W * gamma, colsum[n] = sum_k W'[n,k] (of the ROUNDED W', the matrix the kernel multiplies by),
    b' = W beta + b.  `weights` / `biases`: lists concatenated along N (fused projections).
    A `derived` entry `name` of `holder`.  Returns (W', (colsum, b', eps))."""
    def build():
        w = torch.cat([t.detach().reshape(t.shape[0], -1) for t in weights], dim=0).float()
        b = torch.cat([(bb.detach().float() if bb is not None else torch.zeros(t.shape[0], device=t.device))
                       for t, bb in zip(weights, biases)])
        wp = (w * norm.weight.detach().float()[None, :]).to(weights[0].dtype).contiguous()
        colsum = wp.float().sum(dim=1).contiguous()
        lnb = (w @ norm.bias.detach().float() + b).contiguous()
        return wp, (colsum, lnb, norm.eps)
    return derived(holder, name, [norm.weight, norm.bias] + list(weights) + list(biases), build)


class _Dropout(nn.Module):
    """Placeholder for nn.Dropout(p=0) so that `to_out.1` / `ff.net.1` indices exist."""

    def forward(self, x):
        return x


# --------------------------------------------------------------------------- embeddings ---
class Timesteps(nn.Module):
    def __init__(self, num_channels, flip_sin_to_cos, downscale_freq_shift):
        super().__init__()
        self.num_channels, self.flip_sin_to_cos = num_channels, flip_sin_to_cos
        self.downscale_freq_shift = downscale_freq_shift

    def run(self, t_f32, dtype):
        return O.timestep_embedding(t_f32, self.num_channels, dtype, self.flip_sin_to_cos,
                                    float(self.downscale_freq_shift))


class TimestepEmbedding(nn.Module):
    def __init__(self, in_channels, time_embed_dim):
        super().__init__()
        self.linear_1 = Linear(in_channels, time_embed_dim)
        self.linear_2 = Linear(time_embed_dim, time_embed_dim)

    def run(self, t_emb):
        return self.linear_2.run(self.linear_1.run(t_emb, epilogue=O.DD_EPI_SILU))


# ------------------------------------------------------------------------------- resnet ---
class ResnetBlock2D(nn.Module):
    """GN+SiLU -> conv3x3 (+bias +time-emb vector in the epilogue) -> GN+SiLU -> conv3x3
    (+bias +shortcut in the epilogue).  Input may be the channel-concat of two tensors
    (up path: [h, skip]) which is never materialised."""

    def __init__(self, in_channels, out_channels, temb_channels, groups=32, eps=1e-5):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.norm1 = GroupNorm(groups, in_channels, eps)
        self.conv1 = Conv3x3(in_channels, out_channels)
        self.time_emb_proj = Linear(temb_channels, out_channels)
        self.norm2 = GroupNorm(groups, out_channels, eps)
        self.conv2 = Conv3x3(out_channels, out_channels)
        self.conv_shortcut = Linear(in_channels, out_channels, conv=True) if in_channels != out_channels else None

    def run(self, x, m, h, w, temb_vec, x2=None, extra_res=None, gn_next=None):
        """x: (mhw, c1) [, x2: (mhw, c2)]; temb_vec: (m, cout) = time_emb_proj(SiLU(emb)) view.
        extra_res: optional second residual added to the output (ControlNet mid residual).
        gn_next: the single-source GroupNorm module that reads the block's output next (the Transformer2DModel input
        norm), so that a split-K conv2 can hand its reduction to it."""
        hw = h * w
        a = self.norm1.run(x, m, hw, True, x2=x2)
        hid = self.conv1.run(a, m, h, w, rowvec=temb_vec, gn_next=(self.norm2, True, False))
        a = self.norm2.run(hid, m, hw, True)
        if self.conv_shortcut is not None:
            sc = self.conv_shortcut.run(x, a2=x2, res=extra_res)
        elif extra_res is not None:
            sc = O.add(x, extra_res)
        else:
            sc = x
        return self.conv2.run(a, m, h, w, res=sc, gn_next=None if gn_next is None else (gn_next, False, True))


class Downsample2D(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.conv = Conv3x3(channels, channels, stride=2)


class Upsample2D(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.conv = Conv3x3(channels, channels)


# ---------------------------------------------------------------------------- attention ---
class HIPAttnProcessor:
    """Default attention processor: fused QKV / KV projection GEMMs + flash attention kernel +
    out-projection with the residual folded into its epilogue when the caller provides one.
    Same call protocol as diffusers processors (box_adapter.py:33-40)."""

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None, temb=None,
                 residual=None):
        if attention_mask is not None:
            raise NotImplementedError("attention_mask is None on the denoising path (blocks.py:166-187)")
        b, lq, c = hidden_states.shape
        x = hidden_states.reshape(b * lq, c)
        res2d = residual.reshape(b * lq, -1) if residual is not None else None
        if encoder_hidden_states is None:
            out = attn.run_self(x, b, lq, res=res2d)
        else:
            e = encoder_hidden_states
            out = attn.run_cross(x, b, lq, e.reshape(-1, e.shape[-1]), e.shape[1], res=res2d)
        return out.reshape(b, lq, -1)


class Attention(_Cached):
    """diffusers `Attention` surface (to_q/to_k/to_v/to_out, heads, scale, processor protocol)."""

    def __init__(self, query_dim, cross_attention_dim=None, heads=8, dim_head=64, bias=False):
        super().__init__()
        inner = heads * dim_head
        self.inner_dim, self.heads, self.dim_head = inner, heads, dim_head
        self.scale = dim_head ** -0.5
        self.is_cross = cross_attention_dim is not None
        self.norm_cross = None
        self.group_norm = None
        self.spatial_norm = None
        self.residual_connection = False
        self.rescale_output_factor = 1.0
        self.to_q = Linear(query_dim, inner, bias=bias)
        self.to_k = Linear(cross_attention_dim or query_dim, inner, bias=bias)
        self.to_v = Linear(cross_attention_dim or query_dim, inner, bias=bias)
        self.to_out = nn.ModuleList([Linear(inner, query_dim), _Dropout()])
        self.processor = HIPAttnProcessor()

    def set_processor(self, processor):
        if isinstance(getattr(self, "processor", None), nn.Module) and not isinstance(processor, nn.Module):
            self._modules.pop("processor")
        self.processor = processor
        CACHE_EPOCH[0] += 1          # forward graphs recorded with the old processor are over (model_base.ForwardGraphs)

    def prepare_attention_mask(self, attention_mask, target_length, batch_size=None, out_dim=3):
        if attention_mask is not None:
            raise NotImplementedError
        return None

    def head_to_batch_dim(self, t):
        b, l, c = t.shape
        return t.reshape(b, l, self.heads, c // self.heads).permute(0, 2, 1, 3).reshape(b * self.heads, l, -1)

    def batch_to_head_dim(self, t):
        bh, l, d = t.shape
        return t.reshape(bh // self.heads, self.heads, l, d).permute(0, 2, 1, 3).reshape(bh // self.heads, l, -1)

    def get_attention_scores(self, query, key, attention_mask=None):
        """diffusers `Attention.get_attention_scores`: softmax(scale * q k^T) on (batch*heads, L, d) tensors,
        fp32 softmax, probabilities back in the input dtype.  Part of the surface FOREIGN processors call
        (reference tools/unet_modify.py:30 keeps the probabilities for visualisation); plain torch on the
        caller's tensors — the built-in processors never come here, they run the flash kernel."""
        if attention_mask is not None:
            raise NotImplementedError("attention_mask is None on the denoising path")
        scores = torch.baddbmm(torch.empty((), dtype=query.dtype, device=query.device).expand(
            query.shape[0], query.shape[1], key.shape[1]), query, key.transpose(-1, -2), beta=0, alpha=self.scale)
        return scores.float().softmax(dim=-1).to(query.dtype)

    # fused weights ------------------------------------------------------------------------
    def _fused(self, names):
        ws = [_weight(self, n) for n in names]
        return derived(self, "".join(names), ws, lambda: torch.cat([w.detach() for w in ws], dim=0).contiguous())

    def _fused_bias(self, names):
        """Concatenated biases of the fused projection (None for the bias-free SD layers)."""
        mods = [getattr(self, n) for n in names]
        if all(m.bias is None for m in mods):
            return None
        return derived(self, "b_" + "".join(names), [m.bias for m in mods], lambda: torch.cat([
            m.bias.detach() if m.bias is not None else m.weight.new_zeros(m.out_features) for m in mods]).contiguous())

    fp8_mfma = False   # extension: fused Q|K|V projection as W8A8 on the fp8 matrix path (enable_fp8_weights)

    def _w8p_qkv(self):
        """The fused Q|K|V matrix as the W8 operand of ops.gemm8 (Linear.w8p)."""
        names = ("to_q", "to_k", "to_v")
        return derived(self, "w8p_qkv", [_weight(self, n) for n in names],
                       lambda: O.quantize_fp8_padded(self._fused(names)))

    def _hm(self, planes):
        """head_major argument of the projection GEMMs: [rows][D] planes per head, the Q planes carrying
        scale * log2(e) (attention(..., q_prescaled=True))."""
        return (self.dim_head, planes, self.scale * 1.4426950408889634)

    def project_qkv(self, x2d, norm=None, head_major=False):
        """One GEMM for Q, K, V of a self-attention style layer -> (rows, 3*inner), or with head_major
        (3*heads, rows, dim_head).  With `norm`, x2d is the un-normalised input and the LayerNorm is
        folded into the GEMM."""
        hm = self._hm(self.heads) if head_major else None
        names = ("to_q", "to_k", "to_v")
        if self.fp8_mfma and norm is not None and fp8_mfma_ok(norm, x2d.shape[1], 3 * self.inner_dim, x2d):
            w8, sw = self._w8p_qkv()
            a8, sa = O.rowquant_fp8(x2d, (norm.weight, norm.bias, norm.eps))
            return O.gemm8(a8, sa, w8, sw, self._fused_bias(names), head_major=hm, dtype=x2d.dtype)
        if norm is not None:
            if not ln_fold_ok(norm, x2d.shape[1], 3 * self.inner_dim, x2d):
                return O.gemm(norm.run(x2d), self._fused(("to_q", "to_k", "to_v")),
                              self._fused_bias(("to_q", "to_k", "to_v")), head_major=hm)
            mods = (self.to_q, self.to_k, self.to_v)
            w, ln = fold_layernorm(self, "ln_qkv", norm, [m.weight for m in mods], [m.bias for m in mods])
            return O.gemm(x2d, w, None, ln=ln, head_major=hm)
        return O.gemm(x2d, self._fused(("to_q", "to_k", "to_v")), self._fused_bias(("to_q", "to_k", "to_v")),
                      head_major=hm)

    def project_kv(self, ctx2d):
        """K and V of the context in one GEMM -> (rows_ctx, 2*inner)."""
        return O.gemm(ctx2d, self._fused(("to_k", "to_v")), self._fused_bias(("to_k", "to_v")))

    def run_self(self, x2d, batch, lq, res=None, norm=None, ln_stats=False, ln_next=None):
        c, hd = self.inner_dim, self.heads
        if HEAD_MAJOR and self.to_q.bias is None:
            # Q | K | V written as one contiguous [rows][D] plane per head by the projection's epilogue: the
            # attention kernel then streams a head's K/V linearly, and Q arrives in log2 units
            qkv = self.project_qkv(x2d, norm, head_major=True)
            o = O.attention(qkv[:hd], qkv[hd:2 * hd], qkv[2 * hd:], batch, lq, lq, hd, self.dim_head,
                            q_prescaled=True)
        else:
            qkv = self.project_qkv(x2d, norm)
            o = O.attention(qkv[:, :c], qkv[:, c:2 * c], qkv[:, 2 * c:], batch, lq, lq, hd,
                            self.dim_head, self.scale)
        return self.to_out[0].run(o, res=res, ln_stats=ln_stats, ln_next=ln_next)

    def run_cross(self, x2d, batch, lq, ctx2d, lk, res=None, kv=None, norm=None, ln_stats=False, ln_next=None):
        c = self.inner_dim
        pre = self.__dict__.pop("_kv_prefetched", None)
        if kv is None and pre is not None and pre[0] is ctx2d:
            kv, side = pre[1], pre[2]                # projected ahead of time (bank GEMM, or a side stream)
            if side is not None:
                torch.cuda.current_stream().wait_stream(side)
                if not torch.cuda.is_current_stream_capturing():     # graph pools keep the block alive themselves
                    kv.record_stream(torch.cuda.current_stream())
        if kv is None:
            kv = self.project_kv(ctx2d)
        lk_dev = lk_dev_for(ctx2d, lk)               # the context is laid out at a capacity: its real length (round 6)
        probe = self.__dict__.get("_attn_probe")     # attn_maps.CrossAttnMapCapture: observes q and k, reroutes nothing
        if XATTN_FUSED and O.xattn320_ok(c, self.heads, lk, x2d.shape[0]) and self.to_q.in_features == c and self.to_q.bias is None \
                and not ln_stats and LN_FOLD == "0":
            # 28x50 level: q-projection, attention over the <= 128 context keys and out-projection + residual in ONE
            # launch (csrc/xattn.hip); it owns whole rows, so it also emits the next sub-layer's LayerNorm
            xn = x2d if norm is None else norm.run(x2d)
            lno = (ln_next.weight, ln_next.bias, ln_next.eps) if LN_PRODUCER and isinstance(ln_next, LayerNorm) else None
            if probe is not None:
                # q never reaches memory on this path: the probe gets it from the to_q call the unfused path makes (one
                # extra GEMM, for the probe only); the fused launch below still produces what flows on
                probe(self, self.to_q.run(xn, **({"head_major": self._hm(self.heads)} if HEAD_MAJOR else {})), kv[:, :c],
                      batch, lq, lk, HEAD_MAJOR, lk_dev)
            out = O.xattn320(xn, self.to_q.wx, self.to_out[0].wx, self.to_out[0].bias, kv[:, :c], kv[:, c:], batch, lq,
                             lk, self.scale, res=res, ln_out=lno, lk_dev=lk_dev)
            if lno is not None:
                out._ln_cache = (ln_next, out._ln_out)
            return out
        q_hm = HEAD_MAJOR and self.to_q.bias is None
        kw = {"head_major": self._hm(self.heads)} if q_hm else {}
        q = self.to_q.run(x2d, **kw) if norm is None else self.to_q.run_ln(x2d, norm, **kw)
        if probe is not None:
            probe(self, q, kv[:, :c], batch, lq, lk, q_hm, lk_dev)
        o = O.attention(q, kv[:, :c], kv[:, c:], batch, lq, lk, self.heads, self.dim_head, self.scale,
                        q_prescaled=q_hm, lk_dev=lk_dev)
        return self.to_out[0].run(o, res=res, ln_stats=ln_stats, ln_next=ln_next)

    def forward(self, hidden_states, encoder_hidden_states=None, attention_mask=None, **kw):
        return self.processor(self, hidden_states, encoder_hidden_states=encoder_hidden_states,
                              attention_mask=attention_mask, **kw)


def enable_fp8_weights(model, on=True, mfma=True):
    """EXTENSION (BASELINE configs[4], no reference semantics): W8A8 — the LayerNorm in front of the fused Q|K|V
    projections (attn1, attn4, the video block's attn_temp) and of the GEGLU projection quantises its output rows to
    e4m3fn (dd_rowquant_fp8) and the projection runs on v_mfma_scale_f32_16x16x128_f8f6f4 (dd_gemm8), wherever that is
    faster than the 16-bit pair (K = 640 / 1280, output >= 3 K wide: fp8_mfma_ok); everything else stays 16-bit.
    (The round-2 weights-only form — e4m3fn weights dequantised in registers by the row-panel GEMM family, mfma=False —
    was removed with that family in round 5.)

    Quantisation happens lazily from the CURRENT weights, so fold LoRA deltas first (dualdiff_amd.lora.fold_lora_).
    Returns the number of attention layers switched."""
    if not mfma:
        raise NotImplementedError("the weights-only fp8 form (row-panel GEMM family) was removed in round 5; use mfma=True")
    n = 0
    for mod in model.modules():
        if isinstance(mod, Attention):
            mod.fp8_mfma = bool(on)
            mod._drop_cache()
            n += 1
        elif isinstance(mod, GEGLU):
            mod.proj.fp8_mfma = bool(on)
            mod.proj._drop_cache()
    return n


def prefetch_cross_kv(model, ctx2d, side):
    """Projects K/V of every built-in cross-attention layer of `model` for the context `ctx2d` on the
    stream `side`.  The context (text / camera / box tokens) does not depend on the latents, so these
    GEMMs leave the serial chain of the step and fill CUs the chain leaves idle; the first layer that
    needs them joins the side stream.  Same kernels, same inputs -> same bits."""
    main = torch.cuda.current_stream()
    side.wait_stream(main)
    with torch.cuda.stream(side):
        for blk in model.modules():
            mod = getattr(blk, "attn2", None) if isinstance(blk, BasicTransformerBlock) else None
            if mod is not None and mod.is_cross and isinstance(mod.processor, HIPAttnProcessor):
                mod.__dict__["_kv_prefetched"] = (ctx2d, mod.project_kv(ctx2d), side)


def drop_prefetched_kv(model, side):
    """Joins `side` back and forgets any K/V no layer consumed (keeps graph capture well-formed)."""
    torch.cuda.current_stream().wait_stream(side)
    for mod in model.modules():
        if isinstance(mod, Attention):
            mod.__dict__.pop("_kv_prefetched", None)


class GEGLU(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = Linear(dim_in, dim_out * 2)


class FeedForward(nn.Module):
    """Linear(C, 8C) with the GEGLU gate fused into the GEMM epilogue, then Linear(4C, C) with
    the residual add fused."""

    def __init__(self, dim, mult=4):
        super().__init__()
        self.net = nn.ModuleList([GEGLU(dim, dim * mult), _Dropout(), Linear(dim * mult, dim)])

    def run(self, x2d, res=None, norm=None, defer_out=False):
        """defer_out: return the gated hidden (rows, 4C) instead of net[2](hidden) + res — the caller folds
        the output projection into the layer that follows (Transformer2DModel.run)."""
        if norm is None:
            g = self.net[0].proj.run(x2d, epilogue=O.DD_EPI_GEGLU)
        else:
            g = self.net[0].proj.run_ln(x2d, norm, epilogue=O.DD_EPI_GEGLU)
        if defer_out:
            return g
        return self.net[2].run(g, res=res)


class BasicTransformerBlock(nn.Module):
    """Stock block (ControlNet): LN -> self-attn -> + ; LN -> cross-attn -> + ; LN -> FF -> +."""

    def __init__(self, dim, num_attention_heads, attention_head_dim, cross_attention_dim=None, **unused):
        super().__init__()
        self.dim = dim
        self.norm1 = LayerNorm(dim)
        self.attn1 = Attention(dim, None, num_attention_heads, attention_head_dim)
        self.norm2 = LayerNorm(dim)
        self.attn2 = Attention(dim, cross_attention_dim, num_attention_heads, attention_head_dim)
        self.norm3 = LayerNorm(dim)
        self.ff = FeedForward(dim)

    def _attn(self, attn, norm, h, batch, l, ctx=None, lc=0, ln_next=True, next_norm=None):
        """LayerNorm `norm` + `attn` (+ residual h).  The built-in processor folds the LayerNorm
        into the Q(KV) projection and the residual into the out-projection; foreign processors get
        the normalised (B, L, C) tensor through the diffusers protocol."""
        if isinstance(attn.processor, HIPAttnProcessor) and not getattr(attn.processor, "chunked", False):
            st = ln_next and want_ln_stats()          # the output feeds the block's next LayerNorm
            if ctx is None:
                return attn.run_self(h, batch, l, res=h, norm=norm, ln_stats=st, ln_next=next_norm)
            return attn.run_cross(h, batch, l, ctx, lc, res=h, norm=norm, ln_stats=st, ln_next=next_norm)
        e = None if ctx is None else ctx.reshape(batch, lc, -1)
        out = attn(norm.run(h).reshape(batch, l, -1), encoder_hidden_states=e)
        return O.add(out.reshape(batch * l, -1).contiguous(), h)

    def run(self, h, batch, l, ctx2d, lc, defer_ff_out=False):
        h = self._attn(self.attn1, self.norm1, h, batch, l, next_norm=self.norm2)
        h = self._attn(self.attn2, self.norm2, h, batch, l, ctx2d, lc, next_norm=self.norm3)
        if defer_ff_out:                   # -> (gated hidden, residual): see Transformer2DModel.run
            return self.ff.run(h, norm=self.norm3, defer_out=True), h
        return self.ff.run(h, res=h, norm=self.norm3)


class Transformer2DModel(nn.Module):
    """GN(1e-6) -> 1x1 conv -> blocks -> 1x1 conv -> + residual; NHWC makes the token reshapes free."""

    def __init__(self, num_attention_heads, attention_head_dim, in_channels, cross_attention_dim,
                 norm_num_groups=32, block_cls=BasicTransformerBlock, block_kwargs=None):
        super().__init__()
        inner = num_attention_heads * attention_head_dim
        self.norm = GroupNorm(norm_num_groups, in_channels, eps=1e-6)
        self.proj_in = Linear(in_channels, inner, conv=True)
        self.transformer_blocks = nn.ModuleList([
            block_cls(inner, num_attention_heads, attention_head_dim, cross_attention_dim=cross_attention_dim,
                      **(block_kwargs or {}))])
        self.proj_out = Linear(inner, in_channels, conv=True)

    # The block ends with  t = W2 g + b2 + h  (feed-forward output projection + residual) and proj_out is
    # another Linear right behind it with nothing in between (diffusers Transformer2DModel.forward; reference
    # blocks.py:224-236): y = Wp t + bp + x = [Wp W2 | Wp] [g | h] + (Wp b2 + bp) + x — ONE GEMM over the
    # two-source operand [g | h] (K = 5C) instead of two GEMMs and a round trip of t through HBM.  Folded in
    # fp32 when the weights change, like the attn4 connector.  DD_FOLD_PROJ_OUT=0 turns it off.
    fold_proj_out = __import__("os").environ.get("DD_FOLD_PROJ_OUT", "1") != "0"

    def _folded_ff_out(self, blk):
        w2, b2 = blk.ff.net[2].weight, blk.ff.net[2].bias
        wp, bp = self.proj_out.weight, self.proj_out.bias

        def build():
            wpf = wp.detach().float().reshape(wp.shape[0], -1)
            w = torch.cat([wpf @ w2.detach().float(), wpf], dim=1).to(wp.dtype).contiguous()
            return w, (wpf @ b2.detach().float() + bp.detach().float()).to(wp.dtype).contiguous()
        return derived(self.proj_out, "fold", [w2, b2, wp, bp], build)

    def run(self, x, m, h, w, ctx2d, lc):
        a = self.norm.run(x, m, h * w, False)
        t = self.proj_in.run(a, ln_stats=want_ln_stats(), ln_next=getattr(self.transformer_blocks[0], "norm1", None))
        blocks = self.transformer_blocks
        if self.fold_proj_out and len(blocks) == 1 and isinstance(getattr(blocks[0], "ff", None), FeedForward):
            g, hres = blocks[0].run(t, m, h * w, ctx2d, lc, defer_ff_out=True)
            wf, bf = self._folded_ff_out(blocks[0])
            return O.gemm(g, wf, bf, a2=hres, res=x)
        for blk in blocks:
            t = blk.run(t, m, h * w, ctx2d, lc)
        return self.proj_out.run(t, res=x)


# ------------------------------------------------------------------------------- blocks ---
class CrossAttnDownBlock2D(nn.Module):
    has_cross_attention = True

    def __init__(self, in_channels, out_channels, temb_channels, num_layers, heads, cross_attention_dim,
                 add_downsample, groups=32, eps=1e-5, block_cls=BasicTransformerBlock, block_kwargs=None):
        super().__init__()
        self.resnets = nn.ModuleList([
            ResnetBlock2D(in_channels if i == 0 else out_channels, out_channels, temb_channels, groups, eps)
            for i in range(num_layers)])
        self.attentions = nn.ModuleList([
            Transformer2DModel(heads, out_channels // heads, out_channels, cross_attention_dim, groups,
                               block_cls, block_kwargs) for _ in range(num_layers)])
        self.downsamplers = nn.ModuleList([Downsample2D(out_channels)]) if add_downsample else None


class DownBlock2D(nn.Module):
    has_cross_attention = False

    def __init__(self, in_channels, out_channels, temb_channels, num_layers, add_downsample, groups=32, eps=1e-5):
        super().__init__()
        self.resnets = nn.ModuleList([
            ResnetBlock2D(in_channels if i == 0 else out_channels, out_channels, temb_channels, groups, eps)
            for i in range(num_layers)])
        self.attentions = None
        self.downsamplers = nn.ModuleList([Downsample2D(out_channels)]) if add_downsample else None


def run_down_block(blk, x, m, h, w, temb_slices, ctx2d, lc):
    """-> (x, h, w, [skip tensors with their (h, w)])."""
    skips = []
    for i, resnet in enumerate(blk.resnets):
        x = resnet.run(x, m, h, w, temb_slices[id(resnet)],
                       gn_next=blk.attentions[i].norm if blk.attentions is not None else None)
        if blk.attentions is not None:
            x = blk.attentions[i].run(x, m, h, w, ctx2d, lc)
        skips.append((x, h, w))
    if blk.downsamplers is not None:
        conv = blk.downsamplers[0].conv
        x = conv.run(x, m, h, w)
        h, w = conv.out_hw(h, w)
        skips.append((x, h, w))
    return x, h, w, skips


class UNetMidBlock2DCrossAttn(nn.Module):
    has_cross_attention = True

    def __init__(self, in_channels, temb_channels, heads, cross_attention_dim, groups=32, eps=1e-5,
                 block_cls=BasicTransformerBlock, block_kwargs=None):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(in_channels, in_channels, temb_channels, groups, eps)
                                      for _ in range(2)])
        self.attentions = nn.ModuleList([
            Transformer2DModel(heads, in_channels // heads, in_channels, cross_attention_dim, groups,
                               block_cls, block_kwargs)])

    def run(self, x, m, h, w, temb_slices, ctx2d, lc, extra_res=None):
        x = self.resnets[0].run(x, m, h, w, temb_slices[id(self.resnets[0])], gn_next=self.attentions[0].norm)
        x = self.attentions[0].run(x, m, h, w, ctx2d, lc)
        return self.resnets[1].run(x, m, h, w, temb_slices[id(self.resnets[1])], extra_res=extra_res)


class UpBlock2D(nn.Module):
    has_cross_attention = False

    def __init__(self, in_channels, prev_output_channel, out_channels, temb_channels, num_layers,
                 add_upsample, groups=32, eps=1e-5):
        super().__init__()
        self.resnets = _up_resnets(in_channels, out_channels, prev_output_channel, temb_channels, num_layers, groups, eps)
        self.attentions = None
        self.upsamplers = nn.ModuleList([Upsample2D(out_channels)]) if add_upsample else None


class CrossAttnUpBlock2D(nn.Module):
    has_cross_attention = True

    def __init__(self, in_channels, out_channels, prev_output_channel, temb_channels, num_layers, heads,
                 cross_attention_dim, add_upsample, groups=32, eps=1e-5, block_cls=BasicTransformerBlock,
                 block_kwargs=None):
        super().__init__()
        self.resnets = _up_resnets(in_channels, out_channels, prev_output_channel, temb_channels, num_layers, groups, eps)
        self.attentions = nn.ModuleList([
            Transformer2DModel(heads, out_channels // heads, out_channels, cross_attention_dim, groups,
                               block_cls, block_kwargs) for _ in range(num_layers)])
        self.upsamplers = nn.ModuleList([Upsample2D(out_channels)]) if add_upsample else None


def _up_resnets(in_channels, out_channels, prev_output_channel, temb_channels, num_layers, groups, eps):
    rs = []
    for i in range(num_layers):
        skip = in_channels if i == num_layers - 1 else out_channels
        rin = prev_output_channel if i == 0 else out_channels
        rs.append(ResnetBlock2D(rin + skip, out_channels, temb_channels, groups, eps))
    return nn.ModuleList(rs)


def run_up_block(blk, x, m, h, w, skips, temb_slices, ctx2d, lc, up_size):
    """skips: list of (tensor, h, w) consumed from the end.  The concat [x, skip] is never
    materialised: GroupNorm and the 1x1 shortcut read both sources."""
    for i, resnet in enumerate(blk.resnets):
        s, sh, sw = skips.pop()
        assert (sh, sw) == (h, w)
        x = resnet.run(x, m, h, w, temb_slices[id(resnet)], x2=s,
                       gn_next=blk.attentions[i].norm if blk.attentions is not None else None)
        if blk.attentions is not None:
            x = blk.attentions[i].run(x, m, h, w, ctx2d, lc)
    if blk.upsamplers is not None:
        conv = blk.upsamplers[0].conv
        size = up_size if up_size is not None else (2 * h, 2 * w)
        x = conv.run(x, m, h, w, up_size=size)      # nearest upsample folded into the conv gather
        h, w = size
    return x, h, w


class TimeEmbProjBank:
    """All ResnetBlock2D.time_emb_proj layers of a model evaluated as ONE GEMM per forward
    (~35 tiny launches -> 1).  Returns {id(resnet): (m, cout) view}."""

    def __init__(self, model):
        self.resnets = [mod for mod in model.modules() if isinstance(mod, ResnetBlock2D)]

    def stacked(self):
        """(weights, biases) of every time_emb_proj stacked along N."""
        ps = [r._modules["time_emb_proj"]._parameters for r in self.resnets]        # (see _weight)
        ws, bs = [p["weight"] for p in ps], [p["bias"] for p in ps]
        return derived(self, "wb", ws + bs, lambda: (torch.cat([w.detach() for w in ws], 0).contiguous(),
                                                     torch.cat([b.detach() for b in bs], 0).contiguous()))

    def run(self, emb_act):
        allv = O.gemm(emb_act, *self.stacked())
        out, off = {}, 0
        for r in self.resnets:
            out[id(r)] = allv[:, off:off + r.out_channels]
            off += r.out_channels
        return out


class CrossKVBank:
    """K and V of EVERY text cross-attention (attn2) of a model for one context, as ONE GEMM per
    forward: the context tokens are the same for all layers, so the [2C_l, 768] projection matrices
    of the 16 (UNet) / 7 (ControlNet) layers are stacked along N and each layer attends to its column
    slice of the result (the attention kernel takes row-strided K/V).  Replaces 16 / 7 small
    launch-bound GEMMs on the serial chain by one 1176 x 24960 x 768 (UNet) GEMM."""

    def __init__(self, model):
        self.layers = []
        for blk in model.modules():
            mod = getattr(blk, "attn2", None) if isinstance(blk, BasicTransformerBlock) else None
            if mod is not None and mod.is_cross:
                self.layers.append(mod)

    def banked(self, k):
        """The layers whose K/V projection of a `k`-wide context goes through the bank."""
        return [m for m in self.layers if isinstance(m.processor, HIPAttnProcessor)
                and m.to_k.in_features == k and m.to_k.bias is None and m.to_v.bias is None]

    def stacked(self, mods):
        """The fused K|V matrices of `mods` stacked along N."""
        return derived(self, "kv", [_weight(m, n) for m in mods for n in ("to_k", "to_v")],
                       lambda: torch.cat([m._fused(("to_k", "to_v")) for m in mods], dim=0).contiguous())

    def run(self, ctx2d):
        mods = self.banked(ctx2d.shape[1])
        if not mods:
            return
        allkv = O.gemm(ctx2d, self.stacked(mods))
        off = 0
        for m in mods:
            n2 = 2 * m.inner_dim
            m.__dict__["_kv_prefetched"] = (ctx2d, allkv[:, off:off + n2], None)
            off += n2

    def drop(self):
        for m in self.layers:
            m.__dict__.pop("_kv_prefetched", None)


def seeded_init_(module, seed=0):
    """Deterministic name-keyed random initialisation for synthetic-weight runs (bench / smoke):
    fan-in scaled normals for matrices, ~1 for norm scales, small biases.  Mirrors
    oracle/init_utils.py so the CPU baseline can be given identical weights, without importing it."""
    import zlib
    sd = {}
    for name, t in module.state_dict().items():
        if not t.is_floating_point():
            sd[name] = t
            continue
        g = torch.Generator().manual_seed((zlib.crc32(name.encode()) ^ (seed * 2654435761)) & 0x7FFFFFFF)
        if t.dim() >= 2:
            v = torch.randn(t.shape, generator=g) * (t[0].numel() ** -0.5)
        elif name.endswith("weight"):
            v = 1.0 + 0.1 * torch.randn(t.shape, generator=g)
        else:
            v = 0.05 * torch.randn(t.shape, generator=g)
        sd[name] = v
    module.load_state_dict(sd, strict=True)
    return module


def device_init_(module, seed=0):
    """Same distributions as seeded_init_, drawn directly on the module's device (fast path for
    the full-size synthetic-weight benchmark; not bit-reproducible against the CPU generator)."""
    g = None
    with torch.no_grad():
        for name, t in module.state_dict().items():
            if not t.is_floating_point():
                continue
            if g is None or g.device != t.device:
                g = torch.Generator(device=t.device).manual_seed(seed)
            if t.dim() >= 2:
                v = torch.randn(t.shape, generator=g, device=t.device, dtype=torch.float32) * (t[0].numel() ** -0.5)
            elif name.endswith("weight"):
                v = 1.0 + 0.1 * torch.randn(t.shape, generator=g, device=t.device, dtype=torch.float32)
            else:
                v = 0.05 * torch.randn(t.shape, generator=g, device=t.device, dtype=torch.float32)
            t.copy_(v.to(t.dtype))
    for m in module.modules():
        if hasattr(m, "_drop_cache"):
            m._drop_cache()
    if hasattr(module, "_invalidate"):
        module._invalidate()
    return module
