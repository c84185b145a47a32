"""Torch-tensor front end of the HIP C-ABI (device memory + stream plumbing only).

Every function launches hand-written gfx950 kernels from libdualdiff_hip.so on torch's
current stream.  Tensors are token-major / NHWC 2-D views (rows, channels) in fp16 or bf16.
There is no eager fallback: a non-GPU tensor raises.

The scratch buffers live in _workspace, the per-launch timing in _timer, the tile / split-K tuner and its table in
tuning; their public names are re-exported here.
"""
import collections as _collections
import ctypes
import os as _os

import torch

from . import _native, _timer, _workspace, tuning, upfold as _upfold
from ._consts import device_const
from ._native import DD_BF16, DD_EPI_GEGLU, DD_EPI_NONE, DD_EPI_SILU, DD_F16, AttnDesc, Gemm8Desc, GemmDesc, XAttnDesc
from ._timer import KernelTimer, _stream, set_timer  # noqa: F401
from ._workspace import workspace, workspace_owner  # noqa: F401
from .image_tables import (BILINEAR_MAX, PNG_FILE_FIXED, _image_lut, _image_mean_std, device_bilinear_tables,  # noqa: F401
                           device_jpeg_tables, device_tables, image_norm_lut, jpeg_header, png_capacity, png_unit_lut)
from .tuning import (CHALLENGE_TILES, TUNE_TABLE_PATH, forget_tuned, load_tuned, save_tuned,  # noqa: F401
                     tune_candidates, tuned_table)

_THIN_CONV = _os.environ.get("DD_THIN_CONV", "1") != "0"       # A/B switch of dd_conv3x3_thin
# split-K reduce folded into the GroupNorm that consumes the conv's output (dd_groupnorm_splitk): 50 launches fewer per
# step, bit-identical — and 0.5 % SLOWER on the step (84.9 vs 85.4 steps/s over three alternating pairs: the norm then
# reads `split` fp32 slabs with the few workgroups a 28-pixel image gives it, where the separate reduce spreads them over
# the chip), so it is OFF by default; DD_GN_SPLITK=1 turns it on
GN_SPLITK = _os.environ.get("DD_GN_SPLITK", "0") == "1"
LN_OUT_TILE = int(_os.environ.get("DD_LN_OUT_TILE", "0"))
# dd_xattn320 owns 80-row tiles, one workgroup per CU (135 KB of LDS), and every workgroup re-stages both 205 KB weight
# matrices: it beats the three-launch form while its grid is ONE residency generation (12 instances x 1400 rows = 210
# workgroups on 256 CUs: 40 vs 45 us for the SFA module) and loses beyond it (48 instances = 840 workgroups: 127 vs 114 us,
# profiles/r03_sfa_roofline.txt).  Above this many workgroups the callers take the three launches.
XATTN_MAX_WGS = int(_os.environ.get("DD_XATTN_MAX_WGS", "256"))
CAUSAL_ATTN_MAX_L = 128         # DD_CAUSAL_ATTN_MAX_L of include/dualdiff_hip.h
_FDT = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}


def _dtype_code(dtype):
    if dtype == torch.float16:
        return DD_F16
    if dtype == torch.bfloat16:
        return DD_BF16
    raise TypeError("dualdiff_amd ops take fp16 / bf16 tensors, got %s" % dtype)


def _dt(t):
    return _dtype_code(t.dtype)


def _tname(code):
    return "f16" if code == DD_F16 else "bf16"


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("dualdiff_amd ops run on the GPU only (got a %s tensor); "
                               "there is no CPU fallback" % t.device)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _forget_derived(t):
    """A tensor that is about to be (re)written through its data pointer loses whatever an earlier producer
    attached to it (LayerNorm emitted by an epilogue, row statistics): those describe the OLD contents."""
    for a in ("_ln_cache", "_ln_out", "_ln_stats", "_gn_cache", "_unwritten"):
        if hasattr(t, a):
            delattr(t, a)


def _written(*ts):
    """Counts a version on every tensor of the CALLER's that a kernel is about to write through its data pointer, as
    torch does for its own in-place ops: `tensor._version` is what tells a reader that the bytes changed
    (model_base.sibling_overlap proves with it that an argument was ready before an earlier point of the stream;
    layers.derived keys packed weights on it).  Only a host counter — nothing is launched, also inside a stream capture.
    Tensors the wrapper allocated itself need none (nobody has seen them), inference tensors count none (and are never
    vouched for).  tests/sibling_cases.py lists every wrapper that must come through here."""
    for t in ts:
        if t is not None and not t.is_inference():
            torch.autograd.graph.increment_version(t)


def _out_or_new(out, shape, dtype, device, what):
    """The tensor a wrapper writes: a fresh one (`shape` may be a tensor whose layout it takes: torch.empty_like), or
    the caller's `out` — of the dtype the kernel stores, without the attributes that described its old contents, and
    one version on."""
    if out is None:
        return torch.empty_like(shape) if isinstance(shape, torch.Tensor) else torch.empty(shape, dtype=dtype, device=device)
    if out.dtype != dtype:
        raise TypeError("%s: out must be %s" % (what, dtype))
    _forget_derived(out)
    _written(out)
    return out


def _rows2d(t):
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("expected a 2-D tensor with unit inner stride, got shape %s stride %s"
                         % (tuple(t.shape), t.stride()))
    return t


def _check_lk_dev(lk_dev):
    if lk_dev is not None and (lk_dev.dtype != torch.int32 or lk_dev.numel() < 1):
        raise TypeError("lk_dev must be an int32 device tensor")


def _epilogue_side(d, dtype, bias, rowvec, rows_per_inst, res, out, alpha, accumulate, epilogue, tile, split_k):
    """The output side of a GemmDesc, the same for gemm and conv3x3: alpha * (acc + bias + rowvec[row // rows_per_inst])
    + res -> out, and the tile / split-K the caller asked for (0 = tuned)."""
    d.bias = bias.data_ptr() if bias is not None else None
    if rowvec is not None:
        rowvec = _rows2d(rowvec)
        d.rowvec = rowvec.data_ptr(); d.ld_rowvec = rowvec.stride(0); d.rows_per_inst = rows_per_inst
    if res is not None:
        res = _rows2d(res)
        d.res = res.data_ptr(); d.ldres = res.stride(0)
    out = _rows2d(out)
    d.out = out.data_ptr(); d.ldc = out.stride(0)
    d.alpha = alpha; d.accumulate = int(accumulate); d.epilogue = epilogue
    d.dtype = dtype; d.tile = tile; d.split_k = split_k


def _tune(L, d, key, out_shape, dtype, device, warm):
    """Sets d.tile / d.split_k from the table or the run-time tuner.  CHALLENGE_TILES is read here, from this module, at
    call time: bench.py --challenge-tiles assigns it after import."""
    d.tile, d.split_k = tuning.tune(L, d, key, out_shape, dtype, device, warm, CHALLENGE_TILES)[:2]


def gemm(a, w, bias=None, *, a2=None, res=None, rowvec=None, rows_per_inst=1, alpha=1.0,
         out=None, accumulate=False, epilogue=DD_EPI_NONE, tile=0, split_k=0, ln=None, out_f32=False,
         ln_stats=False, head_major=None, ln_out=None):
    """out = alpha * (cat(a, a2) @ w.T + bias + rowvec[row // rows_per_inst]) + res  (fused).
    head_major = (D, scaled_planes, scale): the result comes back as (n / D, rows, D) — one contiguous
    [rows][D] plane per head of a fused Q|K|V projection, the first `scaled_planes` planes multiplied by
    `scale` before rounding (what `attention(..., q_prescaled=True)` expects).
    out_f32: the result is stored as fp32 (attention logits that feed a softmax).
    ln_stats: the epilogue also leaves per-row partial sums of the output (n % 32 == 0) as `out._ln_stats`;
    a later gemm(out, ..., ln=...) picks them up instead of recomputing the row statistics.

    ln_out = (gamma, beta, eps) (n == 320 only): the epilogue ALSO writes LayerNorm(out) — returned as the
    attribute `out._ln_out` — from a tile that owns whole rows (tile 40, 80 x 320).

    ln = (colsum_f32, bias_f32, eps): LayerNorm fold — `a` is the UN-normalised input, `w` the
    gamma-scaled weight; the kernel computes the row statistics itself (include/dualdiff_hip.h)."""
    lib = _native.load()
    _need_gpu(a, w, bias, a2, res, rowvec, out)
    stats_in = getattr(a, "_ln_stats", None) if ln is not None else None
    a = _rows2d(a)
    w = _rows2d(w)
    rows = a.shape[0]
    k = a.shape[1] + (a2.shape[1] if a2 is not None else 0)
    n_w = w.shape[0]
    if w.shape[1] != k or not w.is_contiguous():
        raise ValueError("weight must be contiguous [N, K=%d], got %s" % (k, tuple(w.shape)))
    n = n_w // 2 if epilogue == DD_EPI_GEGLU else n_w
    odt = torch.float32 if out_f32 else a.dtype
    hm_out = None
    if head_major is not None:
        hd, hplanes, hscale = head_major
        if out is not None or n % hd or hd % 8 or out_f32 or epilogue != DD_EPI_NONE or accumulate or ln_stats:
            raise ValueError("head_major needs a plain epilogue, its own output and n % D == 0")
        hm_out = torch.empty((n // hd, rows, hd), dtype=a.dtype, device=a.device)
        out = hm_out.view(rows, n)           # same bytes; the kernel ignores ldc in this mode
    else:
        out = _out_or_new(out, (rows, n), odt, a.device, "gemm")
    d = GemmDesc()
    d.out_f32 = int(bool(out_f32))
    if hm_out is not None:
        d.out_headmajor_d, d.hm_scaled_planes, d.hm_scale = int(hd), int(hplanes), float(hscale)
    d.a = a.data_ptr(); d.lda = a.stride(0); d.k1 = a.shape[1]
    if a2 is not None:
        a2 = _rows2d(a2)
        d.a2 = a2.data_ptr(); d.lda2 = a2.stride(0)
    d.rows, d.n, d.k = rows, n, k
    d.w = w.data_ptr()
    d.conv = 0
    _epilogue_side(d, _dt(a), bias, rowvec, rows_per_inst, res, out, alpha, accumulate, epilogue, tile, split_k)
    if ln is not None:
        if bias is not None or a2 is not None:
            raise ValueError("gemm(ln=...) folds the bias and takes a single source")
        colsum, lnb, eps = ln
        _need_gpu(colsum, lnb)
        if colsum.dtype != torch.float32 or lnb.dtype != torch.float32 or colsum.numel() != n_w or lnb.numel() != n_w:
            raise ValueError("ln fold vectors must be fp32 with %d entries" % n_w)
        d.ln_colsum, d.ln_bias, d.ln_eps = colsum.data_ptr(), lnb.data_ptr(), float(eps)
        if stats_in is not None:
            if tuple(stats_in.shape) != (rows, k // 32, 2) or stats_in.dtype != torch.float32:
                raise ValueError("stale LayerNorm statistics attached to the input")
            d.ln_stats_in = stats_in.data_ptr()
    if w.dtype != a.dtype:
        raise TypeError("gemm: weight dtype %s != activation dtype %s" % (w.dtype, a.dtype))
    ln_second = None
    if ln_out is not None:
        g_, b_, eps_ = ln_out
        _need_gpu(g_, b_)
        if n != 320 or g_.numel() != n or b_.numel() != n or g_.dtype != a.dtype or b_.dtype != a.dtype:
            raise ValueError("ln_out needs n == 320 and %s gamma / beta of 320 entries" % a.dtype)
        ln_second = torch.empty((rows, n), dtype=a.dtype, device=a.device)
        d.ln_out, d.ld_ln_out = ln_second.data_ptr(), n
        d.lno_gamma, d.lno_beta, d.ln_eps = g_.data_ptr(), b_.data_ptr(), float(eps_)
        # the 80 x 320 whole-row tiles: 74 (pipelined K loop, round 5) / 40 (dd_gemm2, persistent walk); 0 = the library picks
        # by the row count (DD_LN_OUT_TILE forces one for A/Bs)
        if tile not in (40, 74):
            tile = LN_OUT_TILE
        d.tile, d.split_k = tile, 1
        tile = -1                                 # (not 0: no tuner lookup for this call)
    stats_out = None
    if ln_stats:
        if n % 32 or epilogue == DD_EPI_GEGLU or out_f32:
            raise ValueError("ln_stats needs a plain epilogue and n % 32 == 0")
        stats_out = torch.empty((rows, n // 32, 2), dtype=torch.float32, device=a.device)
        d.ln_stats_out = stats_out.data_ptr()
    L = tuning.launcher(lib)
    if tile == 0 and split_k == 0:
        key = tuning.gemm_key(rows, n, k, epilogue, d.dtype, a2 is not None, ln is not None, out_f32=out_f32,
                              stats_out=ln_stats, stats_in=stats_in is not None,
                              head_major=head_major[0] if head_major is not None else None, res=res is not None,
                              acc=accumulate)
        _tune(L, d, key, (rows, n), odt, a.device, (a, a2, res))
    _workspace.attach(d, a.device, lambda: L.ws_bytes(d))
    _timer.gemm_launch(L, d, "gemm", "gemm", n_w, rows * k)
    if stats_out is not None:
        out._ln_stats = stats_out
    if ln_second is not None:
        out._ln_out = ln_second
    return hm_out if hm_out is not None else out


def thin_conv_ok(cin, cout, stride, m):
    return _THIN_CONV and (cin, cout, stride) in ((8, 16, 1), (16, 16, 1), (16, 32, 2), (32, 32, 1), (8, 32, 1), (16, 32, 1),
                                                  (16, 16, 2), (8, 16, 2), (32, 16, 1)) and m <= 65535


def conv3x3(x, w, bias, m, hin, win, *, stride=1, up_size=None, rowvec=None, res=None,
            alpha=1.0, out=None, accumulate=False, epilogue=DD_EPI_NONE, tile=0, split_k=0, gn_next=None, pad=1,
            upfold=None):
    """3x3 / pad 1 convolution as an implicit GEMM on an NHWC batch.

    pad=0 (stride 2, no upsample): diffusers' Downsample2D(padding=0) — F.pad(x, (0, 1, 0, 1)) then a 3x3 / stride 2 /
    pad 0 conv, hout = (hin - 2) // 2 + 1 — launched through dd_gemm_conv_pad with its own tuning key.

    gn_next = (GroupNorm module, silu, want_x): the GroupNorm that reads this conv's output next.  When the conv runs
    split-K (two launches) and the image takes the single-launch GroupNorm, the REDUCE launch is replaced by
    dd_groupnorm_splitk: it adds the slabs, applies the epilogue and normalises in one go; the result is attached as
    `out._gn_cache` (GroupNorm.run picks it up) and `out` itself is written only if want_x.

    x: (m*hin*win, cin); w: (cout, 9*cin) packed [cout][ky][kx][cin]; optional nearest
    upsample of x to `up_size` first; rowvec: (m, cout) per-instance vector (time embedding).

    upfold: the weights of `w` folded for this nearest map (upfold.fold_weight: (classes * cout, 4 * cin)); the launch is
    then the 2 x 2-tap form dd_gemm2u_kernel with its own tuning key.  Without it a resize takes the 9-tap gather.
    Returns (m*hout*wout, cout)."""
    lib = _native.load()
    _need_gpu(x, w, bias, res, rowvec, out)
    x = _rows2d(x)
    cin = x.shape[1]
    if not x.is_contiguous() or x.shape[0] != m * hin * win:
        raise ValueError("conv input must be contiguous (m*h*w, cin)")
    hv, wv = (hin, win) if up_size is None else (int(up_size[0]), int(up_size[1]))
    if pad not in (0, 1):
        raise ValueError("conv3x3: pad is 1 (nn.Conv2d(padding=1)) or 0 (Downsample2D(padding=0))")
    if pad == 0 and (stride != 2 or up_size is not None or hin < 2 or win < 2):
        raise ValueError("conv3x3(pad=0) is the stride-2 downsample of an image of at least 2 x 2 pixels, without upsample")
    hout = (hv + pad + 1 - 3) // stride + 1
    wout = (wv + pad + 1 - 3) // stride + 1
    cout = w.shape[0]
    if w.shape[1] != 9 * cin or not w.is_contiguous():
        raise ValueError("conv weight must be contiguous [cout, 9*cin]")
    rows = m * hout * wout
    if upfold is not None:
        _need_gpu(upfold)
        ncls = _upfold.num_classes(hin, win, hv, wv) if pad == 1 and stride == 1 and up_size is not None and cin % 64 == 0 else 0
        if ncls == 0:
            raise ValueError("conv3x3(upfold=...): no folded form for %dx%d -> %dx%d, stride %d, cin %d" % (hin, win, hv, wv, stride, cin))
        if tuple(upfold.shape) != (ncls * cout, 4 * cin) or not upfold.is_contiguous() or upfold.dtype != x.dtype:
            raise ValueError("folded conv weight must be contiguous %s [%d * cout, 4 * cin]" % (x.dtype, ncls))
    out = _out_or_new(out, (rows, cout), x.dtype, x.device, "conv3x3")
    if pad == 1 and thin_conv_ok(cin, cout, stride, m) and up_size is None and rowvec is None and res is None and alpha == 1.0 \
            and not accumulate and epilogue in (DD_EPI_NONE, DD_EPI_SILU) and tile == 0 and split_k == 0 \
            and out.is_contiguous():
        # thin channel counts on a large image (the condition embedder's first layers): patch-in-LDS direct conv
        def book():
            suffix, flops, nbytes = _timer.mm_cost("conv", rows, cout, 9 * cin, x.numel(), cout)
            return "dd_conv3x3_thin_kernel" + suffix, flops, nbytes
        _timer.launch("conv3x3_thin", lib.dd_conv3x3_thin, _ptr(x), _ptr(w), _ptr(bias), _ptr(out), m, hin, win, cin, cout,
                      stride, int(epilogue == DD_EPI_SILU), _dt(x), _stream(), book=book)
        return out
    d = GemmDesc()
    d.a = x.data_ptr(); d.lda = cin; d.k1 = 9 * cin
    d.rows, d.n, d.k = rows, cout, 9 * cin
    d.w = w.data_ptr()
    d.conv = 1
    d.hin, d.win, d.cin, d.hv, d.wv = hin, win, cin, hv, wv
    d.hout, d.wout, d.stride = hout, wout, stride
    if upfold is not None:
        d.w, d.k, d.k1, d.upfold = upfold.data_ptr(), 4 * cin, 4 * cin, 1
    _epilogue_side(d, _dt(x), bias, rowvec, hout * wout, res, out, alpha, accumulate, epilogue, tile, split_k)
    L = tuning.launcher(lib, pad)
    what = "conv3x3" if pad == 1 else "conv3x3(pad=0)"
    if tile == 0 and split_k == 0:
        key = (tuning.conv_key if pad == 1 else tuning.conv_pad0_key)(m, hin, win, cin, cout, stride, hv, wv, d.dtype)
        hit = None
        if upfold is not None:
            key = tuning.conv_upfold_key(m, hin, win, cin, cout, hv, wv, d.dtype)
            hit = tuning.upfold_tuned(key)
        if hit is not None and hit[0] != 0:
            d.tile, d.split_k = hit[:2]
        else:
            _tune(L, d, key, (rows, cout), x.dtype, x.device, (x, res))
    need = _workspace.attach(d, x.device, lambda: L.ws_bytes(d))
    if pad == 1 and gn_next is not None and GN_SPLITK and need > 0 and alpha == 1.0 and not accumulate \
            and epilogue == DD_EPI_NONE:
        gmod, gsilu, want_x = gn_next
        split = _timer.plan_of(L, d)[1]
        if split > 1 and lib.dd_groupnorm_is_fused(hout * wout, cout, gmod.num_groups):
            # partial slabs only; dd_groupnorm_splitk is reduce + epilogue + GroupNorm(+SiLU) in one launch
            y = torch.empty((rows, cout), dtype=x.dtype, device=x.device)
            _timer.gemm_launch(L, d, what, "conv", cout, x.numel(), reduce=False)
            _timer.launch("groupnorm_splitk", lib.dd_groupnorm_splitk, ctypes.c_void_p(d.ws + 65536), split, _ptr(bias),
                          _ptr(rowvec), rowvec.stride(0) if rowvec is not None else 0, _ptr(res),
                          res.stride(0) if res is not None else 0, _ptr(out) if want_x else None,
                          _ptr(gmod.weight), _ptr(gmod.bias), _ptr(y), m, hout * wout, cout,
                          gmod.num_groups, float(gmod.eps), int(gsilu), _dt(x), _stream(),
                          book=lambda: ("dd_gn_splitk_kernel", 0.0,
                                        4.0 * split * rows * cout + 2.0 * rows * cout * (2 if want_x else 1)))
            out._gn_cache = (gmod, bool(gsilu), y)
            if not want_x:
                out._unwritten = True          # nobody but that GroupNorm may read it
            return out
    _timer.gemm_launch(L, d, what, "conv", cout, x.numel())
    return out


def vae_posterior(moments, wq, bq, m, h, w, noise=None, scale=1.0, out_f32=False):
    """quant_conv + DiagonalGaussianDistribution of the VAE encoder (dd_vae_posterior): moments (m*h*w, 8) NHWC rows in
    T, wq (8, 8) / bq (8,) fp32, noise (m, 4, h, w) in T or None (mode).  Returns scale * z as (m, 4, h, w), fp32 when
    out_f32 else T."""
    lib = _native.load()
    _need_gpu(moments, wq, bq, noise)
    if moments.shape != (m * h * w, 8) or not moments.is_contiguous():
        raise ValueError("moments must be contiguous (m*h*w, 8), got %s" % (tuple(moments.shape),))
    if wq.dtype != torch.float32 or bq.dtype != torch.float32 or wq.numel() != 64 or bq.numel() != 8 \
            or not wq.is_contiguous() or not bq.is_contiguous():
        raise ValueError("quant_conv weight / bias must be contiguous fp32 (8, 8) / (8,)")
    if noise is not None and (noise.shape != (m, 4, h, w) or noise.dtype != moments.dtype or not noise.is_contiguous()):
        raise ValueError("noise must be a contiguous %s (%d, 4, %d, %d) tensor" % (moments.dtype, m, h, w))
    z = torch.empty((m, 4, h, w), dtype=torch.float32 if out_f32 else moments.dtype, device=moments.device)
    _native.check(lib.dd_vae_posterior(_ptr(moments), _ptr(wq), _ptr(bq), _ptr(noise), _ptr(z), m, h, w, float(scale),
                                       int(bool(out_f32)), _dt(moments), _stream()), "vae_posterior")
    return z


def _image_arg(x, what):
    if x.dim() != 4 or x.shape[1] != 3 or x.numel() == 0:
        raise ValueError("%s takes an (m, 3, h, w) image batch, got %s" % (what, tuple(x.shape)))
    if x.dtype not in _FDT:
        raise ValueError("%s takes fp16 / bf16 / fp32 images, got %s" % (what, x.dtype))
    if not x.is_contiguous():
        raise ValueError("%s takes a contiguous NCHW tensor" % what)
    return x.shape[0], x.shape[2], x.shape[3]


def _image_out(out, shape, device, what):
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=device)
    if out.dtype != torch.uint8 or tuple(out.shape) != tuple(shape) or not out.is_contiguous():
        raise ValueError("%s: out must be a contiguous uint8 %s tensor" % (what, tuple(shape)))
    _written(out)
    return out


def image_padding(padding):
    """torchvision.transforms.Pad's forms -> (left, top, right, bottom): an int (every side), a pair (left / right, top /
    bottom) or the four sides."""
    if isinstance(padding, int) and not isinstance(padding, bool):
        p = (padding,) * 4
    else:
        try:
            p = tuple(padding)
        except TypeError:
            raise ValueError("padding must be an int or a sequence of 2 or 4 ints, got %r" % (padding,))
        if len(p) == 1:
            p = p * 4
        elif len(p) == 2:
            p = (p[0], p[1], p[0], p[1])
    if len(p) != 4 or any(isinstance(v, bool) or not isinstance(v, int) or v < 0 for v in p):
        raise ValueError("padding must be an int or a sequence of 2 or 4 non-negative ints, got %r" % (padding,))
    return p


def image_quantize_u8(x, m11=False, out=None):
    """(m, 3, h, w) images in [0, 1] (fp16 / bf16 / fp32) -> (m, h, w, 3) uint8, `(x.float().numpy() * 255).round()
    .astype("uint8")` of diffusers' numpy_to_pil behind a clamp (dd_image_quantize_u8).  m11: x is a decoder output in
    [-1, 1] and goes through decode_latents' `clamp(x / 2 + 0.5, 0, 1)` first."""
    m, h, w = _image_arg(x, "image_quantize_u8")
    out = _image_out(out, (m, h, w, 3), x.device, "image_quantize_u8")
    _need_gpu(x, out)
    lib = _native.load()
    _timer.launch("image_quantize_u8", lib.dd_image_quantize_u8, _ptr(x), _ptr(out), m, h, w, int(bool(m11)),
                  _FDT[x.dtype], _stream(),
                  book=lambda: ("dd_image_quantize_kernel", 0.0, float(x.numel() * x.element_size() + out.numel())))
    return out


def image_resample_u8(x, size, padding=(0, 0, 0, 0), fill=0, m11=False, out=None):
    """PIL's `Image.resize(size[::-1], BICUBIC)` and torchvision's `Pad(padding, fill)` of the quantised images, byte for
    byte and in one launch (dd_image_resample_u8): x (m, 3, h, w) as image_quantize_u8 takes it, size = (h, w) of the
    resize, padding = (left, top, right, bottom) or Pad's shorter forms -> (m, top + h + bottom, left + w + right, 3)
    uint8.  The coefficient tables (image_tables.device_tables) are device constants under the rule of _consts."""
    m, h, w = _image_arg(x, "image_resample_u8")
    try:
        oh, ow = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError("size must be (h, w), got %r" % (size,))
    if oh <= 0 or ow <= 0:
        raise ValueError("size must be positive, got %r" % (size,))
    pl, pt, pr, pb = image_padding(padding)
    if isinstance(fill, bool) or not isinstance(fill, int) or not 0 <= fill <= 255:
        raise ValueError("fill must be a byte value, got %r" % (fill,))
    out = _image_out(out, (m, pt + oh + pb, pl + ow + pr, 3), x.device, "image_resample_u8")
    _need_gpu(x, out)
    lib = _native.load()
    kx, bx = device_tables(w, ow, x.device)
    ky, by = device_tables(h, oh, x.device)
    _timer.launch("image_resample_u8", lib.dd_image_resample_u8, _ptr(x), _ptr(out), m, h, w, oh, ow, _ptr(kx), _ptr(bx),
                  kx.shape[1], _ptr(ky), _ptr(by), ky.shape[1], pl, pt, pr, pb, fill, int(bool(m11)), _FDT[x.dtype],
                  _stream(),
                  book=lambda: ("dd_image_resample_kernel", 0.0, float(x.numel() * x.element_size() + out.numel())))
    return out


_IMAGE_LAYOUTS = {"nchw": 0, "nhwc8": 1}


def image_load_u8(frames, size, box=None, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), dtype=torch.float32, layout="nchw",
                  out=None):
    """uint8 frames (m, h, w, 3) -> normalised pixel values, the dataset transform `ToTensor` / `Normalize(mean, std)` of
    `pil.resize(size[::-1], BICUBIC).crop(box)` element for element and in one launch (dd_image_load_u8): size = (h, w)
    of the resize, box = PIL's (left, top, right, bottom) inside the resized image (default: all of it), dtype fp16 /
    bf16 / fp32.  layout "nchw" -> (m, 3, bottom - top, right - left); "nhwc8" -> (m * rows * cols, 8) channels-last
    with channels 3..7 zero, what `nchw_to_nhwc(x, 8)` hands to the VAE encoder's conv_in.  Only the crop is computed.
    The coefficient tables and the normalisation table (image_tables) are device constants under the rule of _consts."""
    what = "image_load_u8"
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.numel() == 0:
        raise ValueError("%s takes an (m, h, w, 3) frame batch, got %s" % (what, tuple(frames.shape)))
    if frames.dtype != torch.uint8:
        raise ValueError("%s takes uint8 frames, got %s" % (what, frames.dtype))
    if not frames.is_contiguous():
        raise ValueError("%s takes a contiguous NHWC tensor" % what)
    m, h, w = frames.shape[0], frames.shape[1], frames.shape[2]
    try:
        nh, nw = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError("size must be (h, w), got %r" % (size,))
    if nh <= 0 or nw <= 0:
        raise ValueError("size must be positive, got %r" % (size,))
    if box is None:
        box = (0, 0, nw, nh)
    try:
        left, top, right, bottom = (int(v) for v in box)
    except (TypeError, ValueError):
        raise ValueError("box must be (left, top, right, bottom), got %r" % (box,))
    if not (0 <= left < right <= nw and 0 <= top < bottom <= nh):
        raise ValueError("box %r is empty or leaves the %d x %d (w x h) resized image" % (tuple(box), nw, nh))
    if layout not in _IMAGE_LAYOUTS:
        raise ValueError("layout must be one of %s, got %r" % (", ".join(sorted(_IMAGE_LAYOUTS)), layout))
    if dtype not in _FDT:
        raise ValueError("%s writes fp16 / bf16 / fp32, got %s" % (what, dtype))
    mean, std = _image_mean_std(mean, std)
    oh, ow = bottom - top, right - left
    shape = (m, 3, oh, ow) if layout == "nchw" else (m * oh * ow, 8)
    if out is None:
        _need_gpu(frames)
        out = torch.empty(shape, dtype=dtype, device=frames.device)
    elif out.dtype != dtype or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError("%s: out must be a contiguous %s %s tensor" % (what, dtype, shape))
    else:
        _written(out)
    _need_gpu(frames, out)
    _forget_derived(out)
    lib = _native.load()
    kx, bx = device_tables(w, nw, frames.device)
    ky, by = device_tables(h, nh, frames.device)
    lut = _image_lut(mean, std, frames.device)
    _timer.launch(what, lib.dd_image_load_u8, _ptr(frames), _ptr(out), m, h, w, oh, ow, _ptr(kx[left:]), _ptr(bx[left:]),
                  kx.shape[1], _ptr(ky[top:]), _ptr(by[top:]), ky.shape[1], _ptr(lut), _FDT[dtype],
                  _IMAGE_LAYOUTS[layout], _stream(),
                  book=lambda: ("dd_image_load_kernel", 0.0, float(frames.numel() + out.numel() * out.element_size())))
    return out


def jpeg_encode_u8(frames, quality=75, out=None, capacity=None):
    """uint8 frames (m, H, W, 3) -> the files PIL's `Image.save(name.jpg, quality=quality)` writes, byte for byte
    (dd_jpeg_encode_u8): baseline, 4:2:0 chroma, the standard Huffman tables.  -> (buf (m, capacity) uint8, lengths (m,)
    int32), both on the device: file i is buf[i, :lengths[i]].  capacity defaults to header + H * W bytes per frame (at least the header and the end marker); a
    length above the capacity is the file's true length, the row then holds its first `capacity` bytes.  Nothing is read
    back.  The header and the tables (image_tables.device_jpeg_tables) are device constants under the rule of _consts;
    the scratch buffer is ops.workspace's: call once, on the capture stream or under the same workspace_owner, before
    capturing the launches in a graph."""
    what = "jpeg_encode_u8"
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.numel() == 0:
        raise ValueError("%s takes an (m, H, W, 3) frame batch, got %s" % (what, tuple(frames.shape)))
    if frames.dtype != torch.uint8:
        raise ValueError("%s takes uint8 frames, got %s" % (what, frames.dtype))
    if not frames.is_contiguous():
        raise ValueError("%s takes a contiguous NHWC tensor" % what)
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError("quality must be an int in 1..100, got %r" % (quality,))
    m, h, w = frames.shape[0], frames.shape[1], frames.shape[2]
    if h > 65535 or w > 65535:
        raise ValueError("%s: a JPEG frame is at most 65535 x 65535, got %d x %d" % (what, h, w))
    header_len = len(jpeg_header(h, w, quality))
    if out is not None:
        if out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] != m or not out.is_contiguous():
            raise ValueError("%s: out must be a contiguous uint8 (%d, capacity) tensor" % (what, m))
        if capacity is not None and int(capacity) != out.shape[1]:
            raise ValueError("%s: capacity %r does not match out %s" % (what, capacity, tuple(out.shape)))
        capacity = out.shape[1]
        _written(out)
    capacity = header_len + max(h * w, 2) if capacity is None else int(capacity)        # 1 x 1: room for the end marker
    if capacity < header_len + 2:
        raise ValueError("%s: capacity must be at least the header and the end marker (%d bytes), got %d"
                         % (what, header_len + 2, capacity))
    _need_gpu(frames, out)
    if out is None:
        out = torch.empty((m, capacity), dtype=torch.uint8, device=frames.device)
    lengths = torch.empty((m,), dtype=torch.int32, device=frames.device)
    lib = _native.load()
    need = lib.dd_jpeg_workspace_bytes(m, h, w)
    if need < 0:
        raise _native.Unsupported("dualdiff_amd.%s: %d frames of %d x %d are more than one call takes" % (what, m, h, w))
    header, tables = device_jpeg_tables(h, w, quality, frames.device)
    ws = workspace(need, frames.device, kind="jpeg")
    _timer.launch(what, lib.dd_jpeg_encode_u8, _ptr(frames), m, h, w, _ptr(header), header_len, _ptr(tables), _ptr(ws),
                  ws.numel() * 4, _ptr(out), capacity, _ptr(lengths), _stream(),
                  # frames read, the int16 coefficients (768 bytes per MCU) written once and read twice; the bit stream is as
                  # long as the content makes it and is not booked
                  book=lambda: ("dd_jpeg_encode", 0.0, float(frames.numel() + 3 * 768 * m * ((h + 15) // 16) * ((w + 15) // 16))))
    return out, lengths


def png_encode_u8(frames, out=None, capacity=None):
    """uint8 frames (m, H, W, 3) -> one lossless .png file per frame (dd_png_encode_u8): 8-bit RGB, per-row filter choice,
    one dynamic-Huffman or stored deflate block and one IDAT per 16 KiB of filtered bytes.  -> (buf (m,
    capacity) uint8, lengths (m,) int32), both on the device: file i is buf[i, :lengths[i]].  capacity defaults to
    image_tables.png_capacity(H, W), the file with every chunk stored, which no content exceeds; with a smaller one a
    length above the capacity is the file's true length and the row then holds its first `capacity` bytes.  Nothing is read
    back and no table comes from the host.  The scratch buffer is ops.workspace's: call once, on the capture stream or
    under the same workspace_owner, before capturing the launches in a graph."""
    return _png_encode("png_encode_u8", (3,), frames, out, capacity)


def png_encode_u8c(frames, out=None, capacity=None):
    """png_encode_u8 for uint8 frames of 3 or 4 channels, (m, H, W, 3) or (m, H, W, 4) (dd_png_encode_u8c): the same format
    with colour type 6 and four bytes per pixel in the filters for RGBA; capacity defaults to
    image_tables.png_capacity(H, W, channels).  RGB frames give png_encode_u8's bytes."""
    return _png_encode("png_encode_u8c", (3, 4), frames, out, capacity)


def _png_encode(what, channels, frames, out, capacity):
    """The two wrappers above: `channels` is what the last dimension may be.  png_encode_u8 stays on the entry points it
    has always used, png_encode_u8c goes through the ones that take the channel count."""
    if frames.dim() != 4 or frames.shape[3] not in channels or frames.numel() == 0:
        raise ValueError("%s takes an (m, H, W, %s) frame batch, got %s" % (what, " or ".join(map(str, channels)), tuple(frames.shape)))
    if frames.dtype != torch.uint8:
        raise ValueError("%s takes uint8 frames, got %s" % (what, frames.dtype))
    if not frames.is_contiguous():
        raise ValueError("%s takes a contiguous NHWC tensor" % what)
    m, h, w, ch = frames.shape
    if out is not None:
        if out.dtype != torch.uint8 or out.dim() != 2 or out.shape[0] != m or not out.is_contiguous():
            raise ValueError("%s: out must be a contiguous uint8 (%d, capacity) tensor" % (what, m))
        if capacity is not None and int(capacity) != out.shape[1]:
            raise ValueError("%s: capacity %r does not match out %s" % (what, capacity, tuple(out.shape)))
        capacity = out.shape[1]
        _written(out)
    capacity = png_capacity(h, w, ch) if capacity is None else int(capacity)
    if capacity < PNG_FILE_FIXED:
        raise ValueError("%s: capacity must be at least the fixed parts of a file (%d bytes), got %d"
                         % (what, PNG_FILE_FIXED, capacity))
    _need_gpu(frames, out)
    lib = _native.load()
    generic = channels != (3,)
    need = lib.dd_png_workspace_bytes_c(m, h, w, ch) if generic else lib.dd_png_workspace_bytes(m, h, w)
    if need < 0:
        raise _native.Unsupported("dualdiff_amd.%s: %d frames of %d x %d are more than one call takes" % (what, m, h, w))
    if out is None:
        out = torch.empty((m, capacity), dtype=torch.uint8, device=frames.device)
    lengths = torch.empty((m,), dtype=torch.int32, device=frames.device)
    ws = workspace(need, frames.device, kind="png")
    head = (_ptr(frames), m, h, w) + ((ch,) if generic else ())
    _timer.launch(what, lib.dd_png_encode_u8c if generic else lib.dd_png_encode_u8, *head, _ptr(ws), ws.numel() * 4,
                  _ptr(out), capacity, _ptr(lengths), _stream(),
                  # frames read twice by the filter, the filtered bytes written once and read once; the chunks' deflate
                  # forms are as long as the content makes them and are not booked
                  book=lambda: ("dd_png_encode", 0.0, float(2 * frames.numel() + 2 * m * h * (1 + ch * w))))
    return out, lengths


JPEG_DECODE_TABLE_BYTES = 4016      # the table block of one frame (csrc/jpeg_decode_core.h: DdJdTables)
JPEG_DECODE_SAMPLINGS = (420, 444)
JPEG_DECODE_STATUS = ((1, "the stream is exhausted before the last block"), (2, "an invalid Huffman code"),
                      (4, "a zero run past coefficient 63"), (8, "bytes left behind the last block"))


def jpeg_decode_u8(scan, offsets, lengths, tables, h, w, sampling, max_scan_bytes, rounds=None, out=None):
    """The entropy-coded segments of m baseline JPEG files of one geometry -> (frames (m, h, w, 3) uint8, status (m,)
    int32), both on the device, the frames byte for byte PIL's `Image.open(f).convert("RGB")` (dd_jpeg_decode_u8).
    scan: uint8 (n,), the segments still byte-stuffed, frame i at scan[offsets[i] : offsets[i] + lengths[i]] at any byte
    alignment; offsets, lengths: int32 (m,); tables: uint8 (m, 4016), one block per frame
    (pipeline/jpeg_input.py: table_block) — all device tensors, usually views of one upload.  sampling: 420 or 444;
    max_scan_bytes: at least every length (the host knows them; nothing is read back).  status[i] is 0 or an OR of
    JPEG_DECODE_STATUS's bits; a bad frame leaves the others alone.  rounds: None for the library's default; the frames
    do not depend on it.  The scratch buffer is ops.workspace's: call once before capturing the launches in a graph."""
    what = "jpeg_decode_u8"
    if scan.dtype != torch.uint8 or scan.dim() != 1 or scan.numel() == 0 or not scan.is_contiguous():
        raise ValueError("%s takes the scan bytes as a contiguous uint8 (n,) tensor, got %s %s" % (what, tuple(scan.shape), scan.dtype))
    m = offsets.numel()
    for name, t in (("offsets", offsets), ("lengths", lengths)):
        if t.dtype != torch.int32 or t.dim() != 1 or t.numel() != m or m == 0 or not t.is_contiguous():
            raise ValueError("%s: %s must be a contiguous int32 (m,) tensor, got %s %s" % (what, name, tuple(t.shape), t.dtype))
    if tables.dtype != torch.uint8 or tuple(tables.shape) != (m, JPEG_DECODE_TABLE_BYTES) or not tables.is_contiguous():
        raise ValueError("%s: tables must be a contiguous uint8 (%d, %d) tensor, got %s %s"
                         % (what, m, JPEG_DECODE_TABLE_BYTES, tuple(tables.shape), tables.dtype))
    ints = (h, w, sampling, max_scan_bytes) + (() if rounds is None else (rounds,))
    if any(isinstance(v, bool) or not isinstance(v, int) for v in ints):
        raise ValueError("%s: h, w, sampling, max_scan_bytes and rounds are ints" % what)
    if not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError("%s: a JPEG frame is 1 x 1 to 65535 x 65535, got %d x %d" % (what, h, w))
    if sampling not in JPEG_DECODE_SAMPLINGS:
        raise ValueError("%s: sampling must be one of %s, got %r" % (what, JPEG_DECODE_SAMPLINGS, sampling))
    if max_scan_bytes <= 0:
        raise ValueError("%s: max_scan_bytes must be positive, got %d" % (what, max_scan_bytes))
    if rounds is not None and not 0 <= rounds <= 64:
        raise ValueError("%s: rounds must be in 0..64, got %d" % (what, rounds))
    out = _image_out(out, (m, h, w, 3), scan.device, what)
    _need_gpu(scan, offsets, lengths, tables, out)
    if tables.data_ptr() % 4 or offsets.data_ptr() % 4 or lengths.data_ptr() % 4:
        raise ValueError("%s: tables, offsets and lengths must start on a 4-byte boundary" % what)
    status = torch.empty((m,), dtype=torch.int32, device=scan.device)
    lib = _native.load()
    need = lib.dd_jpeg_decode_workspace_bytes(m, h, w, sampling, max_scan_bytes)
    if need < 0:
        raise _native.Unsupported("dualdiff_amd.%s: %d frames of %d x %d with segments of %d bytes are more than one call takes"
                                  % (what, m, h, w, max_scan_bytes))
    ws = workspace(need, scan.device, kind="jpeg_decode")
    _timer.launch(what, lib.dd_jpeg_decode_u8, _ptr(scan), scan.numel(), _ptr(offsets), _ptr(lengths), max_scan_bytes,
                  _ptr(tables), m, h, w, sampling, _ptr(out), _ptr(status), _ptr(ws), ws.numel() * 4,
                  -1 if rounds is None else rounds, _stream(),
                  # the segments read twice and written once without stuffing, the frames written; the decode passes read what
                  # the content makes them read and are not booked
                  book=lambda: ("dd_jpeg_decode", 0.0, float(3 * scan.numel() + out.numel())))
    return out, status


PNG_DECODE_COLOUR_TYPES = (0, 2, 6)  # grey, RGB, RGBA at bit depth 8
PNG_DECODE_CHUNK = 16384            # filtered bytes per IDAT of png_encode_u8's own files (csrc/png.hip)
PNG_DECODE_STATUS = ((1, "the stream ends inside a block or before the Adler-32"), (2, "a reserved block type"),
                     (4, "a stored block whose LEN is not the complement of NLEN"), (8, "bad code lengths"),
                     (16, "an invalid symbol"), (32, "a distance before the start of the output"),
                     (64, "more bytes than the frame"), (128, "fewer bytes than the frame"), (256, "the Adler-32 does not match"),
                     (512, "a bad zlib header"), (1024, "a bad filter type"))


def png_decode_u8(streams, files, tab, colour_types, h, w, chunked=None, out=None):
    """The concatenated IDAT payloads of m .png files of one geometry -> (frames (m, h, w, 3) uint8, status (m,) int32,
    paths (m,) int32), all on the device, the frames byte for byte PIL's `Image.open(f).convert("RGB")`
    (dd_png_decode_u8).  streams: uint8 (n,); files: int32 (m, 4), per file the stream's offset and length, the colour
    type and the index in `tab` of its IDAT boundaries or -1; tab: int32 (k,) or None — device tensors, usually views of
    one upload (pipeline/png_input.py: upload_png).  colour_types: the m colour types as Python ints (the host knows them;
    nothing is read back).  chunked: None to decode the files whose entry names a place in `tab` chunk by chunk where
    the device can verify that this is the sequential decode, False to send every file through the sequential path; the
    frames do not depend on it.  status[i] is 0 or one of PNG_DECODE_STATUS's bits; a bad frame leaves the others alone.
    paths[i] is 1 where the chunk-parallel result was used.  The scratch buffer is ops.workspace's: call once before
    capturing the launches in a graph."""
    what = "png_decode_u8"
    if streams.dtype != torch.uint8 or streams.dim() != 1 or streams.numel() == 0 or not streams.is_contiguous():
        raise ValueError("%s takes the streams as a contiguous uint8 (n,) tensor, got %s %s" % (what, tuple(streams.shape), streams.dtype))
    if files.dtype != torch.int32 or files.dim() != 2 or files.shape[1] != 4 or files.shape[0] == 0 or not files.is_contiguous():
        raise ValueError("%s: files must be a contiguous int32 (m, 4) tensor, got %s %s" % (what, tuple(files.shape), files.dtype))
    m = files.shape[0]
    if tab is not None and (tab.dtype != torch.int32 or tab.dim() != 1 or not tab.is_contiguous()):
        raise ValueError("%s: tab must be a contiguous int32 (k,) tensor or None, got %s %s" % (what, tuple(tab.shape), tab.dtype))
    if any(isinstance(v, bool) or not isinstance(v, int) for v in (h, w)):
        raise ValueError("%s: h and w are ints" % what)
    if h <= 0 or w <= 0:
        raise ValueError("%s: a frame is at least 1 x 1, got %d x %d" % (what, h, w))
    colour_types = [int(c) for c in colour_types]
    if len(colour_types) != m or any(c not in PNG_DECODE_COLOUR_TYPES for c in colour_types):
        raise ValueError("%s: colour_types must be %d of %s, got %r" % (what, m, PNG_DECODE_COLOUR_TYPES, colour_types))
    if chunked not in (None, False):
        raise ValueError("%s: chunked is None (verify and use the chunks) or False (the sequential path), got %r" % (what, chunked))
    out = _image_out(out, (m, h, w, 3), streams.device, what)
    _need_gpu(streams, files, tab, out)
    if files.data_ptr() % 4 or (tab is not None and tab.data_ptr() % 4):
        raise ValueError("%s: files and tab must start on a 4-byte boundary" % what)
    status = torch.empty((m,), dtype=torch.int32, device=streams.device)
    paths = torch.empty((m,), dtype=torch.int32, device=streams.device)
    lib = _native.load()
    need = lib.dd_png_decode_workspace_bytes(m, h, w)
    if need < 0:
        raise _native.Unsupported("dualdiff_amd.%s: %d frames of %d x %d are more than one call takes" % (what, m, h, w))
    ws = workspace(need, streams.device, kind="png_decode")
    ntab = 0 if tab is None else tab.numel()
    types = (ctypes.c_int32 * m)(*colour_types)
    _timer.launch(what, lib.dd_png_decode_u8, _ptr(streams), streams.numel(), _ptr(files), _ptr(tab) if ntab else None, ntab,
                  types, m, h, w, 1 if chunked is None else 0, _ptr(out), _ptr(status), _ptr(paths), _ptr(ws),
                  ws.numel() * 4, _stream(),
                  # the streams read once; the filtered bytes written, summed, unfiltered in place and read once more; the
                  # frames written
                  book=lambda: ("dd_png_decode", 0.0, float(streams.numel() + 5 * m * h * (1 + 4 * w) + out.numel())))
    return out, status, paths


def png_condition(frames, views=6, top=0, left=0, size=None, out=None):
    """uint8 frames (b, H, W, 3), each a panorama of `views` views side by side -> float32 (b, 3, oh, views * ow), NCHW:
    `ToTensor()` of rows top .. top + oh and, per view, columns left .. left + ow (dd_png_condition; dataset/utils.py:
    348-408).  size: (oh, ow), None for the rest of the view.  The value of a byte is float32(byte) / 255 from a table
    built on the host (image_tables.png_unit_lut), a device constant under the rule of _consts."""
    what = "png_condition"
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.numel() == 0:
        raise ValueError("%s takes a (b, H, W, 3) frame batch, got %s" % (what, tuple(frames.shape)))
    if frames.dtype != torch.uint8:
        raise ValueError("%s takes uint8 frames, got %s" % (what, frames.dtype))
    if not frames.is_contiguous():
        raise ValueError("%s takes a contiguous NHWC tensor" % what)
    b, h, w = frames.shape[0], frames.shape[1], frames.shape[2]
    if any(isinstance(v, bool) or not isinstance(v, int) for v in (views, top, left)) or views <= 0 or w % views:
        raise ValueError("%s: views must be a positive int that divides the width %d, top and left ints; got %r, %r, %r"
                         % (what, w, views, top, left))
    pw = w // views
    try:
        oh, ow = (h - top, pw - left) if size is None else (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError("size must be (h, w), got %r" % (size,))
    if not (0 <= top and 0 <= left and 0 < oh and 0 < ow and top + oh <= h and left + ow <= pw):
        raise ValueError("%s: the crop top %d, left %d, size %d x %d leaves the %d x %d view" % (what, top, left, oh, ow, h, pw))
    shape = (b, 3, oh, views * ow)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=frames.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError("%s: out must be a contiguous float32 %s tensor" % (what, shape))
    else:
        _written(out)
    _need_gpu(frames, out)
    _forget_derived(out)
    lib = _native.load()
    lut = device_const("png_unit_lut", frames.device, png_unit_lut)
    _timer.launch(what, lib.dd_png_condition, _ptr(frames), _ptr(out), _ptr(lut), b, h, w, views, top, left, oh, ow, _stream(),
                  book=lambda: ("dd_png_condition_kernel", 0.0, float(out.numel() * 5)))
    return out


def png_condition_resized(frames, views=6, pad_top=0, resize=None, top=0, left=0, size=None, out=None):
    """png_condition with `crop_drivewm`'s pad and resize in front of the crop (dd_png_condition_resize; dataset/utils.py:
    355-358, 374-388): every view of the uint8 frames (b, H, W, 3) gets `pad_top` zero rows on top, is resized to resize =
    (rh, rw) as `F.interpolate(mode="bilinear", align_corners=False)` resizes it, without antialias and per view, and is
    cropped to rows top .. top + oh, columns left .. left + ow of the RESIZED view -> float32 (b, 3, oh, views * ow).
    resize: None keeps (H + pad_top, W / views), and that size gives png_condition's bits.  size: (oh, ow), None for the
    rest of the resized view.  The taps and weights of both axes are built on the host in float32
    (image_tables.bilinear_tables) and are device constants under the rule of _consts, as the byte / 255 table is."""
    what = "png_condition_resized"
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.numel() == 0:
        raise ValueError("%s takes a (b, H, W, 3) frame batch, got %s" % (what, tuple(frames.shape)))
    if frames.dtype != torch.uint8:
        raise ValueError("%s takes uint8 frames, got %s" % (what, frames.dtype))
    if not frames.is_contiguous():
        raise ValueError("%s takes a contiguous NHWC tensor" % what)
    b, h, w = frames.shape[0], frames.shape[1], frames.shape[2]
    if any(isinstance(v, bool) or not isinstance(v, int) for v in (views, pad_top, top, left)) or views <= 0 or w % views:
        raise ValueError("%s: views must be a positive int that divides the width %d, pad_top, top and left ints; got %r, %r, "
                         "%r, %r" % (what, w, views, pad_top, top, left))
    if pad_top < 0:
        raise ValueError("%s: pad_top must not be negative, got %d" % (what, pad_top))
    pw = w // views
    try:
        rh, rw = (h + pad_top, pw) if resize is None else (int(v) for v in resize)
    except (TypeError, ValueError):
        raise ValueError("resize must be (h, w), got %r" % (resize,))
    if not (0 < rh <= BILINEAR_MAX and 0 < rw <= BILINEAR_MAX and h + pad_top <= BILINEAR_MAX and pw <= BILINEAR_MAX):
        raise ValueError("%s: a view of %d x %d resized to %d x %d: sizes are 1..%d" % (what, h + pad_top, pw, rh, rw, BILINEAR_MAX))
    try:
        oh, ow = (rh - top, rw - left) if size is None else (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError("size must be (h, w), got %r" % (size,))
    if not (0 <= top and 0 <= left and 0 < oh and 0 < ow and top + oh <= rh and left + ow <= rw):
        raise ValueError("%s: the crop top %d, left %d, size %d x %d leaves the resized %d x %d view" % (what, top, left, oh, ow, rh, rw))
    shape = (b, 3, oh, views * ow)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=frames.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous():
        raise ValueError("%s: out must be a contiguous float32 %s tensor" % (what, shape))
    else:
        _written(out)
    _need_gpu(frames, out)
    if out.data_ptr() % 16:
        raise ValueError("%s: out must start on a 16-byte boundary" % what)
    _forget_derived(out)
    lib = _native.load()
    lut = device_const("png_unit_lut", frames.device, png_unit_lut)
    row_taps, row_weights = device_bilinear_tables(h + pad_top, rh, frames.device)
    col_taps, col_weights = device_bilinear_tables(pw, rw, frames.device)
    _timer.launch(what, lib.dd_png_condition_resize, _ptr(frames), _ptr(out), _ptr(lut), _ptr(row_taps), _ptr(row_weights),
                  _ptr(col_taps), _ptr(col_weights), b, h, w, views, pad_top, rh, rw, top, left, oh, ow, _stream(),
                  # four bytes read per float written; they share cache lines
                  book=lambda: ("dd_png_condition_resize_kernel", 0.0, float(out.numel() * 4 + frames.numel())))
    return out


BOX_POINT_MODES = {"all-xyz": 0, "cxyz": 1}     # dataset/utils.py:222-226; points per box 8 / 4
BOX_FILTERS = {"all": 0, "positive_z": 1, "canvas": 2}


def box_views(corners, labels, offsets, transforms, views, cap, points_mode="all-xyz", filter_mode="positive_z",
              canvas_size=None, filter_corners=None, out=None):
    """Every scene's box corners -> the per-view `bboxes_3d_data` at a capacity of `cap` slots, in one launch
    (include/dualdiff_hip.h: dd_box_views; dataset/utils.py:128-262).  corners (total, 8, 3) fp32, labels (total,) int64,
    offsets (scenes + 1,) int32, transforms (scenes, views, 4, 4) fp32 or None for filter "all", filter_corners as
    corners or None — all contiguous device tensors.  canvas_size = (h, w) for filter "canvas".
    -> (bboxes (scenes, views, cap, P, 3) fp32, classes (scenes, views, cap) int64, masks (..., cap) bool, counts (scenes,
    views) int32, max_len (1,) int32); out = the same five tensors of the caller's (e.g. the second half of a zeroed CFG
    batch).  Nothing is read back: counts and max_len stay in device memory."""
    what = "box_views"
    if points_mode not in BOX_POINT_MODES:
        raise ValueError("%s: points_mode must be one of %s, got %r" % (what, ", ".join(sorted(BOX_POINT_MODES)), points_mode))
    if filter_mode not in BOX_FILTERS:
        raise ValueError("%s: filter_mode must be one of %s, got %r" % (what, ", ".join(sorted(BOX_FILTERS)), filter_mode))
    if corners.dim() != 3 or tuple(corners.shape[1:]) != (8, 3) or corners.dtype != torch.float32:
        raise ValueError("%s takes fp32 corners (total, 8, 3), got %s %s" % (what, corners.dtype, tuple(corners.shape)))
    total = corners.shape[0]
    if labels.dtype != torch.int64 or tuple(labels.shape) != (total,):
        raise ValueError("%s takes int64 labels (%d,), got %s %s" % (what, total, labels.dtype, tuple(labels.shape)))
    if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.shape[0] < 2:
        raise ValueError("%s takes int32 offsets (scenes + 1,), got %s %s" % (what, offsets.dtype, tuple(offsets.shape)))
    scenes, views, cap = offsets.shape[0] - 1, int(views), int(cap)
    if views <= 0 or cap <= 0:
        raise ValueError("%s: views and cap must be positive, got %d and %d" % (what, views, cap))
    fm = BOX_FILTERS[filter_mode]
    if fm == 0 and views != 1:
        raise ValueError("%s: filter \"all\" is the view-shared form and has one view, got %d" % (what, views))
    if fm != 0 and (transforms is None or transforms.dtype != torch.float32
                    or tuple(transforms.shape) != (scenes, views, 4, 4)):
        raise ValueError("%s: filter %r takes fp32 transforms (%d, %d, 4, 4)" % (what, filter_mode, scenes, views))
    ch = cw = 0
    if fm == 2:
        try:
            ch, cw = (int(v) for v in canvas_size)
        except (TypeError, ValueError):
            raise ValueError("%s: filter \"canvas\" takes canvas_size = (h, w), got %r" % (what, canvas_size))
        if ch <= 0 or cw <= 0:
            raise ValueError("%s: canvas_size must be positive, got %r" % (what, canvas_size))
    if filter_corners is not None and (filter_corners.dtype != torch.float32 or filter_corners.shape != corners.shape):
        raise ValueError("%s: filter_corners must match corners" % what)
    ins = (corners, labels, offsets, transforms, filter_corners)
    if any(t is not None and not t.is_contiguous() for t in ins):
        raise ValueError("%s takes contiguous tensors" % what)
    _need_gpu(*ins)
    pts = 8 if BOX_POINT_MODES[points_mode] == 0 else 4
    shapes = ((scenes, views, cap, pts, 3), (scenes, views, cap), (scenes, views, cap), (scenes, views), (1,))
    dtypes = (torch.float32, torch.int64, torch.bool, torch.int32, torch.int32)
    if out is None:
        out = tuple(torch.empty(s, dtype=d, device=corners.device) for s, d in zip(shapes, dtypes))
    else:
        out = tuple(out)
        if len(out) != 5 or any(tuple(t.shape) != s or t.dtype != d or not t.is_contiguous()
                                for t, s, d in zip(out, shapes, dtypes)):
            raise ValueError("%s: out must be contiguous tensors of %s" % (what, list(zip(shapes, dtypes))))
        _need_gpu(*out)
        _written(*out)
    lib = _native.load()
    _timer.launch(what, lib.dd_box_views, _ptr(corners), _ptr(filter_corners), _ptr(labels), _ptr(offsets),
                  _ptr(transforms) if fm != 0 else None, total, scenes, views, cap, BOX_POINT_MODES[points_mode], fm, ch, cw,
                  *(_ptr(t) for t in out), _stream(),
                  book=lambda: ("dd_box_views_kernel", 0.0,
                                float((1 if fm == 0 else views) * total * 96 + out[0].numel() * 4 + out[1].numel() * 9)))
    return out


BOX_EDGES_MAX = 1024                             # include/dualdiff_hip.h: DD_BOX_EDGES_MAX, the boxes of one scene
BOX_FLAGS = ((1, "a label outside [-n_classes, n_classes): that box is not drawn"),
             (2, "a projected coordinate beyond +-2^29, saturated there"),
             (4, "a view drew more boxes than cap, or a scene holds more than %d" % BOX_EDGES_MAX))


def box_edges(corners, labels, offsets, transforms, cap, n_classes):
    """Every scene's box corners -> per (scene, view) the integer end points of the boxes drawn in that view, in draw
    order, in one launch (include/dualdiff_hip.h: dd_box_edges; runner/box_visualizer.py:89-114).  corners (total, 8, 3)
    fp32 (the re-centred ones), labels (total,) int64, offsets (scenes + 1,) int32, transforms (scenes, views, 4, 4) fp32
    — contiguous device tensors.  cap: slots per (scene, view), at most BOX_EDGES_MAX.
    -> (pts (scenes, views, cap, 8, 2) int32, cls (scenes, views, cap) int32, counts (scenes, views) int32, flags (1,)
    int32: an OR of BOX_FLAGS' bits).  Nothing is read back."""
    what = "box_edges"
    if corners.dim() != 3 or tuple(corners.shape[1:]) != (8, 3) or corners.dtype != torch.float32:
        raise ValueError("%s takes fp32 corners (total, 8, 3), got %s %s" % (what, corners.dtype, tuple(corners.shape)))
    total = corners.shape[0]
    if labels.dtype != torch.int64 or tuple(labels.shape) != (total,):
        raise ValueError("%s takes int64 labels (%d,), got %s %s" % (what, total, labels.dtype, tuple(labels.shape)))
    if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.shape[0] < 2:
        raise ValueError("%s takes int32 offsets (scenes + 1,), got %s %s" % (what, offsets.dtype, tuple(offsets.shape)))
    scenes = offsets.shape[0] - 1
    if transforms.dtype != torch.float32 or transforms.dim() != 4 or transforms.shape[1] == 0 \
            or (transforms.shape[0],) + tuple(transforms.shape[2:]) != (scenes, 4, 4):
        raise ValueError("%s takes fp32 transforms (%d, views, 4, 4), got %s %s"
                         % (what, scenes, transforms.dtype, tuple(transforms.shape)))
    views, cap, n_classes = transforms.shape[1], int(cap), int(n_classes)
    if cap <= 0 or n_classes <= 0:
        raise ValueError("%s: cap and n_classes must be positive, got %d and %d" % (what, cap, n_classes))
    if cap > BOX_EDGES_MAX:
        raise _native.Unsupported("dualdiff_amd.%s: a scene holds at most %d boxes, got cap = %d" % (what, BOX_EDGES_MAX, cap))
    ins = (corners, labels, offsets, transforms)
    if any(not t.is_contiguous() for t in ins):
        raise ValueError("%s takes contiguous tensors" % what)
    _need_gpu(*ins)
    dev = corners.device
    pts = torch.empty((scenes, views, cap, 8, 2), dtype=torch.int32, device=dev)
    cls = torch.empty((scenes, views, cap), dtype=torch.int32, device=dev)
    counts = torch.empty((scenes, views), dtype=torch.int32, device=dev)
    flags = torch.empty((1,), dtype=torch.int32, device=dev)
    lib = _native.load()
    _timer.launch(what, lib.dd_box_edges, _ptr(corners), _ptr(labels), _ptr(offsets), _ptr(transforms), total, scenes,
                  views, cap, n_classes, _ptr(pts), _ptr(cls), _ptr(counts), _ptr(flags), _stream(),
                  book=lambda: ("dd_box_edges_kernel", 0.0, float(2 * views * total * 104 + pts.numel() * 4 + cls.numel() * 4)))
    return pts, cls, counts, flags


def box_draw_u8(frames, pts, cls, counts, palette, transparent=False, size=None):
    """The boxes of box_edges drawn over uint8 frames, or alone on a transparent canvas, in one launch (include/
    dualdiff_hip.h: dd_box_draw_u8): every box's 12 edges as PIL's thin line, the last box of a row on top.  frames (m,
    H, W, 3) uint8, m = scenes * views, or None with transparent=True and size=(H, W); pts (m, cap, 8, 2) int32 (or
    (scenes, views, cap, 8, 2)), cls (m, cap) int32, counts (m,) int32; palette (n, 3) uint8: RGB per class — contiguous
    device tensors.  -> (m, H, W, 3) uint8, a new tensor (the frames are not written), or (m, H, W, 4) RGBA with
    transparent=True: A = 255 where a line of a colour other than black lies."""
    what = "box_draw_u8"
    if pts.dtype != torch.int32 or pts.dim() not in (4, 5) or tuple(pts.shape[-2:]) != (8, 2) or pts.numel() == 0:
        raise ValueError("%s takes int32 pts (m, cap, 8, 2), got %s %s" % (what, pts.dtype, tuple(pts.shape)))
    cap = pts.shape[-3]
    m = pts.numel() // (cap * 16)
    if cls.dtype != torch.int32 or cls.numel() != m * cap or counts.dtype != torch.int32 or counts.numel() != m:
        raise ValueError("%s takes int32 cls (%d, %d) and counts (%d,), got %s %s and %s %s"
                         % (what, m, cap, m, cls.dtype, tuple(cls.shape), counts.dtype, tuple(counts.shape)))
    if palette.dtype != torch.uint8 or palette.dim() != 2 or palette.shape[1] != 3 or palette.shape[0] == 0:
        raise ValueError("%s takes a uint8 palette (n, 3), got %s %s" % (what, palette.dtype, tuple(palette.shape)))
    transparent = bool(transparent)
    if frames is None:
        if not transparent:
            raise ValueError("%s: frames may be None with transparent=True only" % what)
        try:
            h, w = (int(v) for v in size)
        except (TypeError, ValueError):
            raise ValueError("%s: without frames pass size=(H, W), got %r" % (what, size))
        if h <= 0 or w <= 0:
            raise ValueError("%s: size must be positive, got %r" % (what, size))
    else:
        if frames.dim() != 4 or frames.shape[3] != 3 or frames.numel() == 0 or frames.dtype != torch.uint8:
            raise ValueError("%s takes uint8 frames (m, H, W, 3), got %s %s" % (what, frames.dtype, tuple(frames.shape)))
        if frames.shape[0] != m:
            raise ValueError("%s: %d frames for %d rows of boxes" % (what, frames.shape[0], m))
        h, w = frames.shape[1], frames.shape[2]
        if size is not None and tuple(int(v) for v in size) != (h, w):
            raise ValueError("%s: size %r does not match the frames' %d x %d" % (what, size, h, w))
    ins = (frames, pts, cls, counts, palette)
    if any(t is not None and not t.is_contiguous() for t in ins):
        raise ValueError("%s takes contiguous tensors" % what)
    _need_gpu(*ins)
    if h >= 1 << 15 or w >= 1 << 15 or m > 65535:
        raise _native.Unsupported("dualdiff_amd.%s: %d frames of %d x %d are more than one call takes" % (what, m, h, w))
    out = torch.empty((m, h, w, 4 if transparent else 3), dtype=torch.uint8, device=pts.device)
    lib = _native.load()
    _timer.launch(what, lib.dd_box_draw_u8, _ptr(None if transparent else frames), _ptr(pts), _ptr(cls), _ptr(counts),
                  _ptr(palette), _ptr(out), m, cap, h, w, palette.shape[0], 1 if transparent else 0, _stream(),
                  book=lambda: ("dd_box_draw_kernel", 0.0, float(out.numel() + (0 if transparent else out.numel()))))
    return out


BEV_MAP_MAX_LAYERS = 30                          # include/dualdiff_hip.h: DD_BEV_MAP_MAX_LAYERS, one_hot_encode's limit
BEV_MAP_AUX = (("visibility", 1, 1), ("center_offset", 2, 2), ("center_ohw", 4, 4), ("height", 8, 1))   # name, bit, channels


def bev_map_aux_channels(aux_sel):
    return sum(ch for _, bit, ch in BEV_MAP_AUX if aux_sel & bit)


def bev_map_workspace_bytes(total):
    n = _native.load().dd_bev_map_workspace_bytes(int(total))
    if n < 0:
        raise _native.Unsupported("dualdiff_amd.bev_map_layers: %d boxes are more than one call takes" % total)
    return n


def bev_map_layers(static, corners, bottom_center, height, visibility, labels, offsets, size, ns, nd, aux_sel, l2c, *,
                   workspace=None, out=None):
    """The BEV object layers and aux channels of a batch in two launches (include/dualdiff_hip.h: dd_bev_map_layers;
    dataset/pipeline.py:88-217).  static: uint8 (b, ns, S, S) holding 0 / 1, or int32 (b, S, S) bit fields, or None with ns
    = 0; corners (total, 8, 3), bottom_center (total, 3), height, visibility (total,) fp32, labels (total,) int64, offsets
    (b + 1,) int32 — contiguous device tensors; size = S; aux_sel: an OR of BEV_MAP_AUX's bits; l2c = (sx, ox, sy, oy):
    canvas x = x * sx + ox.  workspace: a uint8 device tensor of at least bev_map_workspace_bytes(total) bytes, 16-byte
    aligned (default: a new one); out = (masks, aux, flags) to write into (default: new ones).
    -> (masks (b, ns + nd, S, S) uint8, aux (b, ch, S, S) fp32 or None, flags (1,) int32: the number of boxes whose quad
    is of the family that is not drawn).  Nothing is read back."""
    what = "bev_map_layers"
    size, ns, nd, aux_sel = int(size), int(ns), int(nd), int(aux_sel)
    if size <= 0 or ns < 0 or nd < 0 or ns + nd == 0:
        raise ValueError("%s: size must be positive and ns + nd > 0, got %d, %d + %d" % (what, size, ns, nd))
    if ns + nd > BEV_MAP_MAX_LAYERS:
        raise ValueError("%s: at most %d layers, got %d + %d" % (what, BEV_MAP_MAX_LAYERS, ns, nd))
    if not 0 <= aux_sel <= 15:
        raise ValueError("%s: aux_sel must be an OR of the bits 1, 2, 4, 8, got %d" % (what, aux_sel))
    if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.shape[0] < 2:
        raise ValueError("%s takes int32 offsets (b + 1,), got %s %s" % (what, offsets.dtype, tuple(offsets.shape)))
    b = offsets.shape[0] - 1
    if corners.dim() != 3 or tuple(corners.shape[1:]) != (8, 3) or corners.dtype != torch.float32:
        raise ValueError("%s takes fp32 corners (total, 8, 3), got %s %s" % (what, corners.dtype, tuple(corners.shape)))
    total = corners.shape[0]
    for name, t, shape, dt in (("bottom_center", bottom_center, (total, 3), torch.float32),
                               ("height", height, (total,), torch.float32),
                               ("visibility", visibility, (total,), torch.float32), ("labels", labels, (total,), torch.int64)):
        if t.dtype != dt or tuple(t.shape) != shape:
            raise ValueError("%s takes %s %s %s, got %s %s" % (what, dt, name, shape, t.dtype, tuple(t.shape)))
    bits = False
    if ns > 0:
        if static is None:
            raise ValueError("%s: %d static layers and no static input" % (what, ns))
        if static.dtype == torch.int32 and tuple(static.shape) == (b, size, size):
            bits = True
        elif static.dtype != torch.uint8 or tuple(static.shape) != (b, ns, size, size):
            raise ValueError("%s takes static layers uint8 (%d, %d, %d, %d) or bit fields int32 (%d, %d, %d), got %s %s"
                             % (what, b, ns, size, size, b, size, size, static.dtype, tuple(static.shape)))
    else:
        static = None
    try:
        sx, ox, sy, oy = (float(v) for v in l2c)
    except (TypeError, ValueError):
        raise ValueError("%s: l2c must be (sx, ox, sy, oy), got %r" % (what, l2c))
    ins = (static, corners, bottom_center, height, visibility, labels, offsets)
    if any(t is not None and not t.is_contiguous() for t in ins):
        raise ValueError("%s takes contiguous tensors" % what)
    _need_gpu(*ins)
    dev = offsets.device
    need = bev_map_workspace_bytes(total)
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or workspace.numel() < need or not workspace.is_contiguous():
        raise ValueError("%s: the workspace must be a contiguous uint8 tensor of at least %d bytes" % (what, need))
    ch = bev_map_aux_channels(aux_sel)
    if out is None:
        masks = torch.empty((b, ns + nd, size, size), dtype=torch.uint8, device=dev)
        aux = torch.empty((b, ch, size, size), dtype=torch.float32, device=dev) if ch else None
        flags = torch.empty((1,), dtype=torch.int32, device=dev)
    else:
        masks, aux, flags = out
        if masks.dtype != torch.uint8 or tuple(masks.shape) != (b, ns + nd, size, size) or not masks.is_contiguous() \
                or flags.dtype != torch.int32 or flags.numel() != 1 or (aux is None) != (ch == 0) \
                or (aux is not None and (aux.dtype != torch.float32 or tuple(aux.shape) != (b, ch, size, size)
                                         or not aux.is_contiguous())):
            raise ValueError("%s: out must be (uint8 (%d, %d, %d, %d), fp32 (%d, %d, %d, %d) or None, int32 (1,))"
                             % (what, b, ns + nd, size, size, b, ch, size, size))
        _written(masks, aux, flags)
    _need_gpu(workspace, masks, aux, flags)
    lib = _native.load()
    _native.check(lib.dd_bev_map_layers(_ptr(static), 1 if bits else 0, _ptr(corners), _ptr(bottom_center), _ptr(height),
                                        _ptr(visibility), _ptr(labels), _ptr(offsets), total, b, size, ns, nd, aux_sel,
                                        sx, ox, sy, oy, _ptr(workspace), workspace.numel(), _ptr(masks), _ptr(aux),
                                        _ptr(flags), _stream()), what)
    return masks, aux, flags


FGM_MAX_POINTS, FGM_MAX_PIXELS, FGM_REC_WORDS = 8, 1 << 20, 24     # csrc/fgm_mask_core.h, include/dualdiff_hip.h
FGM_REC_NV, FGM_REC_FLAGGED, FGM_REC_WEIGHT, FGM_REC_AREA, FGM_REC_BBOX = 16, 17, 18, 19, 20
FGM_LOSS_DTYPES = {torch.float16: DD_F16, torch.bfloat16: DD_BF16, torch.float32: _native.DD_F32}


def fgm_workspace_bytes(total):
    n = _native.load().dd_fgm_workspace_bytes(int(total))
    if n < 0:
        raise _native.Unsupported("dualdiff_amd.fgm_mask: %d boxes are more than one call takes" % total)
    return n


def fgm_mask(bboxes, masks, lidar2image, resolution, crop=None, scale=None, *, workspace=None):
    """The FGM loss mask of a batch in two launches (include/dualdiff_hip.h: dd_fgm_mask; networks/utils.py:26-39, 100-163
    and hd_crop, dataset/utils.py:348-353).  bboxes (b, n, m, P, 3) fp32 with P <= 8, masks (b, n, m) bool or uint8,
    lidar2image (b, n, 4, 4) fp32 — contiguous device tensors; resolution = (W, H) of the latent grid; crop = (H_out, W_out)
    or None; scale = (sx, sy), default (W / 1600, H / 900).  workspace: a uint8 device tensor of at least
    fgm_workspace_bytes(b * n * m) bytes, 16-byte aligned (default: a new one); after the call it holds the box records.
    -> (heat (b, n, H_out, W_out) fp32, flags (1,) int32: the number of unsupported boxes).  Nothing is read back."""
    what = "fgm_mask"
    try:
        width, height = (int(v) for v in resolution)
        ho, wo = (height, width) if crop is None else (int(v) for v in crop)
        sx, sy = (width / 1600, height / 900) if scale is None else (float(v) for v in scale)
    except (TypeError, ValueError):
        raise ValueError("%s: resolution = (W, H), crop = (H_out, W_out), scale = (sx, sy), got %r, %r, %r"
                         % (what, resolution, crop, scale))
    if width < 1 or height < 1 or width * height > FGM_MAX_PIXELS:
        raise ValueError("%s: the grid must be at least 1 x 1 and at most %d pixels, got %d x %d"
                         % (what, FGM_MAX_PIXELS, width, height))
    if not (1 <= wo <= width and 1 <= ho <= height) or (width - wo) % 2:
        raise ValueError("%s: the crop (%d, %d) must fit the grid (%d, %d) and leave an even number of columns"
                         % (what, ho, wo, height, width))
    if bboxes.dim() != 5 or bboxes.shape[4] != 3 or not 1 <= bboxes.shape[3] <= FGM_MAX_POINTS or bboxes.dtype != torch.float32:
        raise ValueError("%s takes fp32 bboxes (b, n, m, P <= %d, 3), got %s %s"
                         % (what, FGM_MAX_POINTS, bboxes.dtype, tuple(bboxes.shape)))
    b, n, m, points = bboxes.shape[:4]
    if masks.dtype not in (torch.bool, torch.uint8) or tuple(masks.shape) != (b, n, m):
        raise ValueError("%s takes bool masks (%d, %d, %d), got %s %s" % (what, b, n, m, masks.dtype, tuple(masks.shape)))
    if lidar2image.dtype != torch.float32 or tuple(lidar2image.shape) != (b, n, 4, 4):
        raise ValueError("%s takes fp32 lidar2image (%d, %d, 4, 4), got %s %s"
                         % (what, b, n, lidar2image.dtype, tuple(lidar2image.shape)))
    if b * n < 1:
        raise ValueError("%s: no view in bboxes %s" % (what, tuple(bboxes.shape)))
    ins = (bboxes, masks, lidar2image)
    if any(not t.is_contiguous() for t in ins):
        raise ValueError("%s takes contiguous tensors" % what)
    _need_gpu(*ins)
    dev = bboxes.device
    need = fgm_workspace_bytes(b * n * m)
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or workspace.numel() < need or not workspace.is_contiguous():
        raise ValueError("%s: the workspace must be a contiguous uint8 tensor of at least %d bytes" % (what, need))
    else:
        _written(workspace)
    _need_gpu(workspace)
    heat = torch.empty((b, n, ho, wo), dtype=torch.float32, device=dev)
    flags = torch.empty((1,), dtype=torch.int32, device=dev)
    lib = _native.load()
    _native.check(lib.dd_fgm_mask(_ptr(bboxes), _ptr(masks), _ptr(lidar2image), b * n, m, points, width, height, wo, ho,
                                  sx, sy, _ptr(workspace), workspace.numel(), _ptr(heat), _ptr(flags), _stream()), what)
    return heat, flags


def fgm_loss_groups(count):
    """the workgroups of dd_fgm_loss's first launch (include/dualdiff_hip.h: a function of the element count alone)"""
    return max(1, min((int(count) + 1023) // 1024, 1024))


def fgm_loss(pred, target, heat=None, want_grad=False):
    """sum((pred - target)^2 * (1 + heat)) / N in fp32 and, with want_grad, its gradient to pred in pred's dtype, in one
    pass over the inputs plus one workgroup over the partials (include/dualdiff_hip.h: dd_fgm_loss; runner/
    multiview_runner.py:501-507).  pred, target (b, n, c, h, w) fp16 / bf16 / fp32, heat (b, n, h, w) fp32 or None (the plain
    mean) — contiguous device tensors.  -> (loss () fp32, grad or None).  Nothing is read back."""
    what = "fgm_loss"
    if pred.dtype not in FGM_LOSS_DTYPES:
        raise TypeError("%s takes fp16 / bf16 / fp32 tensors, got %s" % (what, pred.dtype))
    if pred.dim() != 5 or pred.numel() == 0 or target.shape != pred.shape or target.dtype != pred.dtype:
        raise ValueError("%s takes pred and target of one shape (b, n, c, h, w) and dtype, got %s %s and %s %s"
                         % (what, pred.dtype, tuple(pred.shape), target.dtype, tuple(target.shape)))
    b, n, c, h, w = pred.shape
    if heat is not None and (heat.dtype != torch.float32 or tuple(heat.shape) != (b, n, h, w)):
        raise ValueError("%s takes fp32 heat (%d, %d, %d, %d), got %s %s" % (what, b, n, h, w, heat.dtype, tuple(heat.shape)))
    ins = (pred, target, heat)
    if any(t is not None and not t.is_contiguous() for t in ins):
        raise ValueError("%s takes contiguous tensors" % what)
    _need_gpu(*ins)
    lib = _native.load()
    need = lib.dd_fgm_loss_workspace_bytes(pred.numel())
    if need < 0:
        raise _native.Unsupported("dualdiff_amd.%s: %d elements are more than one call takes" % (what, pred.numel()))
    partials = torch.empty((need // 4,), dtype=torch.float32, device=pred.device)
    loss = torch.empty((), dtype=torch.float32, device=pred.device)
    grad = torch.empty_like(pred) if want_grad else None
    _native.check(lib.dd_fgm_loss(_ptr(pred), _ptr(target), _ptr(heat), _ptr(grad), _ptr(loss), _ptr(partials), need, b * n,
                                  c, h * w, FGM_LOSS_DTYPES[pred.dtype], _stream()), what)
    return loss, grad


ADAMW_CHUNK = 8192                               # include/dualdiff_hip.h: DD_ADAMW_CHUNK
ADAMW_ROW_WORDS, ADAMW_STATE_BYTES = 6, 96       # dd_adamw_row as int64 words (p, g, m, v, shadow, numel); dd_adamw_state
ADAMW_STATE_FIELDS = {                           # name -> (byte offset, type) of dd_adamw_state
    "step": (0, torch.int64), "beta1_pow": (8, torch.float64), "beta2_pow": (16, torch.float64),
    "grad_norm": (24, torch.float32), "clip_coef": (28, torch.float32), "found_inf": (32, torch.int32),
    "skipped": (40, torch.int64), "lr": (48, torch.float32), "decay": (52, torch.float32), "w1": (56, torch.float32),
    "b2": (60, torch.float32), "w2": (64, torch.float32), "step_size": (68, torch.float32), "bc2_sqrt": (72, torch.float32),
    "eps": (76, torch.float32), "inv_scale": (80, torch.float32)}
ADAMW_SHADOW_DTYPES = {torch.float16: DD_F16, torch.bfloat16: DD_BF16}
ADAMW_ALL = 7                                    # DD_ADAMW_ALL: the three launches of a step


def adamw_chunk():
    """the elements of one chunk of dd_adamw_step's table (include/dualdiff_hip.h: DD_ADAMW_CHUNK)"""
    return ADAMW_CHUNK


def adamw_chunks(numels):
    """The chunk list of a table whose rows have these element counts -> int32 (n_chunks, 2) on the host: (row, chunk of
    the row), row-major.  A row with no element has no chunk."""
    per_row = [(int(n) + ADAMW_CHUNK - 1) // ADAMW_CHUNK for n in numels]
    if any(int(n) < 0 for n in numels) or sum(per_row) > 2 ** 31 - 1:
        raise ValueError("adamw_chunks: element counts must be non-negative and give fewer than 2^31 chunks")
    if not per_row:
        return torch.empty((0, 2), dtype=torch.int32)
    rows =torch.repeat_interleave(torch.arange(len(per_row), dtype=torch.int32), torch.tensor(per_row, dtype=torch.int64))
    first = torch.cumsum(torch.tensor([0] + per_row[:-1], dtype=torch.int64), 0)
    within = torch.arange(rows.numel(), dtype=torch.int64) - torch.repeat_interleave(first, torch.tensor(per_row, dtype=torch.int64))
    return torch.stack([rows, within.to(torch.int32)], 1).contiguous()


def adamw_table(rows):
    """The descriptor table of dd_adamw_step for rows = [(p, g, m, v, shadow), ...] -> int64 (n, 6) on the host, to be
    copied to the device.  p, m, v: fp32; g: fp32 or None (the row is left alone); shadow: fp16 / bf16 or None — all of
    p's shape, contiguous, on p's device, which is one GPU for the whole table.  Checked here, on the host, before any
    launch; an error names the offending row.  -> (table, the shadows' dtype or None)."""
    what = "adamw_table"
    words, shadow_dtype, device = [], None, None
    for i, row in enumerate(rows):
        if len(row) != 5:
            raise ValueError("%s: row %d is not (p, g, m, v, shadow)" % (what, i))
        p, g, m, v, shadow = row
        for name, t, optional in (("p", p, False), ("g", g, True), ("m", m, False), ("v", v, False)):
            if t is None and optional:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
                raise TypeError("%s: row %d: %s must be an fp32 tensor, got %s"
                                % (what, i, name, t.dtype if isinstance(t, torch.Tensor) else type(t).__name__))
        if shadow is not None:
            if not isinstance(shadow, torch.Tensor) or shadow.dtype not in ADAMW_SHADOW_DTYPES:
                raise TypeError("%s: row %d: the shadow must be an fp16 or bf16 tensor, got %s"
                                % (what, i, shadow.dtype if isinstance(shadow, torch.Tensor) else type(shadow).__name__))
            if shadow_dtype is not None and shadow.dtype != shadow_dtype:
                raise TypeError("%s: row %d: the shadow is %s, the rows before have %s shadows (one type per table)"
                                % (what, i, shadow.dtype, shadow_dtype))
            shadow_dtype = shadow.dtype
        for name, t in (("g", g), ("m", m), ("v", v), ("shadow", shadow)):
            if t is None:
                continue
            if t.shape != p.shape:
                raise ValueError("%s: row %d: %s has shape %s, p has %s" % (what, i, name, tuple(t.shape), tuple(p.shape)))
            if t.device != p.device:
                raise ValueError("%s: row %d: %s is on %s, p is on %s" % (what, i, name, t.device, p.device))
        for name, t in (("p", p), ("g", g), ("m", m), ("v", v), ("shadow", shadow)):
            if t is not None and not t.is_contiguous():
                raise ValueError("%s: row %d: %s is not contiguous" % (what, i, name))
        if device is not None and p.device != device:
            raise ValueError("%s: row %d is on %s, the rows before are on %s" % (what, i, p.device, device))
        device = p.device
        words.append([p.data_ptr(), 0 if g is None else g.data_ptr(), m.data_ptr(), v.data_ptr(),
                      0 if shadow is None else shadow.data_ptr(), p.numel()])
    if device is not None and device.type != "cuda":                # after the rows' own faults, which need no GPU to be found
        raise RuntimeError("%s: dualdiff_amd ops run on the GPU only (the rows are on %s); there is no CPU fallback"
                           % (what, device))
    return torch.tensor(words, dtype=torch.int64).reshape(len(words), ADAMW_ROW_WORDS), shadow_dtype


def adamw_state(step=0, betas=(0.9, 0.999), skipped=0):
    """the bytes of a dd_adamw_state after `step` taken steps, as a uint8 (96,) tensor on the host: the running products
    start from Python's beta ** step, everything else is zero"""
    import struct
    block = struct.pack("<qddffiiq", int(step), float(betas[0]) ** int(step), float(betas[1]) ** int(step), 0.0, 0.0, 0, 0,
                        int(skipped))
    return torch.frombuffer(bytearray(block.ljust(ADAMW_STATE_BYTES, b"\0")), dtype=torch.uint8).clone()


def adamw_state_field(state, name):
    """a one-element view of a field of the state block (device or host), of the field's own type"""
    at, dtype = ADAMW_STATE_FIELDS[name]
    return state[at:at + torch.empty((), dtype=dtype).element_size()].view(dtype)


def adamw_workspace_bytes(n_chunks):
    n = _native.load().dd_adamw_workspace_bytes(int(n_chunks))
    if n < 0:
        raise _native.Unsupported("dualdiff_amd.adamw_step: %d chunks are more than one call takes" % n_chunks)
    return n


def adamw_step(table, chunks, state, lr_table, *, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None,
               grad_scale=None, found_inf=None, shadow_dtype=torch.float16, workspace=None, written=(), launches=ADAMW_ALL):
    """One optimizer step over a descriptor table in three launches — GradScaler's unscale and non-finite search,
    clip_grad_norm_, torch.optim.AdamW's update, the 16-bit shadows — with nothing read back (include/dualdiff_hip.h:
    dd_adamw_step; runner/multiview_runner.py:512-521).  table int64 (n, 6) (adamw_table), chunks int32 (n_chunks, 2)
    (adamw_chunks), state uint8 (96,) (adamw_state), lr_table fp32 (len >= 1,), grad_scale / found_inf one fp32 each or None
    — contiguous tensors of one GPU.  written: a list of the tensors of the caller's that the table points to and a taken
    step rewrites (every p, m, v and shadow of a row with a gradient; no None, no inference tensor); each counts a version.  workspace: a uint8 device tensor
    of at least adamw_workspace_bytes(n_chunks) bytes (default: a new one).  launches: ADAMW_ALL, or a subset of the three
    for timing."""
    what = "adamw_step"
    if table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != ADAMW_ROW_WORDS or not table.is_contiguous():
        raise ValueError("%s takes a contiguous int64 table (n, %d), got %s %s"
                         % (what, ADAMW_ROW_WORDS, table.dtype, tuple(table.shape)))
    if chunks.dtype != torch.int32 or chunks.dim() != 2 or chunks.shape[1] != 2 or not chunks.is_contiguous():
        raise ValueError("%s takes contiguous int32 chunks (n_chunks, 2), got %s %s" % (what, chunks.dtype, tuple(chunks.shape)))
    if state.dtype != torch.uint8 or state.numel() < ADAMW_STATE_BYTES or not state.is_contiguous():
        raise ValueError("%s takes a contiguous uint8 state block of %d bytes" % (what, ADAMW_STATE_BYTES))
    if lr_table.dtype != torch.float32 or lr_table.dim() != 1 or lr_table.numel() < 1 or not lr_table.is_contiguous():
        raise ValueError("%s takes a contiguous 1-D fp32 lr_table with at least one entry, got %s %s"
                         % (what, lr_table.dtype, tuple(lr_table.shape)))
    for name, t in (("grad_scale", grad_scale), ("found_inf", found_inf)):
        if t is not None and (t.dtype != torch.float32 or t.numel() != 1):
            raise ValueError("%s: %s must be one fp32 value, got %s %s" % (what, name, t.dtype, tuple(t.shape)))
    if shadow_dtype not in ADAMW_SHADOW_DTYPES:
        raise TypeError("%s: shadows are fp16 or bf16, got %s" % (what, shadow_dtype))
    beta1, beta2 = (float(b) for b in betas)
    if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0) or not eps >= 0.0 or not weight_decay >= 0.0:
        raise ValueError("%s: betas in [0, 1), eps >= 0, weight_decay >= 0, got %r, %r, %r" % (what, betas, eps, weight_decay))
    if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
        raise ValueError("%s: max_grad_norm must be None or >= 0, got %r" % (what, max_grad_norm))
    if not 1 <= int(launches) <= ADAMW_ALL:
        raise ValueError("%s: launches is a mask in [1, %d], got %r" % (what, ADAMW_ALL, launches))
    ins = (table, chunks, state, lr_table, grad_scale, found_inf)
    _need_gpu(*ins)
    if any(t is not None and t.device != table.device for t in ins):
        raise ValueError("%s takes tensors of one device" % what)
    need = adamw_workspace_bytes(chunks.shape[0])
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=table.device)
    elif workspace.dtype != torch.uint8 or workspace.numel() < need or not workspace.is_contiguous() \
            or workspace.device != table.device:
        raise ValueError("%s: the workspace must be a contiguous uint8 tensor of at least %d bytes on %s"
                         % (what, need, table.device))
    _written(state, workspace)
    if written:                        # _written's count, in one call for the hundreds of tensors of a table (1 ms otherwise)
        torch.autograd.graph.increment_version(written)
    lib = _native.load()
    _native.check(lib.dd_adamw_step(_ptr(table), table.shape[0], _ptr(chunks), chunks.shape[0], _ptr(state), _ptr(lr_table),
                                    lr_table.numel(), _ptr(grad_scale), _ptr(found_inf), beta1, beta2, float(eps),
                                    float(weight_decay), -1.0 if max_grad_norm is None else float(max_grad_norm),
                                    ADAMW_SHADOW_DTYPES[shadow_dtype], _ptr(workspace), workspace.numel(), int(launches),
                                    _stream()), what)


MAP_MAX_LAYERS = 31                              # include/dualdiff_hip.h: DD_MAP_MAX_LAYERS; bit 31 of `used` is taken
MAP_SIDES = {"right": 0, "below": 1}


def map_render_u8(maps, stab, dtab, ns, nd):
    """The layers of a batch of BEV maps -> the coloured maps and the classes in use, in one launch (include/
    dualdiff_hip.h: dd_map_render_u8; runner/map_visualizer.py:106-132, 180-190).  maps (b, C, S, S) uint8 holding 0 / 1,
    stab (ns + 1, 4) fp32 = colour / 255 and priority rank per static layer plus the "nothing" row, dtab (nd, 4) fp32 =
    colour / 255 per dynamic layer or None for nd == 0; ns + nd <= C — all contiguous device tensors.
    -> (img (b, 3, S, S) fp32 holding colour / 255: what image_resample_u8 quantises back to the colour bytes, used (b,)
    int32).  Nothing is read back."""
    what = "map_render_u8"
    if maps.dim() != 4 or maps.shape[2] != maps.shape[3] or maps.numel() == 0:
        raise ValueError("%s takes square maps (b, C, S, S), got %s" % (what, tuple(maps.shape)))
    if maps.dtype != torch.uint8:
        raise ValueError("%s takes uint8 maps, got %s" % (what, maps.dtype))
    b, c, s = maps.shape[0], maps.shape[1], maps.shape[2]
    ns, nd = int(ns), int(nd)
    if ns < 0 or nd < 0 or ns + nd == 0 or ns + nd > c:
        raise ValueError("%s: %d static + %d dynamic layers do not fit a map of %d layers" % (what, ns, nd, c))
    if ns + nd > MAP_MAX_LAYERS:
        raise ValueError("%s: at most %d layers, got %d + %d" % (what, MAP_MAX_LAYERS, ns, nd))
    if stab.dtype != torch.float32 or tuple(stab.shape) != (ns + 1, 4):
        raise ValueError("%s: stab must be fp32 (%d, 4), got %s %s" % (what, ns + 1, stab.dtype, tuple(stab.shape)))
    if nd > 0 and (dtab is None or dtab.dtype != torch.float32 or tuple(dtab.shape) != (nd, 4)):
        raise ValueError("%s: dtab must be fp32 (%d, 4)" % (what, nd))
    ins = (maps, stab, dtab if nd > 0 else None)
    if any(t is not None and not t.is_contiguous() for t in ins):
        raise ValueError("%s takes contiguous tensors" % what)
    _need_gpu(*ins)
    img = torch.empty((b, 3, s, s), dtype=torch.float32, device=maps.device)
    used = torch.empty((b,), dtype=torch.int32, device=maps.device)
    lib = _native.load()
    _timer.launch(what, lib.dd_map_render_u8, _ptr(maps), _ptr(stab), _ptr(ins[2]), _ptr(img), _ptr(used), b, c, s, ns, nd,
                  _stream(), book=lambda: ("dd_map_render_kernel", 0.0, float(b * s * s * (ns + nd + 12))))
    return img, used


def map_compose_u8(src, index=None, legend=None, side="right"):
    """The quarter turn, the zero pad and the legend of `visualize_map` (runner/map_visualizer.py:197-209) for the samples
    of a batch that share a legend, in one launch (dd_map_compose_u8).  src (m, T, T, 3) uint8: the resized, not yet turned
    pictures; index (g,) int32: the samples to take, None for all of them in order; legend (lh, lw, 3) uint8 or None;
    side "right" (lh <= T) or "below" (lw <= T) — contiguous device tensors.
    -> (g, T, T + lw, 3) or (g, T + lh, T, 3) uint8: np.rot90 of the picture, the legend beside or below it, zero elsewhere."""
    what = "map_compose_u8"
    if src.dim() != 4 or src.shape[1] != src.shape[2] or src.shape[3] != 3 or src.numel() == 0 or src.dtype != torch.uint8:
        raise ValueError("%s takes square uint8 pictures (m, T, T, 3), got %s %s" % (what, src.dtype, tuple(src.shape)))
    if side not in MAP_SIDES:
        raise ValueError("%s: side must be one of %s, got %r" % (what, ", ".join(sorted(MAP_SIDES)), side))
    m, t = src.shape[0], src.shape[1]
    g = m
    if index is not None:
        if index.dtype != torch.int32 or index.dim() != 1 or index.numel() == 0:
            raise ValueError("%s: index must be a non-empty int32 vector, got %s %s" % (what, index.dtype, tuple(index.shape)))
        g = index.shape[0]
    lh = lw = 0
    if legend is not None:
        if legend.dim() != 3 or legend.shape[2] != 3 or legend.numel() == 0 or legend.dtype != torch.uint8:
            raise ValueError("%s: legend must be uint8 (lh, lw, 3), got %s %s" % (what, legend.dtype, tuple(legend.shape)))
        lh, lw = legend.shape[0], legend.shape[1]
        if (lh if side == "right" else lw) > t:
            raise ValueError("%s: a %d x %d legend does not lie %s a %d x %d picture" % (what, lh, lw, side, t, t))
    ins = (src, index, legend)
    if any(x is not None and not x.is_contiguous() for x in ins):
        raise ValueError("%s takes contiguous tensors" % what)
    _need_gpu(*ins)
    shape = (g, t, t + lw, 3) if side == "right" else (g, t + lh, t, 3)
    out = torch.empty(shape, dtype=torch.uint8, device=src.device)
    lib = _native.load()
    _timer.launch(what, lib.dd_map_compose_u8, _ptr(src), _ptr(index), _ptr(legend), _ptr(out), m, g, t, lh, lw,
                  MAP_SIDES[side], _stream(),
                  book=lambda: ("dd_map_compose_kernel", 0.0, float(g * t * t * 3 + out.numel())))
    return out


def attn_heat(maps, cols, table, hw, out=None):
    """The selected context columns of an attention map -> one coloured tile per (view, column), in one launch (include/
    dualdiff_hip.h: dd_attn_heat; tools/explore_attn.py:118-128, 138-148).  maps (views, h * w, n) float32 with unit
    stride along n — any row pitch >= n and any view stride, so a slice of a padded buffer is taken as it is; cols (t,)
    int32, each in [0, n); table (257, 4) float32 (image_tables.cmap_table) — device tensors.
    -> img (views * t, 3, h, w) float32 holding colour / 255: what image_resample_u8 quantises back to the colour bytes.
    Nothing is read back."""
    what = "attn_heat"
    try:
        h, w = (int(v) for v in hw)
    except (TypeError, ValueError):
        raise ValueError("%s: hw must be (h, w), got %r" % (what, hw))
    if h <= 0 or w <= 0:
        raise ValueError("%s: hw must be positive, got %r" % (what, hw))
    if maps.dim() != 3 or maps.numel() == 0 or maps.shape[1] != h * w:
        raise ValueError("%s takes maps (views, %d, n) for hw %s, got %s" % (what, h * w, (h, w), tuple(maps.shape)))
    if maps.dtype != torch.float32:
        raise ValueError("%s takes float32 maps, got %s" % (what, maps.dtype))
    views, q, n = maps.shape
    if maps.stride(2) != 1 or maps.stride(1) < n or maps.stride(0) < 0:
        raise ValueError("%s takes maps with unit stride along n and a row pitch >= n, got strides %s"
                         % (what, maps.stride()))
    if cols.dtype != torch.int32 or cols.dim() != 1 or cols.numel() == 0 or not cols.is_contiguous():
        raise ValueError("%s: cols must be a non-empty contiguous int32 vector, got %s %s"
                         % (what, cols.dtype, tuple(cols.shape)))
    if table.dtype != torch.float32 or tuple(table.shape) != (257, 4) or not table.is_contiguous():
        raise ValueError("%s: table must be contiguous float32 (257, 4), got %s %s" % (what, table.dtype, tuple(table.shape)))
    t = cols.shape[0]
    if views * t > 65535:
        raise ValueError("%s: at most 65535 tiles per launch, got %d x %d" % (what, views, t))
    shape = (views * t, 3, h, w)
    if out is not None and (out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous()):
        raise ValueError("%s: out must be a contiguous float32 %s tensor" % (what, shape))
    _need_gpu(maps, cols, table, out)
    _written(out)
    img = torch.empty(shape, dtype=torch.float32, device=maps.device) if out is None else out
    lib = _native.load()
    _timer.launch(what, lib.dd_attn_heat, _ptr(maps), _ptr(cols), _ptr(table), _ptr(img), views, h, w, n, t,
                  maps.stride(1), maps.stride(0), _stream(),
                  book=lambda: ("dd_attn_heat_kernel", 0.0, float(views * t * q * (2 * 4 + 12))))
    return img


def attn_sheet_u8(tiles, index, rows, cols, gap, labels=None, out=None):
    """view_images' canvas (tools/explore_attn.py:25-53) for a batch of sheets, in one launch (dd_attn_sheet_u8).  tiles
    (m, th, tw, 3) uint8; index (sheets, rows * cols) int32: the tile of every cell in row-major order, -1 for an all-255
    cell; gap: the gutter in pixels; labels (m, lh, tw, 3) uint8 or None: pasted over the bottom lh rows of the tile of
    the same number — contiguous device tensors.
    -> (sheets, rows * th + gap * (rows - 1), cols * tw + gap * (cols - 1), 3) uint8, 255 wherever no tile lies."""
    what = "attn_sheet_u8"
    if tiles.dim() != 4 or tiles.shape[3] != 3 or tiles.numel() == 0 or tiles.dtype != torch.uint8:
        raise ValueError("%s takes uint8 tiles (m, th, tw, 3), got %s %s" % (what, tiles.dtype, tuple(tiles.shape)))
    ints = (rows, cols, gap)
    if any(isinstance(v, bool) or not isinstance(v, int) for v in ints) or rows <= 0 or cols <= 0 or gap < 0:
        raise ValueError("%s: rows and cols must be positive ints and gap a non-negative one, got %r" % (what, ints))
    if index.dtype != torch.int32 or index.dim() != 2 or index.shape[0] == 0 or index.shape[1] != rows * cols:
        raise ValueError("%s: index must be int32 (sheets, %d), got %s %s" % (what, rows * cols, index.dtype, tuple(index.shape)))
    m, th, tw = tiles.shape[0], tiles.shape[1], tiles.shape[2]
    sheets, lh = index.shape[0], 0
    if labels is not None:
        if labels.dim() != 4 or labels.dtype != torch.uint8 or labels.shape[0] != m or labels.shape[2:] != (tw, 3) \
                or not 0 < labels.shape[1] <= th:
            raise ValueError("%s: labels must be uint8 (%d, lh <= %d, %d, 3), got %s %s"
                             % (what, m, th, tw, labels.dtype, tuple(labels.shape)))
        lh = labels.shape[1]
    ins = (tiles, index, labels)
    if any(x is not None and not x.is_contiguous() for x in ins):
        raise ValueError("%s takes contiguous tensors" % what)
    oh, ow = rows * th + gap * (rows - 1), cols * tw + gap * (cols - 1)
    if sheets > 65535 or oh * ow >= 1 << 31:
        raise ValueError("%s: at most 65535 sheets of less than 2^31 pixels, got %d of %d x %d" % (what, sheets, oh, ow))
    out = _image_out(out, (sheets, oh, ow, 3), tiles.device, what)
    _need_gpu(*ins, out)
    lib = _native.load()
    _timer.launch(what, lib.dd_attn_sheet_u8, _ptr(tiles), _ptr(index), _ptr(labels), _ptr(out), m, sheets, rows, cols, th,
                  tw, lh, gap, _stream(),
                  book=lambda: ("dd_attn_sheet_kernel", 0.0, float(2 * out.numel())))
    return out


def groupnorm(x, gamma, beta, m, hw, groups, eps, silu, x2=None, out=None):
    """GroupNorm (+SiLU) over an NHWC batch; x2 = optional second source concatenated on C."""
    lib = _native.load()
    _need_gpu(x, gamma, beta, x2, out)
    c1 = x.shape[1]
    c2 = x2.shape[1] if x2 is not None else 0
    if not x.is_contiguous() or (x2 is not None and not x2.is_contiguous()):
        raise ValueError("groupnorm inputs must be contiguous")
    out = _out_or_new(out, (m * hw, c1 + c2), x.dtype, x.device, "groupnorm")
    need = lib.dd_groupnorm_workspace_bytes(m, groups)
    ws = workspace(need, x.device, "gn")

    def book():      # HBM-bound: each element read once and written once
        th = lib.dd_groupnorm_is_fused(hw, c1 + c2, groups)
        return ("dd_gn_fused_kernel<%s, %d, 8>" % (_tname(_dt(x)), th) if th
                else "dd_gn_stats_kernel + dd_gn_apply_kernel (2 launches)", 0.0, (4.0 if th else 6.0) * out.numel())
    _timer.launch("groupnorm", lib.dd_groupnorm_nhwc, _ptr(x), c1, _ptr(x2), c2, _ptr(gamma), _ptr(beta), _ptr(out),
                  m, hw, groups, eps, int(silu), _dt(x), _ptr(ws), ws.numel() * 4, _stream(), book=book)
    return out


def layernorm(x, gamma, beta, eps=1e-5, out=None):
    lib = _native.load()
    _need_gpu(x, gamma, beta, out)
    x = _rows2d(x)
    if not x.is_contiguous():
        raise ValueError("layernorm input must be contiguous")
    out = _out_or_new(out, x, x.dtype, x.device, "layernorm")
    _timer.launch("layernorm", lib.dd_layernorm, _ptr(x), _ptr(gamma), _ptr(beta), _ptr(out), x.shape[0], x.shape[1],
                  eps, _dt(x), _stream(), book=lambda: ("dd_layernorm", 0.0, 4.0 * out.numel()))
    return out


def attention(q, k, v, batch, lq, lk, heads, head_dim, scale=None, *, kv_batch_map=None,
              out=None, accumulate=False, variant=0, q_prescaled=False, seq_strides=None,
              out_seq_strides=None, kv_batch_map2=None, kv_seq_strides=None, lk_dev=None):
    """softmax(scale * q k^T) v per (batch, head).

    q / k / v may also be HEAD-MAJOR 3-D tensors (heads, rows, head_dim) — slices of a
    `gemm(..., head_major=...)` result; q_prescaled: q already carries scale * log2(e).

    q: (batch*lq, >= heads*head_dim) row-strided view; k, v: (kv_batches*lk, ...) likewise, so
    slices of a fused QKV projection can be passed without copies.  kv_batch_map (int32 device
    tensor [batch]) redirects batch b to K/V of another batch (neighbour views); with kv_batch_map2 as well the
    result is Attn(q, kv[map]) + Attn(q, kv[map2]) — the neighbour-view PAIR of attn4 in one launch.

    seq_strides = (row_stride, batch_stride) in elements for q, k, v (row-major 2-D views with the same row
    pitch), out_seq_strides likewise for `out` (default: the same): the sequence runs over rows `row_stride`
    apart and consecutive batches start `batch_stride` apart — attention ALONG ANOTHER AXIS of a (frames, tokens, C) activation without a transpose
    (temporal attention: row_stride = tokens_per_frame * C, batch_stride = C).  kv_seq_strides: the same pair for k / v
    when they live in another buffer than q (frame-split temporal attention: local queries, gathered keys).

    lk_dev: int32 device tensor [1] with the number of keys every batch entry REALLY has; `lk` is then the capacity the
    K / V rows were laid out for (dd_attn_desc.lk_dev: the kernel reads the count at its start, so a recorded HIP graph
    serves every context length up to the capacity)."""
    lib = _native.load()
    _need_gpu(q, k, v, out, kv_batch_map, kv_batch_map2, lk_dev)
    _check_lk_dev(lk_dev)
    if kv_batch_map2 is not None and (kv_batch_map is None or seq_strides is not None):
        raise ValueError("kv_batch_map2 needs kv_batch_map and no seq_strides")
    if kv_seq_strides is not None and seq_strides is None:
        raise ValueError("kv_seq_strides needs seq_strides")
    d = AttnDesc()

    def operand(t, l):
        """-> (ptr, ld, batch stride, head stride) for a row-major 2-D view, a head-major 3-D tensor
        (heads, rows, d) or a batch-major 4-D tensor (batches, heads, l, d) with contiguous [l][d] blocks (the
        K/V layout of the view-sharded neighbour attention: whole instances are contiguous messages)."""
        if t.dim() == 4:
            if t.shape[1] != heads or t.shape[2] != l or t.shape[3] != head_dim or t.stride(3) != 1 \
                    or t.stride(2) != head_dim:
                raise ValueError("batch-major operand must be (batches, heads, l, head_dim) with contiguous blocks")
            return t.data_ptr(), head_dim, t.stride(0), t.stride(1)
        if t.dim() == 3:
            if t.shape[0] != heads or t.shape[2] != head_dim or t.stride(2) != 1 or t.stride(1) != head_dim:
                raise ValueError("head-major operand must be (heads, rows, head_dim) with contiguous planes")
            return t.data_ptr(), head_dim, l * head_dim, t.stride(0)
        t = _rows2d(t)
        return t.data_ptr(), t.stride(0), l * t.stride(0), 0
    d.q, d.ldq, d.q_batch_stride, d.q_head_stride = operand(q, lq)
    d.k, d.ldk, d.k_batch_stride, d.k_head_stride = operand(k, lk)
    d.v, d.ldv, d.v_batch_stride, d.v_head_stride = operand(v, lk)
    d.q_prescaled = int(bool(q_prescaled))
    out = _rows2d(_out_or_new(out, (q.shape[0] if seq_strides is not None else batch * lq, heads * head_dim), q.dtype,
                              q.device, "attention"))
    d.o, d.ldo = out.data_ptr(), out.stride(0)
    d.o_batch_stride = lq * out.stride(0)
    if seq_strides is not None:
        if q.dim() != 2 or k.dim() != 2 or v.dim() != 2 or kv_batch_map is not None:
            raise ValueError("seq_strides takes row-major 2-D q / k / v and no kv_batch_map")
        rs, bs = int(seq_strides[0]), int(seq_strides[1])
        ors, obs = (rs, bs) if out_seq_strides is None else (int(out_seq_strides[0]), int(out_seq_strides[1]))
        krs, kbs = (rs, bs) if kv_seq_strides is None else (int(kv_seq_strides[0]), int(kv_seq_strides[1]))
        d.ldq, d.ldk, d.ldv = rs, krs, krs
        d.q_batch_stride, d.k_batch_stride, d.v_batch_stride = bs, kbs, kbs
        d.ldo, d.o_batch_stride = ors, obs
    d.batch, d.heads, d.head_dim, d.lq, d.lk = batch, heads, head_dim, lq, lk
    d.scale = float(scale) if scale is not None else head_dim ** -0.5
    d.kv_batch_map = kv_batch_map.data_ptr() if kv_batch_map is not None else None
    d.kv_batch_map2 = kv_batch_map2.data_ptr() if kv_batch_map2 is not None else None
    npair = 2 if kv_batch_map2 is not None else 1
    d.accumulate = int(accumulate)
    d.dtype = _dt(q)
    d.variant = variant
    d.lk_dev = lk_dev.data_ptr() if lk_dev is not None else None
    if seq_strides is not None and batch * heads > 65535:
        # the launcher's grid covers at most 65535 (batch, head) pairs: walk the batch in chunks
        es, per = q.element_size(), 65535 // heads
        base = (d.q, d.k, d.v, d.o)
        for b0 in range(0, batch, per):
            d.batch = min(per, batch - b0)
            d.q = base[0] + b0 * d.q_batch_stride * es
            d.k, d.v = base[1] + b0 * d.k_batch_stride * es, base[2] + b0 * d.v_batch_stride * es
            d.o = base[3] + b0 * d.o_batch_stride * es
            _native.check(lib.dd_attention(ctypes.byref(d), _stream()), "attention")
        return out
    _timer.launch("attention", lib.dd_attention, ctypes.byref(d), _stream(),
                  book=lambda: ("dd_attn5_kernel<%s,D%d>" % (_tname(d.dtype), head_dim),
                                4.0 * batch * heads * lq * lk * head_dim * npair,
                                2.0 * heads * head_dim * batch * (2 * lq + 2 * lk * npair)))
    return out


ATTN_PROBS_MAX_LK = 256         # DD_ATTN_PROBS_MAX_LK of include/dualdiff_hip.h


def attention_probs(q, k, batch, lq, lk, heads, head_dim, scale=None, *, q_prescaled=False, per_head=False, out=None,
                    accumulate=False, weight=1.0, lk_dev=None):
    """softmax(scale * q k^T) itself, in float32 (dd_attn_probs) — the probabilities `attention` and `xattn320` never
    write: (batch, heads, lq, lk) with per_head, else their mean over the heads (batch, lq, lk), times `weight`.

    q / k as `attention` takes them: (batch*l, >= heads*head_dim) row-strided 2-D views (column slices of a fused
    projection) or head-major 3-D tensors (heads, rows, head_dim); q_prescaled: q carries scale * log2(e).  Row slices
    of either form select batch entries without a copy.  out: float32 (batch, [heads,] lq, lk) with unit inner stride
    (a row pitch that is a multiple of 4 floats on a 16-byte aligned base takes the vector stores); accumulate: add to
    `out` instead of storing.  lk_dev as in `attention`: the real key count, `lk` the capacity; a store then writes the
    columns past it as zeros, an accumulate leaves them alone.  head_dim 40 / 80 / 160, lk <= ATTN_PROBS_MAX_LK."""
    batch, lq, lk, heads, head_dim = int(batch), int(lq), int(lk), int(heads), int(head_dim)
    if min(batch, lq, lk, heads, head_dim) <= 0:
        raise ValueError("attention_probs: batch, lq, lk, heads and head_dim must be positive")
    if q.dtype != k.dtype:
        raise ValueError("attention_probs: q is %s, k is %s" % (q.dtype, k.dtype))

    def operand(t, l, name):
        if t.dim() == 3:
            if t.shape[0] != heads or t.shape[1] != batch * l or t.shape[2] != head_dim or t.stride(2) != 1 \
                    or t.stride(1) != head_dim:
                raise ValueError("attention_probs: head-major %s must be (%d, %d, %d) with contiguous rows, got %s"
                                 % (name, heads, batch * l, head_dim, tuple(t.shape)))
            return t.data_ptr(), head_dim, l * head_dim, t.stride(0)
        if t.dim() != 2 or t.stride(1) != 1 or t.shape[0] != batch * l or t.shape[1] < heads * head_dim:
            raise ValueError("attention_probs: %s must be a (%d, >= %d) view with unit inner stride, got shape %s stride %s"
                             % (name, batch * l, heads * head_dim, tuple(t.shape), t.stride()))
        return t.data_ptr(), t.stride(0), l * t.stride(0), 0
    qa, ka = operand(q, lq, "q"), operand(k, lk, "k")
    shape = (batch, heads, lq, lk) if per_head else (batch, lq, lk)
    if out is None:
        if accumulate:
            raise ValueError("attention_probs: accumulate needs out")
    elif tuple(out.shape) != shape or out.stride(-1) != 1:
        raise ValueError("attention_probs: out must be %s with unit inner stride, got shape %s stride %s"
                         % (shape, tuple(out.shape), out.stride()))
    _dtype_code(q.dtype)
    _check_lk_dev(lk_dev)
    _need_gpu(q, k, out, lk_dev)
    lib = _native.load()
    if out is None:             # rows at a pitch of whole float4 groups
        out = torch.empty(shape[:-1] + ((lk + 3) // 4 * 4,), dtype=torch.float32, device=q.device)[..., :lk]
    elif out.dtype != torch.float32:
        raise TypeError("attention_probs: out must be torch.float32")
    else:
        _written(out)
    _timer.launch("attention_probs", lib.dd_attn_probs, _ptr(q), _ptr(k), _ptr(out), qa[1], ka[1], qa[2], ka[2], qa[3],
                  ka[3], out.stride(-2), out.stride(0), out.stride(1) if per_head else 0, batch, lq, lk, heads, head_dim,
                  float(scale) if scale is not None else head_dim ** -0.5, int(bool(q_prescaled)), int(bool(per_head)),
                  int(bool(accumulate)), float(weight), _ptr(lk_dev), _dt(q), _stream(),
                  book=lambda: ("dd_attn_probs_kernel<%s,D%d>" % (_tname(_dt(q)), head_dim),
                                2.0 * batch * heads * lq * lk * head_dim,
                                2.0 * heads * head_dim * batch * (lq + lk) + 4.0 * out.numel() * (2 if accumulate else 1)))
    return out


def causal_attention(q, k, v, batch, l, heads, head_dim, out=None):
    """softmax_{j <= i}(head_dim^-0.5 * q_i . k_j) v_j per (sequence, head) — CLIP's self-attention (dd_causal_attention:
    head_dim 64, l <= CAUSAL_ATTN_MAX_L).  q, k, v: (batch*l, >= heads*head_dim) row-strided views, so the column slices
    of a fused Q|K|V projection are passed without copies; returns (batch*l, heads*head_dim)."""
    lib = _native.load()
    _need_gpu(q, k, v, out)
    q, k, v = _rows2d(q), _rows2d(k), _rows2d(v)
    for t in (q, k, v):
        if t.shape[0] != batch * l or t.shape[1] < heads * head_dim or t.dtype != q.dtype:
            raise ValueError("causal_attention operands must be (%d, >= %d) %s views, got %s %s"
                             % (batch * l, heads * head_dim, q.dtype, tuple(t.shape), t.dtype))
    if out is not None and (out.shape[0] != batch * l or out.shape[1] < heads * head_dim or out.dtype != q.dtype):
        raise ValueError("causal_attention: out must be (%d, >= %d) %s" % (batch * l, heads * head_dim, q.dtype))
    out = _rows2d(_out_or_new(out, (batch * l, heads * head_dim), q.dtype, q.device, "causal_attention"))
    _timer.launch("causal_attention", lib.dd_causal_attention, _ptr(q), _ptr(k), _ptr(v), _ptr(out), q.stride(0),
                  k.stride(0), v.stride(0), out.stride(0), l * q.stride(0), l * k.stride(0), l * v.stride(0),
                  l * out.stride(0), batch, l, heads, head_dim, float(head_dim) ** -0.5, _dt(q), _stream(),
                  book=lambda: ("dd_causal_attn_kernel<%s>" % _tname(_dt(q)), 2.0 * batch * heads * l * l * head_dim,
                                2.0 * heads * head_dim * batch * l * 4))
    return out


def clip_embed(ids, tok, pos, eos_token_id):
    """CLIPTextEmbeddings + the pooling position (dd_clip_embed): ids (b, l) int64 on the GPU, tok (vocab, c), pos
    (>= l, c) -> (rows (b*l, c) = tok[ids] + pos[:l] summed in fp32 and rounded once, pool_index (b,) int32 = the
    position pooler_output reads: ids.argmax(-1) for eos_token_id == 2, else the first eos_token_id, 0 when absent).
    Ids outside [0, vocab) are clamped by the kernel."""
    lib = _native.load()
    _need_gpu(ids, tok, pos)
    if ids.dim() != 2 or ids.dtype != torch.int64 or not ids.is_contiguous():
        raise ValueError("ids must be a contiguous (b, l) int64 tensor, got %s %s" % (tuple(ids.shape), ids.dtype))
    b, l = ids.shape
    if tok.dim() != 2 or pos.dim() != 2 or tok.shape[1] != pos.shape[1] or pos.shape[0] < l or tok.dtype != pos.dtype \
            or not tok.is_contiguous() or not pos.is_contiguous():
        raise ValueError("token / position tables must be contiguous (vocab, c) / (>= %d, c) of one dtype" % l)
    rows = torch.empty((b * l, tok.shape[1]), dtype=tok.dtype, device=tok.device)
    pool = torch.empty((b,), dtype=torch.int32, device=tok.device)
    rc = lib.dd_clip_embed(_ptr(ids), _ptr(tok), _ptr(pos), _ptr(rows), _ptr(pool), b, l, tok.shape[1], tok.shape[0],
                           int(eos_token_id), _dt(tok), _stream())
    _native.check(rc, "clip_embed")
    return rows, pool


def xattn320_ok(c, heads, lk, rows=None):
    """Shapes the fused cross-attention kernel covers (dd_xattn320): the 320-channel level, 8 heads, <= 128 keys — and,
    when the caller states its row count, a grid of at most XATTN_MAX_WGS 80-row workgroups."""
    if rows is not None and (int(rows) + 79) // 80 > XATTN_MAX_WGS:
        return False
    return int(c) == 320 and int(heads) == 8 and 0 < int(lk) <= 128


def xattn_pack_weight(w):
    """[320, 320] Linear weight -> the K-step-major, pre-swizzled 1-D copy dd_xattn320 streams by linear LDS-DMA
    (dd_xattn_pack_weight).  NOT cached here: the owning module keeps the copy as a `_pk_*` entry beside its other packed
    weights (layers.Linear.wx), so it lives exactly as long as the module, is dropped by `_drop_cache` on .to() /
    load_state_dict, and can never be evicted under a captured HIP graph that holds its address (a
    process-global, size-capped cache could free buffers a graph still replays from)."""
    if tuple(w.shape) != (320, 320) or not w.is_contiguous():
        raise ValueError("xattn320 weights must be contiguous (320, 320)")
    _need_gpu(w)
    lib = _native.load()
    packed = torch.empty(320 * 320, dtype=w.dtype, device=w.device)
    _native.check(lib.dd_xattn_pack_weight(_ptr(w), _ptr(packed), _dt(w), _stream()), "xattn_pack_weight")
    return packed


def _xpacked(w):
    """Packed weights are 1-D (102400,); a raw (320, 320) weight is packed on the spot (uncached: a fresh buffer, which
    inside a capture belongs to the graph's own pool)."""
    return w if w.dim() == 1 and w.numel() == 320 * 320 else xattn_pack_weight(w)


def _zero_bias(dtype, device):
    return device_const(("zero_bias", dtype), device, lambda: torch.zeros(320, dtype=dtype))


def xattn320(x, wq, wo, bo, k, v, instances, rows_per_inst, lk, scale, *, res=None, ln_out=None, out=None, lk_dev=None):
    """Fused q-projection -> attention over the lk context keys of each view-instance -> out-projection + bias +
    residual, one launch (include/dualdiff_hip.h: dd_xattn320).  x: (instances * rows_per_inst, 320); k / v: either
    (instances * lk, >= 320) row-strided 2-D views (column slices of a wider projection) or HEAD-MAJOR 3-D tensors
    (8, instances * lk, 40) — slices of a `gemm(..., head_major=(40, 0, 1.0))` result, the form the kernel streams
    fastest; wq / wo: the packed copies of the (320, 320) Linear weights (xattn_pack_weight; layers.Linear.wx) or the raw weights; ln_out = (gamma, beta, eps):
    LayerNorm(out) comes back as `out._ln_out`.  lk_dev: as in attention() — the real key count in device memory, `lk`
    the capacity of the K / V layout."""
    lib = _native.load()
    _need_gpu(x, wq, wo, bo, k, v, res, out, lk_dev)
    _check_lk_dev(lk_dev)
    x = _rows2d(x)
    rows = instances * rows_per_inst
    if x.shape != (rows, 320):
        raise ValueError("xattn320: x must be (instances * rows_per_inst, 320)")

    def kv_operand(t):
        if t.dim() == 3:                      # head-major planes
            if t.shape[0] != 8 or t.shape[1] != instances * lk or t.shape[2] != 40 or t.stride(2) != 1 or t.stride(1) != 40:
                raise ValueError("head-major K / V must be (8, instances * lk, 40) with contiguous planes")
            return t.data_ptr(), 40, lk * 40, t.stride(0)
        t = _rows2d(t)
        if t.shape[0] != instances * lk or t.shape[1] < 320:
            raise ValueError("row-major K / V must be (instances * lk, >= 320)")
        return t.data_ptr(), t.stride(0), lk * t.stride(0), 40
    out = _rows2d(_out_or_new(out, (rows, 320), x.dtype, x.device, "xattn320"))
    wqp, wop = _xpacked(wq), _xpacked(wo)
    d = XAttnDesc()
    d.x, d.ldx = x.data_ptr(), x.stride(0)
    if res is not None:
        res = _rows2d(res)
        d.res, d.ldres = res.data_ptr(), res.stride(0)
    d.wq, d.wo = wqp.data_ptr(), wop.data_ptr()
    if bo is None:                      # the kernel loads the bias unconditionally (a conditional load would be waited for in place)
        bo = _zero_bias(x.dtype, x.device)
    d.bo = bo.data_ptr()
    d.k, d.ldk, d.k_inst_stride, d.k_head_stride = kv_operand(k)
    d.v, d.ldv, d.v_inst_stride, d.v_head_stride = kv_operand(v)
    d.out, d.ldo = out.data_ptr(), out.stride(0)
    d.instances, d.rows_per_inst, d.lk = int(instances), int(rows_per_inst), int(lk)
    d.channels, d.heads, d.scale, d.dtype = 320, 8, float(scale), _dt(x)
    d.lk_dev = lk_dev.data_ptr() if lk_dev is not None else None
    second = None
    if ln_out is not None:
        g_, b_, eps_ = ln_out
        _need_gpu(g_, b_)
        second = torch.empty((rows, 320), dtype=x.dtype, device=x.device)
        d.ln_out, d.ld_ln_out = second.data_ptr(), 320
        d.ln_gamma, d.ln_beta, d.ln_eps = g_.data_ptr(), b_.data_ptr(), float(eps_)
    # 2 projections + attention; bytes: x in, out out (+ res, + ln_out), weights, K / V
    _timer.launch("xattn320", lib.dd_xattn320, ctypes.byref(d), _stream(),
                  book=lambda: ("dd_xattn320_kernel", 4.0 * rows * 320 * 320 + 4.0 * rows * lk * 320,
                                2.0 * (rows * 320 * (2 + (1 if res is not None else 0) + (1 if second is not None else 0))
                                       + 2 * 320 * 320 + 2 * instances * lk * 320)))
    if second is not None:
        out._ln_out = second
    return out


def add(a, b, c=None, out=None):
    lib = _native.load()
    _need_gpu(a, b, c, out)
    out = _out_or_new(out, a, a.dtype, a.device, "add")
    _timer.launch("add", lib.dd_add, _ptr(a), _ptr(b), _ptr(c), _ptr(out), a.numel(), _dt(a), _stream(),
                  book=lambda: ("dd_add", 0.0, 2.0 * a.numel() * (3 + (1 if c is not None else 0))))
    return out


def scale(x, s, out=None):
    lib = _native.load()
    _need_gpu(x, out)
    out = _out_or_new(out, x, x.dtype, x.device, "scale")
    _native.check(lib.dd_scale(_ptr(x), _ptr(out), s, x.numel(), _dt(x), _stream()), "scale")
    return out


def silu(x, out=None):
    lib = _native.load()
    _need_gpu(x, out)
    out = _out_or_new(out, x, x.dtype, x.device, "silu")
    _native.check(lib.dd_silu(_ptr(x), _ptr(out), x.numel(), _dt(x), _stream()), "silu")
    return out


def nchw_to_nhwc(x, c_pad=None, views=1):
    """(m, c, h, views * w) contiguous -> (m * views * h * w, c_pad) NHWC rows with zero-padded channels (default: no
    padding); views > 1 also splits a panorama into its views (map_embedder.py:116-125).  c_pad % 8 == 0: one LDS-tiled
    launch, both sides coalesced (csrc/tokens.hip); other widths (views == 1 only): the element-wise kernel."""
    lib = _native.load()
    _need_gpu(x)
    m, c, h, wt = x.shape
    if wt % views:
        raise ValueError("nchw_to_nhwc: width %d is not %d views" % (wt, views))
    c_pad = c if c_pad is None else c_pad
    x = x.contiguous()
    out = torch.empty((m * views * h * (wt // views), c_pad), dtype=x.dtype, device=x.device)
    if c_pad % 8 == 0:
        rc = lib.dd_nchw_to_nhwc_views(_ptr(x), _ptr(out), m, c, h, wt // views, views, c_pad, _dt(x), _stream())
    elif views == 1:
        rc = lib.dd_nchw_to_nhwc(_ptr(x), _ptr(out), m, c, h * wt, c_pad, _dt(x), _stream())
    else:
        raise ValueError("nchw_to_nhwc: a view split needs c_pad % 8 == 0")
    _native.check(rc, "nchw_to_nhwc")
    return out


def nhwc_to_nchw(x, m, c, h, w):
    """(m*h*w, ld>=c) -> (m, c, h, w) contiguous."""
    lib = _native.load()
    _need_gpu(x)
    x = _rows2d(x)
    out = torch.empty((m, c, h, w), dtype=x.dtype, device=x.device)
    rc = lib.dd_nhwc_to_nchw(_ptr(x), _ptr(out), m, c, h * w, x.stride(0), _dt(x), _stream())
    _native.check(rc, "nhwc_to_nchw")
    return out


def timestep_embedding(t, dim, dtype, flip_sin_to_cos=True, freq_shift=0.0, out=None):
    """t: fp32 device tensor [n] -> (n, dim) sinusoidal embedding in `dtype`."""
    lib = _native.load()
    _need_gpu(t, out)
    if t.dtype != torch.float32:
        raise TypeError("timesteps must be fp32")
    n = t.numel()
    out = _out_or_new(out, (n, dim), dtype if out is None else out.dtype, t.device, "timestep_embedding")
    rc = lib.dd_timestep_embedding(_ptr(t), _ptr(out), n, dim, int(flip_sin_to_cos), freq_shift,
                                   _dt(out), _stream())
    _native.check(rc, "timestep_embedding")
    return out


def conv3x3_small_cout(x, w, bias, m, h, wd, out=None):
    """conv_out: x (m*h*wd, cin) NHWC, w (cout<=8, 9*cin) -> (m, cout, h, wd) NCHW."""
    lib = _native.load()
    _need_gpu(x, w, bias, out)
    cin = x.shape[1]
    cout = w.shape[0]
    out = _out_or_new(out, (m, cout, h, wd), x.dtype, x.device, "conv3x3_small_cout")
    rc = lib.dd_conv3x3_small_cout(_ptr(x), _ptr(w), _ptr(bias), _ptr(out), m, h, wd, cin, cout,
                                   _dt(x), _stream())
    _native.check(rc, "conv3x3_small_cout")
    return out


class GivenViews(_collections.namedtuple("GivenViews", "mask clean noise0 gcoef mode")):
    """Given-view state of the fused sampler step (pipeline_bev_controlnet_given_view.py; include/dualdiff_hip.h):
    mask   uint8 device (views,), non-zero for a given view-instance (the latents are `views` equal blocks);
    clean  fp32 device (n...), the clean latents of the given views (any values elsewhere);
    noise0 device (n...) in the latents' dtype, the latents at loop entry;
    gcoef  fp32 device [3], the current row of schedulers.given_view_table (refreshed between graph replays);
    mode   1: re-noise the given views every step (conditional_latents_change_every_input=True), 2: fixed noise."""


def _given_args(g, x):
    _need_gpu(g.mask, g.clean, g.noise0, g.gcoef)
    if g.mode not in (1, 2):
        raise ValueError("given-view mode is 1 (change every input) or 2 (fixed noise), got %r" % (g.mode,))
    if g.mask.dtype != torch.uint8 or g.mask.dim() != 1 or not g.mask.is_contiguous() or g.mask.numel() == 0:
        raise ValueError("given-view mask must be a contiguous uint8 vector with one byte per view-instance")
    if x.numel() % g.mask.numel():
        raise ValueError("%d latent elements are not %d equal views" % (x.numel(), g.mask.numel()))
    if g.clean.dtype != torch.float32 or g.clean.numel() != x.numel() or not g.clean.is_contiguous():
        raise ValueError("given-view clean latents must be contiguous fp32 with the latents' %d elements" % x.numel())
    if g.noise0.dtype != x.dtype or g.noise0.numel() != x.numel() or not g.noise0.is_contiguous():
        raise ValueError("given-view noise0 must be contiguous, in the latents' dtype, with their %d elements" % x.numel())
    if g.gcoef.dtype != torch.float32 or g.gcoef.numel() < 3:
        raise ValueError("given-view gcoef must be a fp32 device row of 3")
    return x.numel() // g.mask.numel()


def cfg_ddim_step(eps, x, coef, guidance, x_out=None, x_dup=None, given=None):
    """eps: (2, n...) uncond first; x: (n...); coef: fp32 device [4].
    given: None (the plain step) or a GivenViews — dd_cfg_ddim_step_given."""
    lib = _native.load()
    _need_gpu(eps, x, coef, x_out, x_dup)
    _written(x_out, x_dup)
    if x_out is None:
        x_out = torch.empty_like(x)
    if given is None:
        rc = lib.dd_cfg_ddim_step(_ptr(eps), _ptr(x), _ptr(x_out), _ptr(x_dup), _ptr(coef),
                                  float(guidance), x.numel(), _dt(x), _stream())
        _native.check(rc, "cfg_ddim_step")
        return x_out
    ve = _given_args(given, x)
    rc = lib.dd_cfg_ddim_step_given(_ptr(eps), _ptr(x), _ptr(x_out), _ptr(x_dup), _ptr(coef), float(guidance),
                                    _ptr(given.mask), _ptr(given.clean), _ptr(given.noise0), _ptr(given.gcoef),
                                    int(given.mode), x.numel(), ve, _dt(x), _stream())
    _native.check(rc, "cfg_ddim_step_given")
    return x_out


def cfg_unipc_step(eps, x, hist, coef, guidance, x_out=None, x_dup=None, given=None):
    """eps: (2, n...) uncond first; x: (n...); hist: fp32 (3, n...) = [last, m1, m2] updated in place;
    coef: fp32 device [10] (dualdiff_amd.pipeline.schedulers.unipc_schedule row).
    given: None (the plain step) or a GivenViews — dd_cfg_unipc_step_given."""
    lib = _native.load()
    _need_gpu(eps, x, hist, coef, x_out, x_dup)
    if hist.dtype != torch.float32 or hist.shape[0] != 3 or hist[0].numel() != x.numel() or not hist.is_contiguous():
        raise ValueError("hist must be a contiguous fp32 (3, n...) tensor")
    _written(x_out, x_dup, hist)
    if x_out is None:
        x_out = torch.empty_like(x)
    if given is None:
        rc = lib.dd_cfg_unipc_step(_ptr(eps), _ptr(x), _ptr(x_out), _ptr(x_dup), _ptr(hist[0]), _ptr(hist[1]),
                                   _ptr(hist[2]), _ptr(coef), float(guidance), x.numel(), _dt(x), _stream())
        _native.check(rc, "cfg_unipc_step")
        return x_out
    ve = _given_args(given, x)
    rc = lib.dd_cfg_unipc_step_given(_ptr(eps), _ptr(x), _ptr(x_out), _ptr(x_dup), _ptr(hist[0]), _ptr(hist[1]),
                                     _ptr(hist[2]), _ptr(coef), float(guidance), _ptr(given.mask), _ptr(given.clean),
                                     _ptr(given.noise0), _ptr(given.gcoef), int(given.mode), x.numel(), ve, _dt(x),
                                     _stream())
    _native.check(rc, "cfg_unipc_step_given")
    return x_out


def given_views_noise(x, given, t0, x_dup=None):
    """x[v] (and x_dup[v]) = add_noise(clean, noise0, timesteps[0]) on the given views of `given` (a GivenViews; its
    gcoef and mode are not used), in place; t0 = schedulers.given_view_table(...)[0] (host or device, 2 values)."""
    lib = _native.load()
    _need_gpu(x, x_dup)
    ve = _given_args(given, x)
    if x_dup is not None and (x_dup.dtype != x.dtype or x_dup.numel() != x.numel()):
        raise ValueError("x_dup must match x")
    _written(x, x_dup)
    sa, s1a = (float(v) for v in t0.tolist()[:2])
    rc = lib.dd_given_views_noise(_ptr(x), _ptr(x_dup), _ptr(given.mask), _ptr(given.clean), _ptr(given.noise0),
                                  sa, s1a, x.numel(), ve, _dt(x), _stream())
    _native.check(rc, "given_views_noise")
    return x


def softmax_rows(s, dtype, pad_to=8):
    """fp32 logits (rows, cols) -> probabilities in `dtype`, (rows, cols rounded up to `pad_to`) with zero
    padding columns (the K dimension of the following P @ V GEMM must be a multiple of 8)."""
    lib = _native.load()
    _need_gpu(s)
    if s.dtype != torch.float32 or s.dim() != 2 or s.stride(1) != 1:
        raise ValueError("softmax_rows takes a row-major fp32 matrix")
    rows, cols = s.shape
    ldp = (cols + pad_to - 1) // pad_to * pad_to
    p = torch.empty((rows, ldp), dtype=dtype, device=s.device)
    _native.check(lib.dd_softmax_rows(_ptr(s), _ptr(p), rows, cols, s.stride(0), ldp, _dtype_code(dtype), _stream()), "softmax_rows")
    return p


def ors_project(occ, origin, direction, samples, step=0.2, *, want_labels=True, cond_dtype=None,
                keep_fg=True, keep_bg=True):
    """ORS ray sampling (include/dualdiff_hip.h: dd_ors_project).  occ: (200, 200, 16) uint8 on the GPU;
    origin (n, 3), direction (n, hw, 3) fp32.  Returns (labels (n, hw, samples) uint8 | None,
    cond (n, samples, hw) cond_dtype | None)."""
    lib = _native.load()
    _need_gpu(occ, origin, direction)
    if occ.dtype != torch.uint8 or tuple(occ.shape) != (200, 200, 16) or not occ.is_contiguous():
        raise ValueError("occ must be a contiguous (200, 200, 16) uint8 volume")
    origin = origin.to(torch.float32).contiguous()
    direction = direction.to(torch.float32).contiguous()
    n, hw = direction.shape[0], direction.shape[1]
    labels = torch.empty((n, hw, samples), dtype=torch.uint8, device=occ.device) if want_labels else None
    cond = torch.empty((n, samples, hw), dtype=cond_dtype, device=occ.device) if cond_dtype is not None else None
    if cond_dtype not in (None, torch.float16, torch.bfloat16):
        raise TypeError("cond_dtype must be fp16 / bf16")
    code = DD_F16 if cond_dtype is None else _dtype_code(cond_dtype)
    _native.check(lib.dd_ors_project(_ptr(occ), _ptr(origin), _ptr(direction), _ptr(labels), _ptr(cond), n, hw,
                                     int(samples), float(step), int(keep_fg), int(keep_bg), code, _stream()),
                  "ors_project")
    return labels, cond


ORS_MODES = {"all": 0, "bg": 1, "fg": 2}
ORS_OVERLAY_FLAGS = ((1, "a sample's camera picture is constant (max == min): its blend is 0 / 0 in the reference"),)


def ors_first_hit(occ, origin, direction, rig_of_sample, size, samples, step=0.2, *, mode="bg", palette,
                  want_frames=True, want_classes=False, want_visited=False, exits=3):
    """The ORS panorama in one launch (include/dualdiff_hip.h: dd_ors_first_hit; networks/occ3d_proj.py:156-198).
    occ: (b, 200, 200, 16) uint8 on the GPU; origin (r, n, 3), direction (r, n, h * w, 3) fp32 on the GPU: the ray tables
    of r rigs; rig_of_sample: b integers in [0, r) (host sequence or tensor; the range is checked here, on the host);
    size = (h, w); palette: 18 (r, g, b) byte triples.  -> (frames (b, h, n * w, 3) uint8 | None, cls (b, n, h, w) uint8
    | None), and the per-ray count of samples looked up, (b, n, h, w) int32, as a third item with want_visited."""
    lib = _native.load()
    _need_gpu(occ, origin, direction)
    if occ.dtype != torch.uint8 or occ.dim() != 4 or tuple(occ.shape[1:]) != (200, 200, 16) or not occ.is_contiguous():
        raise ValueError("occ must be a contiguous (b, 200, 200, 16) uint8 batch of volumes, got %s %s"
                         % (occ.dtype, tuple(occ.shape)))
    if origin.dtype != torch.float32 or direction.dtype != torch.float32:
        raise TypeError("origin and direction must be fp32, got %s and %s" % (origin.dtype, direction.dtype))
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError("size must be (h, w), got %r" % (size,))
    if h <= 0 or w <= 0 or int(samples) <= 0 or not float(step) > 0:
        raise ValueError("size, samples and step must be positive, got %r, %r, %r" % (size, samples, step))
    if origin.dim() != 3 or origin.shape[2] != 3 or direction.dim() != 4 or \
            tuple(direction.shape) != (origin.shape[0], origin.shape[1], h * w, 3):
        raise ValueError("origin must be (r, n, 3) and direction (r, n, %d, 3), got %s and %s"
                         % (h * w, tuple(origin.shape), tuple(direction.shape)))
    if mode not in ORS_MODES:
        raise ValueError("mode must be one of %s, got %r" % (", ".join(ORS_MODES), mode))
    if exits not in (0, 1, 2, 3):
        raise ValueError("exits must be 0 .. 3, got %r" % (exits,))
    if not (want_frames or want_classes):
        raise ValueError("ors_first_hit writes frames, classes or both: both were declined")
    pal = [int(c) for row in palette for c in row]
    if len(pal) != 54 or any(not 0 <= c <= 255 for c in pal):
        raise ValueError("palette must be 18 (r, g, b) byte triples")
    b, (r, n) = occ.shape[0], origin.shape[:2]
    rig = torch.as_tensor(rig_of_sample).detach().cpu().reshape(-1)
    if rig.dtype.is_floating_point or rig.dtype == torch.bool or rig.numel() != b:
        raise ValueError("rig_of_sample must be %d integers, got %s %s" % (b, rig.dtype, tuple(rig.shape)))
    if int(rig.min()) < 0 or int(rig.max()) >= r:
        raise ValueError("rig_of_sample must lie in [0, %d), got %s" % (r, rig.tolist()))
    rig = rig.to(torch.int32).to(occ.device)
    origin, direction = origin.contiguous(), direction.contiguous()
    frames = torch.empty((b, h, n * w, 3), dtype=torch.uint8, device=occ.device) if want_frames else None
    cls = torch.empty((b, n, h, w), dtype=torch.uint8, device=occ.device) if want_classes else None
    visited = torch.empty((b, n, h, w), dtype=torch.int32, device=occ.device) if want_visited else None
    arr = (ctypes.c_uint8 * 54)(*pal)
    _native.check(lib.dd_ors_first_hit(_ptr(occ), _ptr(origin), _ptr(direction), _ptr(rig), _ptr(cls), _ptr(frames),
                                       _ptr(visited), ctypes.cast(arr, ctypes.c_void_p), b, r, n, h, w, int(samples),
                                       float(step), ORS_MODES[mode], int(exits), _stream()), "ors_first_hit")
    return (frames, cls, visited) if want_visited else (frames, cls)


def ors_overlay(frames, camera):
    """The blend of ORS panoramas over camera panoramas of the same shape in two launches (include/dualdiff_hip.h:
    dd_ors_overlay_u8; networks/occ3d_proj.py:196-203).  frames, camera: (b, h, W, 3) uint8 on the GPU.  -> (out (b, h, W,
    3) uint8, flags (1,) int32: an OR of ORS_OVERLAY_FLAGS' bits).  Nothing is read back."""
    lib = _native.load()
    for name, t in (("frames", frames), ("camera", camera)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("ors_overlay: %s must be a tensor, got %s" % (name, type(t).__name__))
        if t.dtype != torch.uint8:
            raise TypeError("ors_overlay: %s must be uint8, got %s" % (name, t.dtype))
    _need_gpu(frames, camera)
    if frames.dim() != 4 or frames.shape[-1] != 3 or frames.numel() == 0:
        raise ValueError("ors_overlay: frames must be (b, h, W, 3), got %s" % (tuple(frames.shape),))
    if camera.shape != frames.shape:
        raise ValueError("ors_overlay: the camera panorama must have the frames' shape %s, got %s (resize it first)"
                         % (tuple(frames.shape), tuple(camera.shape)))
    frames, camera = frames.contiguous(), camera.contiguous()
    b, h, w = frames.shape[:3]
    out = torch.empty_like(frames)
    parts = torch.empty((b, 64, 2), dtype=torch.int32, device=frames.device)
    flags = torch.empty((1,), dtype=torch.int32, device=frames.device)
    _native.check(lib.dd_ors_overlay_u8(_ptr(frames), _ptr(camera), _ptr(out), _ptr(parts), _ptr(flags), b, h, w,
                                        _stream()), "ors_overlay")
    return out, flags


def fourier_embed(x, freqs, include_input=True):
    """[x, sin(f0 x), cos(f0 x), ...] on the last dim (networks/embedder.py), one kernel."""
    lib = _native.load()
    _need_gpu(x)
    code = _FDT.get(x.dtype)
    if code is None:
        raise TypeError("fourier_embed takes fp16 / bf16 / fp32 tensors, got %s" % x.dtype)
    x = x.contiguous()
    dims = x.shape[-1]
    rows = x.numel() // dims
    nf = len(freqs)
    out = torch.empty(x.shape[:-1] + (dims * ((1 if include_input else 0) + 2 * nf),), dtype=x.dtype, device=x.device)
    arr = (ctypes.c_float * nf)(*[float(f) for f in freqs])
    _native.check(lib.dd_fourier_embed(_ptr(x), _ptr(out), rows, dims, arr, nf, int(include_input), code, code,
                                       _stream()), "fourier_embed")
    return out


def camera_features(camera_param, freqs, include_input, dtype, k_pad):
    """(b, n, 3, j) camera parameters -> (b * n, k_pad) Fourier features of the j column vectors, back to back, in
    `dtype`, zero-padded from j * 3 * (include_input + 2 F) to k_pad columns — `cam_embedder(camera_param.permute(0, 1,
    3, 2)).reshape(b, n, -1)` of unet_addon_rawbox.py:308-325 plus the K padding of cam2token, in ONE launch (the
    transposed read and the padding are strides of the kernel)."""
    lib = _native.load()
    _need_gpu(camera_param)
    code = _FDT.get(camera_param.dtype)
    if code is None or camera_param.dim() != 4:
        raise TypeError("camera_features takes a (b, n, 3, j) fp16 / bf16 / fp32 tensor")
    x = camera_param.contiguous()
    b, n, dims, j = x.shape
    nf = len(freqs)
    width = dims * ((1 if include_input else 0) + 2 * nf)
    if not j * width <= k_pad <= j * width + dims:
        raise ValueError("camera_features: k_pad %d does not fit %d features" % (k_pad, j * width))
    out = torch.empty((b * n, k_pad), dtype=dtype, device=x.device)
    arr = (ctypes.c_float * nf)(*[float(f) for f in freqs])
    rc = lib.dd_fourier_embed_strided(_ptr(x), _ptr(out), b * n * j, dims, arr, nf, int(include_input), code, _FDT[dtype],
                                      j, dims * j, 1, j, k_pad, _stream())
    _native.check(rc, "camera_features")
    return out


def box_tokens(points, classes, masks, class_tokens, null_pos, null_class, freqs, include_input, pos, cat, cls_offset,
               cls_out=None, normalize=None):
    """Both operands of the box MLP in one launch (include/dualdiff_hip.h: dd_box_tokens; bbox_embedder.py:164-203).
    points (rows, P, 3) fp16 / bf16 / fp32; classes (rows,) int64; masks (rows,) bool or None; pos (rows, P * 3 * (inc + 2
    F)) and cat (rows, >= cls_offset + D) are written in place (dtype of class_tokens), and cls_out where one is given;
    normalize = (xyz_min, xyz_range)."""
    lib = _native.load()
    _need_gpu(points, classes, masks, class_tokens, null_pos, null_class, pos, cat, cls_out)
    rows, npts = points.shape[0], points.shape[1]
    d = _native.BoxTokensDesc()
    points, classes = points.contiguous(), classes.contiguous()
    if classes.dtype != torch.int64:
        classes = classes.long()
    if masks is not None:
        masks = masks.contiguous()
        masks = masks.view(torch.uint8) if masks.dtype == torch.bool else (masks != 0).view(torch.uint8)
    code = _FDT.get(points.dtype)
    if code is None or points.shape[2] != 3 or not pos.is_contiguous() or cat.stride(1) != 1:
        raise TypeError("box_tokens: points (rows, P, 3) in fp16 / bf16 / fp32, pos contiguous, cat row-major")
    nf = len(freqs)
    if tuple(pos.shape) != (rows, npts * 3 * ((1 if include_input else 0) + 2 * nf)) or pos.dtype != class_tokens.dtype \
            or cat.dtype != class_tokens.dtype or cat.shape[0] != rows:
        raise ValueError("box_tokens: operand shapes / dtypes do not match")
    _written(pos, cat, cls_out)
    d.points, d.classes, d.masks = points.data_ptr(), classes.data_ptr(), (masks.data_ptr() if masks is not None else None)
    d.class_tokens, d.null_pos, d.null_class = class_tokens.data_ptr(), null_pos.data_ptr(), null_class.data_ptr()
    d.pos, d.cat, d.cls_out = pos.data_ptr(), cat.data_ptr(), (cls_out.data_ptr() if cls_out is not None else None)
    d.rows, d.points_per_box, d.num_freqs, d.include_input = rows, npts, nf, int(include_input)
    d.class_token_dim, d.cls_offset, d.ld_cat = class_tokens.shape[1], int(cls_offset), cat.stride(0)
    d.n_classes = class_tokens.shape[0]          # kept rows with a class outside the table get NaN tokens, never a stray read
    d.points_dtype, d.dtype = code, _dt(class_tokens)
    for i, f in enumerate(freqs):
        d.freqs[i] = float(f)
    if normalize is not None:
        d.normalize = 1
        for i in range(3):
            d.xyz_min[i], d.xyz_range[i] = float(normalize[0][i]), float(normalize[1][i])
    _native.check(lib.dd_box_tokens(ctypes.byref(d), _stream()), "box_tokens")


def ctx_assemble(cam, text, box, n_cam, text_per_view=False, want_txt=True):
    """[cam_i | text | box tokens] per view-instance, and the text tokens alone (unet_addon_rawbox.py:337-361, :1007,
    :977) in one gather-copy.  cam (m, D); text (scenes, L, D) or (m, L, D) with text_per_view; box (scenes * v, N, D)
    with v in {n_cam, 1}, or None.  Returns (full (m, 1 + L + N, D), txt (m, L, D) or None)."""
    lib = _native.load()
    _need_gpu(cam, text, box)
    m, dim = cam.shape
    lt = text.shape[1]
    scenes = m // n_cam
    nbox = 0 if box is None else box.shape[1]
    box_views = n_cam if box is None else box.shape[0] // scenes
    if text.shape[0] != (m if text_per_view else scenes) or (box is not None and box.shape[0] not in (scenes, m)):
        raise ValueError("ctx_assemble: text / box batch does not match %d scenes x %d views" % (scenes, n_cam))
    cam, text = cam.contiguous(), text.contiguous()
    box = None if box is None else box.contiguous()
    full = torch.empty((m, 1 + lt + nbox, dim), dtype=cam.dtype, device=cam.device)
    txt = torch.empty((m, lt, dim), dtype=cam.dtype, device=cam.device) if want_txt else None
    rc = lib.dd_ctx_assemble(_ptr(cam), _ptr(text), _ptr(box), _ptr(full), _ptr(txt), m, n_cam, lt, nbox, dim,
                             int(text_per_view), box_views, _dt(cam), _stream())
    _native.check(rc, "ctx_assemble")
    return full, txt


def quantize_fp8(w):
    """[n, k] weight matrix -> (float8_e4m3fn [n, k], fp32 scale [n]): symmetric per-output-channel quantisation,
    scale = max|w_row| / 448 (the e4m3fn maximum), round-to-nearest (what quantize_fp8_padded() builds on for gemm8)."""
    wf = w.detach().float()
    scale = (wf.abs().amax(dim=1).clamp_min(1e-12) / 448.0).contiguous()
    q = (wf / scale[:, None]).to(torch.float8_e4m3fn).contiguous()
    return q, scale


def _kpad(k):
    return (int(k) + 127) // 128 * 128


def quantize_fp8_padded(w):
    """[n, k] weight -> (float8_e4m3fn [n, k rounded up to 128] with zero padding, fp32 scale [n]): the W8 operand of
    gemm8 (per-output-channel symmetric quantisation, the values quantize_fp8 produces)."""
    q, scale = quantize_fp8(w)
    kp = _kpad(w.shape[1])
    if kp != w.shape[1]:
        qp = torch.zeros((w.shape[0], kp), dtype=torch.uint8, device=w.device)
        qp[:, :w.shape[1]] = q.view(torch.uint8)
        q = qp.view(torch.float8_e4m3fn)
    return q.contiguous(), scale


def rowquant_fp8(x, norm=None):
    """Per-row e4m3fn quantisation of the activations (dd_rowquant_fp8), optionally behind LayerNorm `norm =
    (gamma, beta, eps)` in the same launch -> (float8_e4m3fn [rows, k rounded up to 128], fp32 scale [rows]).
    scale = max(amax / 448, 2^-126), 1 for a zero row; a row that holds a NaN or an Inf (behind the LayerNorm: anywhere in
    it) gets scale = NaN, which gemm8 turns into a NaN output row."""
    lib = _native.load()
    _need_gpu(x)
    x = _rows2d(x)
    if not x.is_contiguous():
        raise ValueError("rowquant_fp8 input must be contiguous")
    rows, c = x.shape
    kp = _kpad(c)
    q = torch.empty((rows, kp), dtype=torch.uint8, device=x.device)
    scale = torch.empty(rows, dtype=torch.float32, device=x.device)
    g_, b_, eps_ = norm if norm is not None else (None, None, 0.0)
    _timer.launch("rowquant_fp8", lib.dd_rowquant_fp8, _ptr(x), _ptr(g_), _ptr(b_), _ptr(q), _ptr(scale), rows, c, kp,
                  float(eps_), _dt(x), _stream(), book=lambda: ("dd_rowquant_fp8_kernel", 0.0, 2.0 * rows * c + rows * kp))
    return q.view(torch.float8_e4m3fn), scale


def gemm8(a8, a_scale, w8, w_scale, bias=None, *, res=None, out=None, head_major=None, dtype=torch.float16, geglu=False):
    """W8A8 projection on the fp8 matrix path (include/dualdiff_hip.h: dd_gemm8): a8 (rows, Kp) / w8 (n, Kp)
    float8_e4m3fn with rows zero-padded to Kp % 128 == 0, fp32 per-row / per-output-channel scales.  head_major as in
    gemm(): the result comes back as (n / D, rows, D) planes, the first `scaled_planes` multiplied by `scale`."""
    lib = _native.load()
    _need_gpu(a8, a_scale, w8, w_scale, bias, res, out)
    if a8.dtype != torch.float8_e4m3fn or w8.dtype != torch.float8_e4m3fn or a8.shape[1] != w8.shape[1] \
            or a8.shape[1] % 128 or not a8.is_contiguous() or not w8.is_contiguous():
        raise ValueError("gemm8 operands must be contiguous float8_e4m3fn with a common K padded to a multiple of 128")
    rows, n = a8.shape[0], w8.shape[0]
    if geglu:
        if n % 2 or res is not None or head_major is not None:
            raise ValueError("geglu: w8 has 2n rows (h | g), no residual, no head-major output")
    if a_scale.numel() != rows or w_scale.numel() != n or a_scale.dtype != torch.float32 or w_scale.dtype != torch.float32:
        raise ValueError("gemm8 scales must be fp32 [rows] / [n]")
    hm_out = None
    d = Gemm8Desc()
    if head_major is not None:
        hd, hplanes, hscale = head_major
        if out is not None or res is not None or n % hd or hd % 4:
            raise ValueError("head_major needs its own output, no residual and n % D == 0")
        hm_out = torch.empty((n // hd, rows, hd), dtype=dtype, device=a8.device)
        out = hm_out.view(rows, n)
        d.out_headmajor_d, d.hm_scaled_planes, d.hm_scale = int(hd), int(hplanes), float(hscale)
    else:
        out = _rows2d(_out_or_new(out, (rows, n // 2 if geglu else n), dtype if out is None else out.dtype, a8.device, "gemm8"))
    d.a, d.a_scale, d.lda = a8.data_ptr(), a_scale.data_ptr(), a8.stride(0)
    d.w, d.w_scale, d.ldw = w8.data_ptr(), w_scale.data_ptr(), w8.stride(0)
    d.bias = bias.data_ptr() if bias is not None else None
    if res is not None:
        res = _rows2d(res)
        d.res, d.ldres = res.data_ptr(), res.stride(0)
    d.out, d.ldc = out.data_ptr(), out.stride(0)
    if geglu:
        n //= 2
        d.geglu = 1
    d.rows, d.n, d.k_padded = rows, n, a8.shape[1]
    d.dtype = _dt(out)
    _timer.launch("gemm8", lib.dd_gemm8, ctypes.byref(d), _stream(),
                  book=lambda: ("dd_gemm8_kernel", 2.0 * rows * n * a8.shape[1],
                                1.0 * (rows + n) * a8.shape[1] + 2.0 * rows * n * (1 + (1 if res is not None else 0))))
    return hm_out if hm_out is not None else out


def gemm_kernel_name(rows, n, k, dtype=torch.bfloat16, conv=False, cin=0, hw=(0, 0)):
    """Name/plan string of the kernel dd_gemm picks for a shape (profile matching)."""
    lib = _native.load()
    d = GemmDesc()
    dummy = 16
    d.a = d.w = d.out = dummy
    d.rows, d.n, d.k, d.k1 = rows, n, k, k
    d.lda, d.ldc = k, n
    d.alpha = 1.0
    d.dtype = _dtype_code(dtype)
    if conv:
        d.conv = 1
        d.cin = cin; d.hin = d.hv = d.hout = hw[0]; d.win = d.wv = d.wout = hw[1]; d.stride = 1
    return lib.dd_gemm_kernel_name(ctypes.byref(d)).decode()


# ---- FID feature extractor (csrc/conv2d.hip) ----------------------------------------------------------------------------
CONV2D_TILES = {None: 0, "64x64": 1, "128x64": 2}
POOL3X3_MODES = {"max_s2": 0, "max_s1": 1, "avg_s1": 2}     # avg: count_include_pad=False


def conv2d_out_hw(h, w, kh, kw, stride, pad):
    """Output size of conv2d: pad = (pad_h, pad_w)."""
    return (h + 2 * pad[0] - kh) // stride + 1, (w + 2 * pad[1] - kw) // stride + 1


def _slice_out(out, rows, cols, c_off, dtype, device, what):
    """The (rows, ldc) tensor a slice-writing kernel stores into and its column offset: a fresh (rows, cols) one, or the
    caller's, of which columns c_off .. c_off + cols - 1 are written and every other one is left alone."""
    if out is None:
        if c_off:
            raise ValueError("%s: c_off needs out" % what)
        return torch.empty((rows, cols), dtype=dtype, device=device)
    if out.dtype != dtype:
        raise TypeError("%s: out must be %s" % (what, dtype))
    _rows2d(out)
    if out.shape[0] != rows or c_off < 0 or c_off + cols > out.shape[1]:
        raise ValueError("%s: out %s cannot hold %d rows x columns %d..%d" % (what, tuple(out.shape), rows, c_off,
                                                                               c_off + cols))
    _forget_derived(out)
    _written(out)
    return out


def conv2d(x, w, scale, shift, m, h, wd, kh, kw, *, stride=1, pad=(0, 0), relu=True, out=None, c_off=0, tile=None):
    """General NHWC convolution with the eval-mode BatchNorm + ReLU epilogue (dd_conv2d_nhwc): x (m*h*wd, cin) dense, w
    (cout, kh*kw*cin) packed [cout][ky][kx][cin], scale / shift fp32 (cout,) ->
    relu(conv * scale + shift) in columns c_off .. c_off + cout - 1 of `out` (rows m*hout*wout; a fresh (rows, cout)
    tensor when None).  kh, kw in 1..7, stride 1 / 2, pad = (pad_h, pad_w) <= (kh // 2, kw // 2), cin % 8 == 0,
    cout % 4 == 0."""
    lib = _native.load()
    _need_gpu(x, w, scale, shift, out)
    cin, cout = x.shape[1], w.shape[0]
    if x.shape[0] != m * h * wd or not x.is_contiguous():
        raise ValueError("conv2d: x must be contiguous (m*h*wd, cin), got %s" % (tuple(x.shape),))
    if w.dtype != x.dtype or w.shape[1] != kh * kw * cin or not w.is_contiguous():
        raise ValueError("conv2d: w must be contiguous %s (cout, %d), got %s %s" % (x.dtype, kh * kw * cin, w.dtype,
                                                                                    tuple(w.shape)))
    for t in (scale, shift):
        if t.dtype != torch.float32 or t.shape != (cout,) or not t.is_contiguous():
            raise ValueError("conv2d: scale / shift must be contiguous fp32 (%d,)" % cout)
    if tile not in CONV2D_TILES:
        raise ValueError("conv2d: tile must be one of %s" % (sorted(k for k in CONV2D_TILES if k),))
    pad_h, pad_w = (int(v) for v in pad)
    hout, wout = conv2d_out_hw(h, wd, kh, kw, stride, (pad_h, pad_w))
    if hout <= 0 or wout <= 0:
        raise ValueError("conv2d: a %d x %d image has no output under a %d x %d kernel with pad %s" % (h, wd, kh, kw, pad))
    rows = m * hout * wout
    out = _slice_out(out, rows, cout, c_off, x.dtype, x.device, "conv2d")
    _timer.launch("conv2d", lib.dd_conv2d_nhwc, _ptr(x), _ptr(w), _ptr(scale), _ptr(shift), _ptr(out), out.stride(0),
                  c_off, m, h, wd, cin, cout, kh, kw, stride, pad_h, pad_w, int(bool(relu)), CONV2D_TILES[tile], _dt(x),
                  _stream(),
                  book=lambda: (conv2d_kernel_name(rows, cout, x.dtype, tile)
                                + (" conv %dx%dx%d" % (rows, cout, kh * kw * cin) if _timer._TIMER.shapes else ""),
                                2.0 * rows * cout * kh * kw * cin,
                                2.0 * (x.numel() + w.numel() + rows * cout)))
    return out


def conv2d_kernel_name(rows, cout, dtype=torch.float16, tile=None):
    """Name of the kernel dd_conv2d_nhwc picks for a shape (profile matching)."""
    return _native.load().dd_conv2d_kernel_name(rows, cout, CONV2D_TILES[tile], _dtype_code(dtype)).decode()


def pool3x3(x, m, h, wd, mode, *, out=None, c_off=0):
    """3 x 3 pooling of NHWC rows (dd_pool3x3_nhwc): x (m*h*wd, c) dense, c % 8 == 0; mode "max_s2" (stride 2, pad 0),
    "max_s1" (stride 1, pad 1) or "avg_s1" (stride 1, pad 1, count_include_pad=False) -> columns c_off .. c_off + c - 1
    of `out`."""
    lib = _native.load()
    _need_gpu(x, out)
    if mode not in POOL3X3_MODES:
        raise ValueError("pool3x3: mode must be one of %s, got %r" % (", ".join(sorted(POOL3X3_MODES)), mode))
    c = x.shape[1]
    if x.shape[0] != m * h * wd or not x.is_contiguous():
        raise ValueError("pool3x3: x must be contiguous (m*h*wd, c), got %s" % (tuple(x.shape),))
    hout, wout = ((h - 3) // 2 + 1, (wd - 3) // 2 + 1) if mode == "max_s2" else (h, wd)
    if hout <= 0 or wout <= 0:
        raise ValueError("pool3x3: a %d x %d image has no 3 x 3 stride-2 output" % (h, wd))
    rows = m * hout * wout
    out = _slice_out(out, rows, c, c_off, x.dtype, x.device, "pool3x3")
    _timer.launch("pool3x3", lib.dd_pool3x3_nhwc, _ptr(x), _ptr(out), out.stride(0), c_off, m, h, wd, c,
                  POOL3X3_MODES[mode], _dt(x), _stream(),
                  book=lambda: ("dd_pool3x3_kernel" + (" %s %dx%d" % (mode, rows, c) if _timer._TIMER.shapes else ""), 0.0,
                                2.0 * (x.numel() + rows * c)))
    return out


def global_avgpool(x, m, hw, out=None):
    """x (m*hw, c) NHWC rows -> fp32 (m, c) means over the hw pixels, summed in fp32 (dd_global_avgpool_nhwc)."""
    lib = _native.load()
    _need_gpu(x, out)
    c = x.shape[1]
    if x.shape[0] != m * hw or not x.is_contiguous():
        raise ValueError("global_avgpool: x must be contiguous (m*hw, c), got %s" % (tuple(x.shape),))
    out = _out_or_new(out, (m, c), torch.float32, x.device, "global_avgpool")
    if tuple(out.shape) != (m, c) or not out.is_contiguous():
        raise ValueError("global_avgpool: out must be contiguous (%d, %d)" % (m, c))
    _timer.launch("global_avgpool", lib.dd_global_avgpool_nhwc, _ptr(x), _ptr(out), m, hw, c, _dt(x), _stream(),
                  book=lambda: ("dd_global_avgpool_kernel", 0.0, 2.0 * x.numel() + 4.0 * m * c))
    return out


def inception_input(x, size=(299, 299), *, resize=True, normalize=True, dtype=torch.float16, c_pad=8, out=None):
    """(m, 3, h, w) images in [0, 1] (fp16 / bf16 / fp32) -> (m*oh*ow, c_pad) NHWC rows of `dtype`:
    F.interpolate(size, mode="bilinear", align_corners=False) unless resize is false, then 2 x - 1 unless normalize is
    false; channels 3 .. c_pad - 1 are zero (dd_inception_input)."""
    m, h, w = _image_arg(x, "inception_input")
    oh, ow = (int(size[0]), int(size[1])) if resize else (h, w)
    if oh <= 0 or ow <= 0:
        raise ValueError("inception_input: size must be positive, got %r" % (size,))
    _need_gpu(x, out)
    lib = _native.load()
    out = _out_or_new(out, (m * oh * ow, c_pad), dtype, x.device, "inception_input")
    if tuple(out.shape) != (m * oh * ow, c_pad) or not out.is_contiguous():
        raise ValueError("inception_input: out must be contiguous (%d, %d)" % (m * oh * ow, c_pad))
    _timer.launch("inception_input", lib.dd_inception_input, _ptr(x), _ptr(out), m, h, w, oh, ow, c_pad,
                  int(bool(resize)), int(bool(normalize)), _FDT[x.dtype], _dtype_code(dtype), _stream(),
                  book=lambda: ("dd_inception_input_kernel", 0.0,
                                float(x.numel() * x.element_size() + out.numel() * out.element_size())))
    return out
