"""Return codes of the dtype validation of every launcher outside the GEMM family, without a GPU.

Each entry point is called with dummy non-null, 16-byte-aligned pointers (the value 16), small sizes that are valid
otherwise, a null stream and an element-type code it does not take: it must answer DD_ERR_BAD_ARG (-1) before any HIP
runtime call.  DD_ERR_LAUNCH (-3) on a box without a GPU would mean that the validation came after a launch.  Where a
call is wrong in two ways at once, the code that is returned is part of the contract (dd_conv3x3_thin tests the dtype
before the stride, dd_layernorm the channel count before the dtype); the expected values are literals."""
import ctypes
import os

import pytest

from dualdiff_amd import _build, _native

BAD_ARG, UNSUPPORTED = -1, -2
P = 16                                                   # non-null, 16-byte aligned, never dereferenced
FREQS = (ctypes.c_float * 4)(1.0, 2.0, 4.0, 8.0)
F16, BF16, F32 = _native.DD_F16, _native.DD_BF16, _native.DD_F32


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_build.lib_path()):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _native.load(build_if_missing=False)


def box_desc(dt, points_dt=F32):
    d = _native.BoxTokensDesc()
    d.points = d.classes = d.class_tokens = d.null_pos = d.null_class = d.pos = d.cat = P
    d.rows, d.points_per_box, d.num_freqs, d.include_input = 2, 8, 4, 1
    d.class_token_dim, d.cls_offset, d.ld_cat, d.n_classes = 8, 8, 16, 1
    d.points_dtype, d.dtype = points_dt, dt
    return ctypes.byref(d)


def gemm8_desc(dt):
    d = _native.Gemm8Desc()
    d.a = d.a_scale = d.w = d.w_scale = d.out = P
    d.rows, d.n, d.k_padded, d.lda, d.ldw, d.ldc, d.dtype = 8, 8, 128, 128, 128, 8, dt
    return ctypes.byref(d)


def xattn_desc(dt):
    d = _native.XAttnDesc()
    d.x = d.wq = d.wo = d.bo = d.k = d.v = d.out = P
    d.ldx = d.ldk = d.ldv = d.ldo = 320
    d.k_inst_stride, d.k_head_stride, d.v_inst_stride, d.v_head_stride = 1280, 40, 1280, 40
    d.instances, d.rows_per_inst, d.lk, d.channels, d.heads, d.scale, d.dtype = 1, 4, 4, 320, 8, 0.158, dt
    return ctypes.byref(d)


def attn_desc(dt):
    d = _native.AttnDesc()
    d.q = d.k = d.v = d.o = P
    d.ldq = d.ldk = d.ldv = d.ldo = 320
    d.batch, d.heads, d.head_dim, d.lq, d.lk, d.scale, d.dtype = 1, 8, 40, 4, 4, 0.158, dt
    return ctypes.byref(d)


# entry point -> its arguments without the stream, as a function of the dtype code: the 16-bit-only launchers ...
CALLS16 = {
    "dd_add": lambda dt: (P, P, None, P, 8, dt),
    "dd_scale": lambda dt: (P, P, 1.0, 8, dt),
    "dd_silu": lambda dt: (P, P, 8, dt),
    "dd_nchw_to_nhwc": lambda dt: (P, P, 1, 4, 16, 8, dt),
    "dd_nhwc_to_nchw": lambda dt: (P, P, 1, 4, 16, 8, dt),
    "dd_timestep_embedding": lambda dt: (P, P, 1, 8, 1, 0.0, dt),
    "dd_ors_project": lambda dt: (P, P, P, P, P, 1, 16, 4, 0.5, 1, 1, dt),
    "dd_softmax_rows": lambda dt: (P, P, 4, 8, 8, 8, dt),
    "dd_conv3x3_small_cout": lambda dt: (P, P, None, P, 1, 4, 4, 8, 4, dt),
    "dd_conv3x3_thin": lambda dt: (P, P, None, P, 1, 8, 8, 8, 16, 1, 0, dt),
    "dd_cfg_ddim_step": lambda dt: (P, P, P, None, P, 2.0, 64, dt),
    "dd_cfg_unipc_step": lambda dt: (P, P, P, None, P, P, P, P, 2.0, 64, dt),
    "dd_cfg_ddim_step_given": lambda dt: (P, P, P, None, P, 2.0, P, P, P, P, 1, 64, 32, dt),
    "dd_cfg_unipc_step_given": lambda dt: (P, P, P, None, P, P, P, P, 2.0, P, P, P, P, 1, 64, 32, dt),
    "dd_given_views_noise": lambda dt: (P, None, P, P, P, 0.5, 0.5, 64, 32, dt),
    "dd_groupnorm_nhwc": lambda dt: (P, 32, None, 0, P, P, P, 1, 16, 8, 1e-5, 0, dt, P, 1 << 20),
    "dd_groupnorm_splitk": lambda dt: (P, 2, None, None, 0, None, 0, None, P, P, P, 1, 16, 64, 8, 1e-5, 0, dt),
    "dd_layernorm": lambda dt: (P, P, P, P, 5, 64, 1e-5, dt),
    "dd_nchw_to_nhwc_views": lambda dt: (P, P, 1, 4, 4, 4, 1, 8, dt),
    "dd_box_tokens": lambda dt: (box_desc(dt),),
    "dd_ctx_assemble": lambda dt: (P, P, None, P, None, 1, 1, 4, 0, 8, 0, 1, dt),
    "dd_clip_embed": lambda dt: (P, P, P, P, P, 1, 4, 8, 10, 9, dt),
    "dd_causal_attention": lambda dt: (P, P, P, P, 64, 64, 64, 64, 256, 256, 256, 256, 1, 4, 1, 64, 0.125, dt),
    "dd_vae_posterior": lambda dt: (P, P, P, None, P, 1, 4, 4, 1.0, 0, dt),
    "dd_rowquant_fp8": lambda dt: (P, None, None, P, P, 4, 128, 128, 1e-5, dt),
    "dd_gemm8": lambda dt: (gemm8_desc(dt),),
    "dd_xattn_pack_weight": lambda dt: (P, P, dt),
    "dd_xattn320": lambda dt: (xattn_desc(dt),),
    "dd_attention": lambda dt: (attn_desc(dt),),
}
# ... and those that also take DD_F32 (for the two Fourier launchers and the box points: the input dtype, output fp16)
CALLS32 = {
    "dd_image_quantize_u8": lambda dt: (P, P, 2, 8, 8, 1, dt),
    "dd_image_resample_u8": lambda dt: (P, P, 2, 8, 8, 8, 8, P, P, 1, P, P, 1, 0, 0, 0, 0, 0, 1, dt),
    "dd_image_load_u8": lambda dt: (P, P, 2, 8, 8, 8, 8, P, P, 1, P, P, 1, P, dt, 0),
    "dd_fourier_embed": lambda dt: (P, P, 4, 3, FREQS, 4, 1, dt, F16),
    "dd_fourier_embed_strided": lambda dt: (P, P, 4, 3, FREQS, 4, 1, dt, F16, 1, 3, 3, 1, 27),
    "dd_box_tokens": lambda dt: (box_desc(F16, points_dt=dt),),
}
# the output dtype of the Fourier launchers, input fp32
CALLS_OUT = {
    "dd_fourier_embed": lambda dt: (P, P, 4, 3, FREQS, 4, 1, F32, dt),
    "dd_fourier_embed_strided": lambda dt: (P, P, 4, 3, FREQS, 4, 1, F32, dt, 1, 3, 3, 1, 27),
}


def test_every_dtype_taking_entry_point_is_listed():
    """The tables name every exported function that takes a dtype, the GEMM family (its own dispatch) apart."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "dualdiff_hip.h")).read(), flags=re.S)
    takes_dtype = set(re.findall(r"\bint\s+(dd_[a-z0-9_]+)\s*\([^)]*\b(?:in_|out_)?dtype\b[^)]*\)", hdr))
    by_desc = {"dd_box_tokens", "dd_gemm8", "dd_xattn320", "dd_attention"}
    assert takes_dtype | by_desc == set(CALLS16) | set(CALLS32)


@pytest.mark.parametrize("dt", [3, -1, 2])
@pytest.mark.parametrize("name", sorted(CALLS16))
def test_16_bit_launchers_reject_other_dtypes(lib, name, dt):
    assert getattr(lib, name)(*CALLS16[name](dt), None) == BAD_ARG


@pytest.mark.parametrize("dt", [3, -1])
@pytest.mark.parametrize("name", sorted(CALLS32))
def test_three_way_launchers_reject_other_dtypes(lib, name, dt):
    assert getattr(lib, name)(*CALLS32[name](dt), None) == BAD_ARG


@pytest.mark.parametrize("dt", [3, -1])
@pytest.mark.parametrize("name", sorted(CALLS_OUT))
def test_fourier_launchers_reject_other_output_dtypes(lib, name, dt):
    assert getattr(lib, name)(*CALLS_OUT[name](dt), None) == BAD_ARG


def test_conv3x3_thin_checks_the_dtype_before_the_stride(lib):
    def thin(stride, dt):
        return lib.dd_conv3x3_thin(P, P, None, P, 1, 8, 8, 8, 16, stride, 0, dt, None)
    assert thin(3, 3) == BAD_ARG
    assert thin(3, -1) == BAD_ARG
    assert thin(3, F16) == UNSUPPORTED
    assert thin(3, BF16) == UNSUPPORTED


def test_layernorm_checks_the_channel_count_before_the_dtype(lib):
    for dt in (3, -1, 2, F16, BF16):
        assert lib.dd_layernorm(P, P, P, P, 5, 12, 1e-5, dt, None) == UNSUPPORTED


def test_small_cout_conv_checks_the_shape_before_the_dtype(lib):
    assert lib.dd_conv3x3_small_cout(P, P, None, P, 1, 4, 4, 8, 16, 3, None) == UNSUPPORTED     # cout > 8
    assert lib.dd_conv3x3_small_cout(P, P, None, P, 1, 4, 4, 12, 4, -1, None) == UNSUPPORTED    # cin % 8
