"""VAE encoder without a GPU: parameter names against the CPU restatement (a full AutoencoderKL state dict splits
between the two HIP halves), encode_pixel_values' argument checks, and dd_gemm_conv_pad's planning query."""
import ctypes
import os

import pytest
import torch

from oracle import vae_decoder as OV
from tests import vae_encoder_reference as RE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = 1 << 20                       # 16-byte aligned, never dereferenced by a planning query

# the three Downsample2D(padding=0) convs of a 224 x 400 view: (hin, win, channels)
ENCODER_DOWNSAMPLES = [(224, 400, 128), (112, 200, 256), (56, 100, 512)]


def _hip_encoder():
    from dualdiff_amd.networks.vae_encoder import AutoencoderKLEncoder
    return AutoencoderKLEncoder()


def test_state_dict_keys_match_the_restatement():
    hip = {k: tuple(v.shape) for k, v in _hip_encoder().state_dict().items()}
    ref = {k: tuple(v.shape) for k, v in RE.AutoencoderKLEncoder().state_dict().items()}
    assert hip == ref
    for k in ("quant_conv.weight", "encoder.conv_in.weight", "encoder.down_blocks.3.resnets.1.conv2.weight",
              "encoder.down_blocks.0.downsamplers.0.conv.weight", "encoder.down_blocks.2.downsamplers.0.conv.bias",
              "encoder.mid_block.attentions.0.to_q.weight", "encoder.conv_norm_out.weight", "encoder.conv_out.weight"):
        assert k in hip, k
    assert "encoder.down_blocks.3.downsamplers.0.conv.weight" not in hip
    assert hip["encoder.conv_out.weight"] == (8, 512, 3, 3) and hip["quant_conv.weight"] == (8, 8, 1, 1)
    assert hip["encoder.down_blocks.1.resnets.0.conv_shortcut.weight"] == (256, 128, 1, 1)


def test_full_vae_state_dict_splits_between_the_halves():
    from dualdiff_amd.networks.vae_decoder import AutoencoderKLDecoder
    enc_sd = RE.AutoencoderKLEncoder().state_dict()
    dec_sd = OV.AutoencoderKLDecoder().state_dict()
    assert not set(enc_sd) & set(dec_sd)
    full = dict(enc_sd)
    full.update(dec_sd)
    missing, unexpected = _hip_encoder().load_state_dict(full, strict=False)
    assert missing == [] and sorted(unexpected) == sorted(dec_sd)
    missing, unexpected = AutoencoderKLDecoder().load_state_dict(full, strict=False)
    assert missing == [] and sorted(unexpected) == sorted(enc_sd)


def test_encode_pixel_values_argument_checks():
    from dualdiff_amd.networks.vae_encoder import encode_pixel_values
    vae = _hip_encoder()
    with pytest.raises(ValueError, match="multiples of 8"):
        encode_pixel_values(vae, torch.zeros(1, 2, 3, 36, 64))
    with pytest.raises(ValueError, match="multiples of 8"):
        encode_pixel_values(vae, torch.zeros(1, 2, 3, 32, 60))
    with pytest.raises(ValueError, match=r"\(b, n, 3, H, W\)"):
        encode_pixel_values(vae, torch.zeros(1, 2, 4, 32, 64))
    with pytest.raises(ValueError, match=r"\(b, n, 3, H, W\)"):
        encode_pixel_values(vae, torch.zeros(2, 3, 32, 64))
    with pytest.raises(ValueError, match="float"):
        encode_pixel_values(vae, torch.zeros(1, 2, 3, 32, 64, dtype=torch.int32))
    with pytest.raises(ValueError, match="bool"):
        encode_pixel_values(vae, torch.zeros(1, 2, 3, 32, 64), given=torch.ones(1, 3, dtype=torch.bool))
    with pytest.raises(ValueError, match="bool"):
        encode_pixel_values(vae, torch.zeros(1, 2, 3, 32, 64), given=torch.ones(1, 2))
    with pytest.raises(RuntimeError, match="GPU only"):
        encode_pixel_values(vae, torch.zeros(1, 2, 3, 32, 64))
    with pytest.raises(RuntimeError, match="GPU only"):
        vae.encode(torch.zeros(2, 3, 32, 64))
    with pytest.raises(ValueError):
        vae.encode(torch.zeros(2, 4, 32, 64))


def _lib():
    from dualdiff_amd import _build, _native
    if not os.path.exists(_build.lib_path()):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _native.load(build_if_missing=False)


def _conv_desc(m, hin, win, cin, cout, stride, hout, wout, hv=None, wv=None, tile=0, split=0, dtype=0):
    from dualdiff_amd import _native
    d = _native.GemmDesc()
    d.a = d.w = d.out = d.bias = DUMMY
    d.alpha = 1.0
    d.tile, d.split_k, d.dtype = tile, split, dtype
    d.rows, d.n, d.k, d.k1 = m * hout * wout, cout, 9 * cin, 9 * cin
    d.lda, d.ldc = cin, cout
    d.conv = 1
    d.cin, d.hin, d.win, d.hv, d.wv, d.hout, d.wout, d.stride = cin, hin, win, hv or hin, wv or win, hout, wout, stride
    return d


def _name(lib, d, pad_lo):
    return lib.dd_gemm_conv_pad_kernel_name(ctypes.byref(d), pad_lo).decode()


@pytest.mark.parametrize("shape", ENCODER_DOWNSAMPLES, ids=["%dx%dx%d" % s for s in ENCODER_DOWNSAMPLES])
def test_pad0_plans_the_encoder_downsamples(shape):
    lib = _lib()
    hin, win, c = shape
    for m in (1, 6):
        for dt in (0, 1):
            d = _conv_desc(m, hin, win, c, c, 2, hin // 2, win // 2, dtype=dt)
            name = _name(lib, d, 0)
            assert name.startswith("dd_gemm_pad0_kernel<"), name
            for tile in (1, 2, 3, 4, 5):
                d.tile, d.split_k = tile, 1
                assert _name(lib, d, 0).startswith("dd_gemm_pad0_kernel<"), tile
            for tile in (11, 15, 52, 31, 39, 72):          # no pad_lo = 0 instantiation in these families
                d.tile = tile
                assert _name(lib, d, 0) == "unsupported", tile


def test_pad0_odd_sizes_and_rejections():
    lib = _lib()
    # odd input: hout = (hin - 2) // 2 + 1, which pad 1 would reject
    d = _conv_desc(2, 27, 51, 64, 64, 2, 13, 25)
    assert _name(lib, d, 0).startswith("dd_gemm_pad0_kernel<")
    assert lib.dd_gemm_kernel_name(ctypes.byref(d)).decode() == "invalid"
    assert _name(lib, _conv_desc(2, 27, 51, 64, 64, 2, 14, 26), 0) == "invalid"      # pad-1 output size
    assert _name(lib, _conv_desc(2, 28, 50, 64, 64, 2, 13, 25), 0) == "invalid"      # wrong hout
    assert _name(lib, _conv_desc(2, 28, 50, 64, 64, 1, 27, 49), 0) == "unsupported"  # stride 1
    assert _name(lib, _conv_desc(2, 14, 25, 64, 64, 2, 14, 25, hv=28, wv=50), 0) == "unsupported"   # upsample
    assert _name(lib, _conv_desc(2, 1, 8, 64, 64, 2, 1, 4), 0) == "invalid"          # 1-pixel-high image
    assert _name(lib, _conv_desc(2, 28, 50, 64, 64, 2, 14, 25), 2) == "invalid"      # pad_lo not in {0, 1}
    from dualdiff_amd import _native
    dense = _native.GemmDesc()
    dense.a = dense.w = dense.out = DUMMY
    dense.rows, dense.n, dense.k, dense.k1, dense.lda, dense.ldc, dense.alpha = 64, 64, 64, 64, 64, 64, 1.0
    assert _name(lib, dense, 0) == "invalid"
    assert lib.dd_gemm_conv_pad(ctypes.byref(_conv_desc(2, 28, 50, 64, 64, 1, 28, 50)), 0, None) == -2
    assert lib.dd_gemm_conv_pad(ctypes.byref(_conv_desc(2, 28, 50, 64, 64, 2, 13, 25)), 0, None) == -1
    d = _conv_desc(2, 28, 50, 64, 64, 2, 14, 25, tile=15, split=1)
    assert lib.dd_gemm_conv_pad(ctypes.byref(d), 0, None) == -2                     # tile without the kernel


def test_pad1_is_dd_gemm():
    """pad_lo = 1 plans exactly what dd_gemm plans: same name string and workspace, conv and dense alike."""
    lib = _lib()
    from dualdiff_amd import _native, ops
    descs = []
    for hin, win, c in ENCODER_DOWNSAMPLES:
        descs.append(_conv_desc(6, hin, win, c, c, 2, hin // 2, win // 2))
        descs.append(_conv_desc(6, hin, win, c, c, 1, hin, win, dtype=1))
    descs.append(_conv_desc(2, 27, 51, 64, 64, 2, 14, 26))
    descs.append(_conv_desc(6, 28, 50, 640, 640, 1, 28, 50))
    for d in list(descs):
        for tile, split in ((1, 1), (15, 4), (31, 2), (39, 1), (52, 3)):
            e = _native.GemmDesc.from_buffer_copy(d)
            e.tile, e.split_k = tile, split
            descs.append(e)
    dense = _native.GemmDesc()
    dense.a = dense.w = dense.out = dense.bias = DUMMY
    dense.rows, dense.n, dense.k, dense.k1, dense.lda, dense.ldc, dense.alpha = 1092, 1280, 1280, 1280, 1280, 1280, 1.0
    dense.epilogue = ops.DD_EPI_GEGLU
    descs.append(dense)
    for d in descs:
        ref = lib.dd_gemm_kernel_name(ctypes.byref(d)).decode()
        assert _name(lib, d, 1) == ref
        assert lib.dd_gemm_conv_pad_workspace_bytes(ctypes.byref(d), 1) == lib.dd_gemm_workspace_bytes(ctypes.byref(d))
