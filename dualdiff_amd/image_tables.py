"""Host-side builders of the constants the image and JPEG kernels read, and their device copies.

Pure host code below `ops`: PIL's fixed-point bicubic coefficient tables, torch's bilinear taps and weights, torchvision's
normalisation table, the JPEG header and the encoder's tables, and what the PNG encoder builds (it reads no host-built table: its length codes are
arithmetic, its CRC bitwise).  The `device_*` functions put them on a device under the one rule of `_consts`.
`pipeline.image_output` re-exports the names for the callers that know them from there.
"""
import math

import torch

from ._consts import device_const

PRECISION_BITS = 32 - 8 - 2            # PIL's fixed point for 8-bit pixels

_TABLES = {}                           # (in, out) -> (kk int32 (out, ksize), bounds int32 (out, 2))


def _bicubic(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resample_tables(in_size, out_size):
    """PIL's precompute_coeffs + normalize_coeffs_8bpc for the bicubic filter (src/libImaging/Resample.c), operation for
    operation in float64: -> (kk int32 (out_size, ksize), bounds int32 (out_size, 2) = [xmin, count]).  Output xx is
    `sum_j pixel[xmin + j] * kk[xx, j]` over `count` taps in 22-bit fixed point; kk is zero beyond `count`."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise ValueError("sizes must be positive, got %d -> %d" % (in_size, out_size))
    key = (in_size, out_size)
    if key in _TABLES:
        return _TABLES[key]
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    rows, bnd = [], []
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w = []
        ww = 0.0
        for x in range(xmax):
            v = _bicubic((x + xmin - center + 0.5) * ss)
            w.append(v)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        row = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w]
        rows.append(row + [0] * (ksize - xmax))
        bnd.append((xmin, xmax))
    _TABLES[key] = (torch.tensor(rows, dtype=torch.int32), torch.tensor(bnd, dtype=torch.int32))
    return _TABLES[key]


def device_tables(in_size, out_size, device):
    """The tables of one axis on `device` (_consts.device_const).  An axis that keeps its size gets the one-tap identity
    table: PIL skips that pass, and since its table there is exactly [0, 1, 0, 0] the bytes are the same."""
    n, out = int(in_size), int(out_size)

    def build():
        if n != out:
            return resample_tables(n, out)
        return (torch.full((n, 1), 1 << PRECISION_BITS, dtype=torch.int32),
                torch.stack([torch.arange(n, dtype=torch.int32), torch.ones(n, dtype=torch.int32)], dim=1))
    return device_const(("resample", n, out), device, build)


# ---- the normalisation table of the image input ---------------------------------------------------------------------------

def _image_mean_std(mean, std):
    try:
        mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
    except (TypeError, ValueError):
        raise ValueError("mean and std must be 3 numbers each, got %r / %r" % (mean, std))
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("mean and std must be 3 numbers each, got %r / %r" % (mean, std))
    if any(v == 0 for v in std):
        raise ValueError("std must not be 0 (Normalize would divide by zero), got %r" % (std,))
    return mean, std


def image_norm_lut(mean, std):
    """torchvision's ToTensor + Normalize on every byte value, with torch's own float32 ops: (3, 256) float32 on the host,
    lut[c, b] = (b / 255 - mean[c]) / std[c]."""
    mean, std = _image_mean_std(mean, std)
    x = torch.arange(256).float().div(255)                   # ToTensor
    mean, std = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    return x[None].sub(mean[:, None]).div(std[:, None]).contiguous()      # Normalize: float32 tensors, as torchvision's


def _image_lut(mean, std, device):
    """image_norm_lut of a checked (mean, std) on `device`: float32 (3, 256)."""
    return device_const(("image_lut", mean, std), device, lambda: image_norm_lut(mean, std))


# ---- JPEG: the header and the tables of the encoder ----------------------------------------------------------------------

# ITU-T T.81 Annex K.1, natural (row-major) order: libjpeg's std_luminance_quant_tbl / std_chrominance_quant_tbl
JPEG_BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                  14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
JPEG_BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                    47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# Annex K.3: (table class and id of the DHT segment, bits[1..16], values), in the order libjpeg writes them
JPEG_HUFFMAN = (
    (0x00, "00010501010101010100000000000000", "000102030405060708090a0b"),
    (0x10, "0002010303020403050504040000017d",
     "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43"
     "4445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2"
     "b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"),
    (0x01, "00030101010101010101010000000000", "000102030405060708090a0b"),
    (0x11, "00020102040403040705040400010277",
     "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
     "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
     "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"),
)
JPEG_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
               28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
               54, 47, 55, 62, 63)                       # natural index of the i-th coefficient of the scan
JPEG_MODES = "baseline, 4:2:0 chroma (subsampling 2), the standard Huffman tables, quality 1..100"

_JPEG_HEADERS = {}                     # (h, w, quality) -> bytes


def _jpeg_quality(quality):
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
        raise ValueError("quality must be an int in 1..100, got %r" % (quality,))
    return quality


def jpeg_quant_tables(quality):
    """libjpeg's jpeg_set_quality: -> (luma, chroma), 64 values each in ZIGZAG order, as the DQT segments hold them and
    as the kernels divide by them (times 8, the scale of the integer DCT)."""
    q = _jpeg_quality(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(tuple(min(max((base[k] * scale + 50) // 100, 1), 255) for k in JPEG_ZIGZAG)
                 for base in (JPEG_BASE_LUMA, JPEG_BASE_CHROMA))


def _jpeg_segment(marker, body):
    return bytes((0xFF, marker)) + (len(body) + 2).to_bytes(2, "big") + body


def jpeg_header(h, w, quality=75):
    """The file up to and including SOS, in PIL's layout: SOI, JFIF 1.1 APP0 (unit 0, density 1 x 1), the two DQT
    segments, SOF0 with sampling 2x2 / 1x1 / 1x1, the four DHT segments, SOS.  Host only, cached."""
    h, w, quality = int(h), int(w), _jpeg_quality(quality)
    if not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError("a JPEG frame is 1..65535 pixels on each side, got %d x %d" % (h, w))
    key = (h, w, quality)
    if key not in _JPEG_HEADERS:
        out = b"\xff\xd8" + _jpeg_segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
        for i, table in enumerate(jpeg_quant_tables(quality)):
            out += _jpeg_segment(0xDB, bytes((i,)) + bytes(table))
        out += _jpeg_segment(0xC0, b"\x08" + h.to_bytes(2, "big") + w.to_bytes(2, "big")
                             + b"\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01")
        for tc_th, bits, vals in JPEG_HUFFMAN:
            out += _jpeg_segment(0xC4, bytes((tc_th,)) + bytes.fromhex(bits) + bytes.fromhex(vals))
        _JPEG_HEADERS[key] = out + _jpeg_segment(0xDA, b"\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00")
    return _JPEG_HEADERS[key]


def jpeg_tables(quality=75):
    """What dd_jpeg_encode_u8 takes as `tables` (include/dualdiff_hip.h): int32 (672,) = the two quantisation tables of
    jpeg_quant_tables, then per Huffman table of JPEG_HUFFMAN's DC pair and AC pair the entry (code << 8) | length of
    every symbol (0 for a symbol the table does not have); codes assigned as T.81 Annex C does."""
    words = [v for table in jpeg_quant_tables(quality) for v in table]
    for want in (0x00, 0x01, 0x10, 0x11):                # dc luma, dc chroma, ac luma, ac chroma
        _, bits, vals = next(t for t in JPEG_HUFFMAN if t[0] == want)
        bits, vals = bytes.fromhex(bits), bytes.fromhex(vals)
        entries = [0] * (16 if want < 0x10 else 256)
        code = k = 0
        for length in range(1, 17):
            for _ in range(bits[length - 1]):
                entries[vals[k]] = (code << 8) | length
                code += 1
                k += 1
            code <<= 1
        words += entries
    return torch.tensor(words, dtype=torch.int32)


def device_jpeg_tables(h, w, quality, device):
    """(header uint8 (len,), tables int32 (672,)) of one (h, w, quality) on `device` (_consts.device_const)."""
    def build():
        return torch.frombuffer(bytearray(jpeg_header(h, w, quality)), dtype=torch.uint8), jpeg_tables(quality)
    return device_const(("jpeg", int(h), int(w), int(quality)), device, build)


# ---- PNG: what is built, and the sizes of its format (csrc/png.hip) ---------------------------------

PNG_MODES = "8-bit RGB (colour type 2), no interlace, no ancillary chunks"
PNG_CHUNK = 16384                      # filtered bytes per deflate chunk and per IDAT
PNG_FILE_FIXED = 8 + 25 + 12 + 2 + 4   # signature, IHDR, IEND, the zlib header, the Adler-32
PNG_CHUNK_FIXED = 12 + 5               # an IDAT's length / type / CRC, a stored block's header


def png_unit_lut():
    """torchvision's ToTensor on every byte value, with torch's own float32 division: (256,) float32 on the host,
    lut[b] = float32(b) / 255 — what the image-mode ORS condition is made of (ops.png_condition)."""
    return torch.arange(256).float().div(255).contiguous()


BILINEAR_MAX = 1 << 14                 # sizes up to which bilinear_tables' float64 steps are exact (below)
_BILINEAR = {}                         # (in, out) -> (taps int32 (out, 2), weights float32 (out, 2))


def bilinear_tables(in_size, out_size):
    """One axis of `F.interpolate(mode="bilinear", align_corners=False)` without antialias, in float32 as torch's CPU
    kernel computes it: -> (taps int32 (out_size, 2) = [i0, i1], weights float32 (out_size, 2) = [l0, l1]); output d is
    `l0 * x[i0] + l1 * x[i1]`.  scale = float32(in) / float32(out); src = fma(scale, float32(d) + 0.5, -0.5), negative
    -> 0; i0 = int(src), i1 = i0 + (i0 < in - 1); l1 = clamp(src - i0, 0, 1), l0 = 1 - l1.  The fused multiply-add is
    taken in float64 and rounded once: for sizes up to BILINEAR_MAX the product of the 24-bit scale and d + 0.5 (15 bits)
    and its sum with -0.5 both fit 53 bits, so float64 holds them exactly.  The unfused float32 form differs (by up to
    4e-6 in the result at 225 -> 216) and is not what torch computes."""
    import numpy as np
    in_size, out_size = int(in_size), int(out_size)
    if not (0 < in_size <= BILINEAR_MAX and 0 < out_size <= BILINEAR_MAX):
        raise ValueError("sizes must be in 1..%d, got %d -> %d" % (BILINEAR_MAX, in_size, out_size))
    key = (in_size, out_size)
    if key not in _BILINEAR:
        f32 = np.float32
        scale = f32(in_size) / f32(out_size)
        dst = np.arange(out_size, dtype=f32) + f32(0.5)
        src = (np.float64(scale) * dst.astype(np.float64) - 0.5).astype(f32)
        src = np.maximum(src, f32(0))
        i0 = np.minimum(src.astype(np.int32), in_size - 1)
        i1 = i0 + (i0 < in_size - 1)
        l1 = np.clip(src - i0.astype(f32), f32(0), f32(1)).astype(f32)
        l0 = (f32(1) - l1).astype(f32)
        _BILINEAR[key] = (torch.from_numpy(np.stack([i0, i1], axis=1).astype(np.int32)),
                          torch.from_numpy(np.stack([l0, l1], axis=1).astype(f32)))
    return _BILINEAR[key]


def device_bilinear_tables(in_size, out_size, device):
    """bilinear_tables of one axis on `device` (_consts.device_const)."""
    n, out = int(in_size), int(out_size)
    return device_const(("bilinear", n, out), device, lambda: bilinear_tables(n, out))


def png_capacity(h, w, channels=3):
    """The longest file of an (h, w) frame of 3 (RGB) or 4 (RGBA) channels: every chunk stored.  No content makes a file
    longer."""
    n = int(h) * (1 + int(channels) * int(w))
    return PNG_FILE_FIXED + PNG_CHUNK_FIXED * (-(-n // PNG_CHUNK)) + n
