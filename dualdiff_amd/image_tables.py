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


# ---- the colour map of the attention heat maps (csrc/attn_heat.hip, pipeline/attn_output.py) ---------------------------

# matplotlib's "coolwarm" as bytes: (cmap(arange(256))[:, :3] * 255).astype(uint8) of matplotlib 3.10, computed once and
# kept as data so that nothing needs matplotlib at run time (tests/test_attn_output_cpu.py compares it where matplotlib
# is installed)
COOLWARM_U8 = (
    (58, 76, 192), (59, 77, 193), (60, 79, 195), (62, 81, 196), (63, 83, 198), (64, 84, 199), (65, 86, 201), (66, 88, 202),
    (67, 90, 204), (69, 91, 205), (70, 93, 207), (71, 95, 208), (72, 96, 209), (73, 98, 211), (75, 100, 212), (76, 102, 214),
    (77, 103, 215), (78, 105, 216), (80, 107, 218), (81, 108, 219), (82, 110, 220), (83, 112, 221), (85, 113, 222), (86, 115, 224),
    (87, 117, 225), (88, 118, 226), (90, 120, 227), (91, 121, 228), (92, 123, 229), (93, 125, 230), (95, 126, 231), (96, 128, 232),
    (97, 130, 234), (99, 131, 234), (100, 133, 235), (101, 134, 236), (103, 136, 237), (104, 137, 238), (105, 139, 239), (107, 141, 240),
    (108, 142, 241), (109, 144, 241), (111, 145, 242), (112, 147, 243), (113, 148, 244), (115, 149, 244), (116, 151, 245), (117, 152, 246),
    (119, 154, 246), (120, 155, 247), (122, 157, 248), (123, 158, 248), (124, 160, 249), (126, 161, 249), (127, 162, 250), (128, 164, 250),
    (130, 165, 251), (131, 166, 251), (133, 168, 251), (134, 169, 252), (135, 170, 252), (137, 172, 252), (138, 173, 253), (139, 174, 253),
    (141, 175, 253), (142, 177, 253), (144, 178, 254), (145, 179, 254), (146, 180, 254), (148, 181, 254), (149, 183, 254), (151, 184, 254),
    (152, 185, 254), (153, 186, 254), (155, 187, 254), (156, 188, 254), (157, 189, 254), (159, 190, 254), (160, 191, 254), (162, 192, 254),
    (163, 193, 254), (164, 194, 254), (166, 195, 253), (167, 196, 253), (168, 197, 253), (170, 198, 253), (171, 199, 252), (172, 200, 252),
    (174, 201, 252), (175, 202, 251), (176, 203, 251), (178, 203, 251), (179, 204, 250), (180, 205, 250), (182, 206, 249), (183, 207, 249),
    (184, 207, 248), (185, 208, 248), (187, 209, 247), (188, 209, 246), (189, 210, 246), (190, 211, 245), (192, 211, 245), (193, 212, 244),
    (194, 212, 243), (195, 213, 242), (197, 213, 242), (198, 214, 241), (199, 214, 240), (200, 215, 239), (201, 215, 238), (202, 216, 238),
    (204, 216, 237), (205, 217, 236), (206, 217, 235), (207, 217, 234), (208, 218, 233), (209, 218, 232), (210, 218, 231), (211, 219, 230),
    (213, 219, 229), (214, 219, 228), (215, 219, 226), (216, 219, 225), (217, 220, 224), (218, 220, 223), (219, 220, 222), (220, 220, 221),
    (221, 220, 219), (222, 219, 218), (223, 219, 217), (224, 218, 215), (225, 218, 214), (226, 217, 212), (227, 217, 211), (228, 216, 209),
    (229, 216, 208), (230, 215, 207), (231, 214, 205), (231, 214, 204), (232, 213, 202), (233, 212, 201), (234, 211, 199), (235, 211, 198),
    (236, 210, 196), (236, 209, 195), (237, 208, 193), (237, 207, 192), (238, 207, 190), (239, 206, 188), (239, 205, 187), (240, 204, 185),
    (241, 203, 184), (241, 202, 182), (242, 201, 181), (242, 200, 179), (242, 199, 178), (243, 198, 176), (243, 197, 175), (244, 196, 173),
    (244, 195, 171), (244, 194, 170), (245, 193, 168), (245, 192, 167), (245, 191, 165), (246, 189, 164), (246, 188, 162), (246, 187, 160),
    (246, 186, 159), (246, 185, 157), (246, 183, 156), (246, 182, 154), (247, 181, 152), (247, 179, 151), (247, 178, 149), (247, 177, 148),
    (247, 176, 146), (247, 174, 145), (247, 173, 143), (246, 171, 141), (246, 170, 140), (246, 169, 138), (246, 167, 137), (246, 166, 135),
    (246, 164, 134), (246, 163, 132), (245, 161, 130), (245, 160, 129), (245, 158, 127), (244, 157, 126), (244, 155, 124), (244, 154, 123),
    (243, 152, 121), (243, 150, 120), (243, 149, 118), (242, 147, 117), (242, 145, 115), (241, 144, 114), (241, 142, 112), (240, 141, 111),
    (240, 139, 109), (239, 137, 108), (238, 135, 106), (238, 134, 105), (237, 132, 103), (236, 130, 102), (236, 128, 100), (235, 127, 99),
    (234, 125, 97), (234, 123, 96), (233, 121, 94), (232, 119, 93), (231, 117, 92), (230, 116, 90), (230, 114, 89), (229, 112, 87),
    (228, 110, 86), (227, 108, 84), (226, 106, 83), (225, 104, 82), (224, 102, 80), (223, 100, 79), (222, 98, 78), (221, 96, 76),
    (220, 94, 75), (219, 92, 74), (218, 90, 72), (217, 88, 71), (216, 86, 70), (215, 84, 68), (214, 82, 67), (212, 79, 66),
    (211, 77, 64), (210, 75, 63), (209, 73, 62), (207, 70, 61), (206, 68, 60), (205, 66, 58), (204, 63, 57), (202, 61, 56),
    (201, 59, 55), (200, 56, 53), (198, 53, 52), (197, 50, 51), (196, 48, 50), (194, 45, 49), (193, 42, 48), (191, 40, 46),
    (190, 35, 45), (188, 31, 44), (187, 26, 43), (185, 22, 42), (184, 17, 41), (182, 13, 40), (181, 8, 39), (179, 3, 38),
)
CMAPS = {"coolwarm": COOLWARM_U8}
CMAP_BAD_U8 = (0, 0, 0)                 # matplotlib's "bad" colour (0, 0, 0, 0) behind `[:3]`: what a NaN pixel gets


def cmap_bytes(cmap):
    """A colour map as a tuple of 256 (r, g, b) byte triples: a name of CMAPS, or any (256, 3) uint8 table (an ndarray, a
    tensor or nested sequences) — e.g. `(plt.get_cmap(name)(np.arange(256))[:, :3] * 255).astype(np.uint8)`."""
    if isinstance(cmap, str):
        if cmap not in CMAPS:
            raise ValueError("colour map %r is not built in (%s): pass its (256, 3) uint8 table" % (cmap, ", ".join(sorted(CMAPS))))
        return CMAPS[cmap]
    dtype = getattr(cmap, "dtype", None)
    if dtype is not None and str(dtype) not in ("uint8", "torch.uint8"):
        raise ValueError("a colour-map table must be uint8, got %s" % (dtype,))
    rows = cmap.tolist() if hasattr(cmap, "tolist") else cmap
    try:
        rows = tuple(tuple(v for v in row) for row in rows)
    except TypeError:
        raise ValueError("a colour map is a name or a (256, 3) uint8 table, got %r" % (type(cmap).__name__,))
    if len(rows) != 256 or any(len(row) != 3 for row in rows):
        raise ValueError("a colour-map table must be (256, 3)")
    if any(isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 255 for row in rows for v in row):
        raise ValueError("a colour-map table must hold bytes")
    return rows


def cmap_table(cmap):
    """What dd_attn_heat takes as `table`: (257, 4) float32 on the host, row k = colour byte / 255 of index k with torch's
    own float32 division (the quotient dd_image_resample_u8's quantiser returns the byte for), row 256 the NaN colour,
    the fourth column unused."""
    rows = cmap_bytes(cmap) + (CMAP_BAD_U8,)
    out = torch.zeros((257, 4), dtype=torch.float32)
    out[:, :3] = torch.tensor(rows, dtype=torch.float32).div(255)
    return out


def device_cmap_table(cmap, device):
    """cmap_table on `device` (_consts.device_const), keyed by the name or by the table's bytes."""
    key = cmap if isinstance(cmap, str) else cmap_bytes(cmap)
    return device_const(("attn_cmap", key), device, lambda: cmap_table(key))


def png_capacity(h, w, channels=3):
    """The longest file of an (h, w) frame of 3 (RGB) or 4 (RGBA) channels: every chunk stored.  No content makes a file
    longer."""
    n = int(h) * (1 + int(channels) * int(w))
    return PNG_FILE_FIXED + PNG_CHUNK_FIXED * (-(-n // PNG_CHUNK)) + n
