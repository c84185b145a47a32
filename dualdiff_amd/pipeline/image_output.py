"""Image output on the GPU: the decoded views as the uint8 frames the reference saves.

What the reference does after `decode_latents` in the run that produces its generated validation set
(perception/data_prepare/val_set_gen.py):

1. `image.cpu().permute(0, 2, 3, 1).float().numpy()` (pipeline/pipeline_bev_controlnet.py:112),
2. diffusers' `numpy_to_pil`, `(images * 255).round().astype("uint8")` (:540, `numpy_to_pil_double` :72-80),
3. per view `torchvision.transforms.Resize(cfg.fid.resize, interpolation=BICUBIC)` and `Pad(cfg.fid.padding)` on the PIL
   image (val_set_gen.py:147-159, applied at :44) — `dataset.back_resize` / `back_pad`, by default 224 x 400 -> 896 x 1600
   and four rows on top (configs/dataset/Nuscenes.yaml:35-36).

Here that is one launch per batch of views (`ops.image_resample_u8`, or `ops.image_quantize_u8` for `raw_output: true`), byte
for byte: PIL resamples 8-bit images in integer arithmetic over fixed-point coefficient tables, and the only floating
point, the construction of those tables, is done here in Python float64 exactly as PIL's C does it in double.

    post = ImagePostProcess.from_config(cfg)              # cfg.fid.resize / cfg.fid.padding / cfg.fid.raw_output
    frames = decode_images(vae, latents, post)            # (b, n_cam, H, W, 3) uint8, on the GPU
    pil = to_pil(frames)                                  # the 2-level list numpy_to_pil_double returns

The reference then saves every view with `post_trans(img).save(<nuScenes name>.jpg)` and no options (val_set_gen.py:44,
tools/downstream_v3_batched.py:244-252): libjpeg's baseline encoder at quality 75, 4:2:0 chroma, the standard Huffman
tables.  That is integer arithmetic too, and `ops.jpeg_encode_u8` produces the same bytes on the device:

    files = encode_jpeg(frames)                           # the 2-level list of `bytes`, one .jpg file each
    save_jpeg(frames, paths)                              # ... written to `paths` (same nesting), directories created

File decoding, PNG and FID stay with the caller.
"""
import math
import os

import torch

from .. import ops as O

PRECISION_BITS = 32 - 8 - 2            # PIL's fixed point for 8-bit pixels
INTERPOLATIONS = ("bicubic",)

_TABLES = {}                           # (in, out) -> (kk int32 (out, ksize), bounds int32 (out, 2))
_DEVICE_TABLES = {}                    # (in, out, device) -> the same on the device


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
    """The tables of one axis on `device`, cached.  An axis that keeps its size gets the one-tap identity table: PIL skips
    that pass, and since its table there is exactly [0, 1, 0, 0] the bytes are the same."""
    device = torch.device(device)
    key = (int(in_size), int(out_size), device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _DEVICE_TABLES:
        if key[0] == key[1]:
            kk = torch.full((key[0], 1), 1 << PRECISION_BITS, dtype=torch.int32)
            bounds = torch.stack([torch.arange(key[0], dtype=torch.int32), torch.ones(key[0], dtype=torch.int32)], dim=1)
        else:
            kk, bounds = resample_tables(*key[:2])
        _DEVICE_TABLES[key] = (kk.contiguous().to(device), bounds.contiguous().to(device))
    return _DEVICE_TABLES[key]


def _get(cfg, name, default=None):
    if hasattr(cfg, "get"):
        return cfg.get(name, default)
    return getattr(cfg, name, default)


class ImagePostProcess:
    """The reference's `post_trans` (val_set_gen.py:147-159) on GPU tensors: images (b, n, 3, h, w) or (m, 3, h, w) in
    [0, 1] -> uint8 (b, n, H, W, 3) / (m, H, W, 3).  resize = (h, w) or None (`raw_output: true`: quantise only, padding
    is not applied either, as in the reference); padding = torchvision.transforms.Pad's int / pair / (left, top, right,
    bottom)."""

    def __init__(self, resize=None, padding=None, interpolation="bicubic"):
        if str(interpolation).lower() not in INTERPOLATIONS:
            raise ValueError("interpolation %r is not built; available: %s" % (interpolation, ", ".join(INTERPOLATIONS)))
        if resize is not None:
            if isinstance(resize, int):
                raise ValueError("resize must be (h, w); the shorter-edge form of Resize(int) is not built")
            resize = tuple(int(v) for v in resize)
            if len(resize) != 2 or min(resize) <= 0:
                raise ValueError("resize must be a positive (h, w), got %r" % (resize,))
        elif padding is not None:
            raise ValueError("padding without resize: raw output is not padded (val_set_gen.py:147-148)")
        self.resize = resize
        self.padding = O.image_padding(0 if padding is None else padding)

    @classmethod
    def from_config(cls, cfg):
        """cfg: any mapping (or object) with `fid.resize`, `fid.padding`, `fid.raw_output` — the reference's test config."""
        fid = _get(cfg, "fid")
        if fid is None:
            raise ValueError("config has no `fid` section")
        if _get(fid, "raw_output", False):
            return cls()
        resize = _get(fid, "resize")
        if resize is None:
            raise ValueError("config has no fid.resize (and fid.raw_output is false)")
        padding = _get(fid, "padding")
        return cls(resize=list(resize), padding=None if padding is None else (padding if isinstance(padding, int) else list(padding)))

    def __call__(self, images, m11=False):
        if images.dim() not in (4, 5):
            raise ValueError("images must be (b, n, 3, h, w) or (m, 3, h, w), got %s" % (tuple(images.shape),))
        x = images.flatten(0, 1) if images.dim() == 5 else images
        x = x.contiguous()
        if self.resize is None:
            y = O.image_quantize_u8(x, m11=m11)
        else:
            y = O.image_resample_u8(x, self.resize, self.padding, m11=m11)
        return y.view(*images.shape[:2], *y.shape[1:]) if images.dim() == 5 else y


@torch.no_grad()
def decode_images(vae, latents, post=None):
    """latents (b, n_cam, 4, h, w) -> uint8 frames (b, n_cam, H, W, 3) on the GPU: `post(decode_latents(vae, latents))`
    byte for byte, with the decoder's output going straight into the kernel (its `/ 2 + 0.5`, clamp and quantisation
    happen on load; neither the fp32 images nor a uint8 copy at the decoder's size is written)."""
    post = ImagePostProcess() if post is None else post
    b = latents.shape[0]
    img = vae.decode(latents.flatten(0, 1), pre_scale=1.0 / vae.scaling_factor)
    return post(img.view(b, -1, *img.shape[1:]), m11=True)


def to_pil(u8):
    """uint8 frames (b, n, H, W, 3) -> the 2-level list of PIL images `numpy_to_pil_double` returns
    (pipeline_bev_controlnet.py:72-80); (m, H, W, 3) -> a flat list.  The one place that needs PIL."""
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("to_pil needs Pillow (PIL), which is not installed; the uint8 frames themselves do not") from e
    if u8.dtype != torch.uint8 or u8.dim() not in (4, 5) or u8.shape[-1] != 3:
        raise ValueError("to_pil takes uint8 frames (b, n, H, W, 3) or (m, H, W, 3), got %s %s" % (tuple(u8.shape), u8.dtype))
    arr = u8.cpu().numpy()
    if arr.ndim == 4:
        return [Image.fromarray(a) for a in arr]
    return [[Image.fromarray(a) for a in scene] for scene in arr]


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
_JPEG_DEVICE = {}                      # (h, w, quality, device) -> (header uint8, tables int32) on the device


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
    """(header uint8 (len,), tables int32 (672,)) of one (h, w, quality) on `device`, cached as device_tables does."""
    device = torch.device(device)
    key = (int(h), int(w), int(quality), device.type,
           device.index if device.index is not None else torch.cuda.current_device())
    if key not in _JPEG_DEVICE:
        header = torch.frombuffer(bytearray(jpeg_header(h, w, quality)), dtype=torch.uint8)
        _JPEG_DEVICE[key] = (header.to(device), jpeg_tables(quality).to(device))
    return _JPEG_DEVICE[key]


def _jpeg_options(options):
    for name, value in options.items():
        raise ValueError("JPEG option %s=%r is not built; available: %s" % (name, value, JPEG_MODES))


@torch.no_grad()
def encode_jpeg(u8, quality=75, **options):
    """uint8 frames (b, n, H, W, 3) -> the 2-level list of `bytes` (one .jpg file per view, nested as to_pil nests its
    images), (m, H, W, 3) -> a flat list: what `Image.fromarray(frame).save(f, "JPEG", quality=quality)` writes, byte
    for byte, encoded on the GPU.  One readback of the lengths and one copy of the files' bytes; should a file not fit
    the default capacity (header + H * W bytes), the call is repeated once with the capacity the lengths ask for."""
    _jpeg_options(options)
    if u8.dtype != torch.uint8 or u8.dim() not in (4, 5) or u8.shape[-1] != 3:
        raise ValueError("encode_jpeg takes uint8 frames (b, n, H, W, 3) or (m, H, W, 3), got %s %s" % (tuple(u8.shape), u8.dtype))
    frames = (u8.flatten(0, 1) if u8.dim() == 5 else u8).contiguous()
    buf, lengths = O.jpeg_encode_u8(frames, quality)
    n = lengths.cpu().tolist()
    if max(n) > buf.shape[1]:
        buf, lengths = O.jpeg_encode_u8(frames, quality, capacity=max(n))
        n = lengths.cpu().tolist()
    raw = buf[:, :max(n)].cpu().numpy()
    files = [raw[i, :k].tobytes() for i, k in enumerate(n)]
    if u8.dim() == 4:
        return files
    per = u8.shape[1]
    return [files[i * per:(i + 1) * per] for i in range(u8.shape[0])]


def save_jpeg(u8, paths, quality=75, **options):
    """encode_jpeg, each file written to its path: `paths` nested as the frames are ((b, n) names, or m names).  Missing
    directories are created, as the reference's `mkdir -p` does.  Returns the files' sizes, nested the same way."""
    files = encode_jpeg(u8, quality, **options)
    nested = u8.dim() == 5
    rows = list(zip(files, paths)) if nested else [(files, paths)]
    if len(paths) != len(files) or any(len(p) != len(f) for f, p in rows):
        raise ValueError("save_jpeg takes one path per frame, nested as the frames are")
    sizes = []
    for fs, ps in rows:
        for data, path in zip(fs, ps):
            path = os.fspath(path)
            if os.path.dirname(path):
                os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "wb") as f:
                f.write(data)
        sizes.append([len(d) for d in fs])
    return sizes if nested else sizes[0]
