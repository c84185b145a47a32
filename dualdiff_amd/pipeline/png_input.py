"""PNG input on the GPU: .png files -> uint8 frames, and the image-mode ORS condition made of them.

With `use_occ_3d=False` (the DualDiff default for both ControlNet branches) the ORS condition of a sample is one .png, an
RGBA panorama of the six views, that the reference opens with PIL on the host (`OccFolderSetWrapper(mode='image')`,
magicdrive/dataset/dataset_wrapper.py:62-81, misc/test_utils.py:218-222: `ToTensor()(Image.open(f).convert("RGB"))`) and
that `collate_fn` stacks and, for 256 x 704, crops per view and, for 192 x 384, pads, resizes and crops per view
(dataset/utils.py:348-408; ResizedOccCondition, one launch of `ops.png_condition_resized`).  Here the host walks each file's
chunks — framing and checksums, not the compressed bytes — and the device does the rest in one call per batch
(`ops.png_decode_u8`): inflate, the Adler-32, the five row filters and the conversion to RGB, so the frames equal
`np.asarray(Image.open(f).convert("RGB"))` byte for byte.  The files `encode_png` / `save_png` write come back the same
way, their 16 KiB chunks decoded side by side where the device can verify that this is the sequential decode.

    frames = load_png(paths)                              # (b, n, H, W, 3) uint8 on the GPU; paths nested (b, n), or flat
    frames = decode_png(files)                            # ... from `bytes`
    cond = occ_condition_from_config(cfg)(files)          # (b, 3, h, 6 w) float32: `controlnet_cond` of the default mode,
                                                          # for every image_size the reference configures

What is built is PNG_INPUT_MODES; any other file is turned down on the host with a ValueError that names the frame and
what was found, before anything is uploaded, and is the caller's to decode (with PIL).  This module does not import PIL.
"""
import os
import struct
import zlib

import numpy as np
import torch

from .. import ops as O

PNG_INPUT_MODES = "bit depth 8, no interlace, colour type 0 (grey), 2 (RGB) or 6 (RGBA, alpha dropped), one image per file"
SIGNATURE = b"\x89PNG\r\n\x1a\n"
_COLOUR_NAMES = {3: "a palette image (colour type 3)", 4: "grey with alpha (colour type 4)"}
_KNOWN_CRITICAL = (b"IHDR", b"PLTE", b"IDAT", b"IEND")


class PngInfo:
    """What parse_png found: h, w; colour_type (0 / 2 / 6); idats [(offset, length)], the payload of every IDAT chunk in
    the file's order, empty ones included; chunked: the file has the shape of encode_png's own format (colour type 2,
    exactly ceil(h (1 + 3 w) / 16384) IDATs, none of them empty, room for the zlib header in the first and for the
    Adler-32 in the last) — a shape a foreign file can have too, so the device verifies before it relies on it."""
    __slots__ = ("h", "w", "colour_type", "idats", "chunked")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])


def _refuse(frame, found):
    where = "" if frame is None else "frame %d: " % frame
    raise ValueError("%s%s is not built; available: %s" % (where, found, PNG_INPUT_MODES))


def _broken(frame, what):
    raise ValueError("%s%s" % ("" if frame is None else "frame %d: " % frame, what))


def parse_png(data, frame=None):
    """A walk over the chunks of one file -> PngInfo.  Checked: the signature; IHDR first, with compression method 0 and
    filter method 0; IEND last; at least one IDAT, the IDATs consecutive; every chunk's CRC (zlib.crc32 — a checksum, not
    a decode).  Ancillary chunks are skipped, as PIL's convert("RGB") ignores them.  Raises ValueError (with `frame`, when
    given, in front) for a file that is broken or of a kind that is not built."""
    data = data if isinstance(data, (bytes, bytearray)) else bytes(data)
    n = len(data)
    if data[:8] != SIGNATURE:
        _refuse(frame, "a file that is not a PNG (no PNG signature)")
    pos, head, idats, seen_idat, idat_closed, ended = 8, None, [], False, False, False
    while pos < n:
        if ended:
            _broken(frame, "%d bytes behind the IEND chunk" % (n - pos))
        if pos + 12 > n:
            _broken(frame, "the chunk at byte %d is cut short" % pos)
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        if pos + 12 + length > n:
            _broken(frame, "chunk %s at byte %d is cut short" % (kind.decode("latin-1"), pos))
        body = pos + 8
        if zlib.crc32(data[pos + 4:body + length]) != struct.unpack(">I", data[body + length:body + length + 4])[0]:
            _broken(frame, "chunk %s at byte %d: the CRC does not match" % (kind.decode("latin-1"), pos))
        if head is None:
            if kind != b"IHDR" or length != 13:
                _broken(frame, "the first chunk is not a 13-byte IHDR")
            head = struct.unpack(">IIBBBBB", data[body:body + 13])
        elif kind == b"IHDR":
            _broken(frame, "a second IHDR chunk")
        elif kind == b"IDAT":
            if idat_closed:
                _broken(frame, "IDAT chunks that are not consecutive")
            seen_idat = True
            idats.append((body, length))
        elif kind == b"IEND":
            ended = True
        elif kind == b"acTL":
            _refuse(frame, "an animated PNG (acTL)")
        elif not (kind[0] & 32) and kind not in _KNOWN_CRITICAL:
            _refuse(frame, "the critical chunk %s" % kind.decode("latin-1"))
        if seen_idat and kind != b"IDAT":
            idat_closed = True
        pos = body + length + 4
    if head is None:
        _broken(frame, "no IHDR chunk")
    if not ended:
        _broken(frame, "no IEND chunk at the end of the file")
    w, h, depth, colour, compression, filtering, interlace = head
    if compression != 0 or filtering != 0:
        _broken(frame, "IHDR names compression method %d, filter method %d (PNG has 0, 0)" % (compression, filtering))
    if colour in _COLOUR_NAMES:
        _refuse(frame, _COLOUR_NAMES[colour])
    if colour not in O.PNG_DECODE_COLOUR_TYPES:
        _broken(frame, "IHDR names colour type %d" % colour)
    if depth != 8:
        _refuse(frame, "%d-bit samples" % depth)
    if interlace != 0:
        _refuse(frame, "Adam7 interlace")
    if w == 0 or h == 0:
        _broken(frame, "a frame of %d x %d" % (h, w))
    if not idats:
        _broken(frame, "no IDAT chunk")
    want = -(-(h * (1 + 3 * w)) // O.PNG_DECODE_CHUNK)
    chunked = (colour == 2 and len(idats) == want and all(length > 0 for _, length in idats)
               and idats[0][1] >= 2 and idats[-1][1] >= 4 and sum(length for _, length in idats) >= 6)
    return PngInfo(h=h, w=w, colour_type=colour, idats=idats, chunked=chunked)


def _flatten(files):
    if isinstance(files, (bytes, bytearray, memoryview)) or not len(files):
        raise ValueError("decode_png takes a list of files (bytes), flat or nested (b, n)")
    if isinstance(files[0], (bytes, bytearray, memoryview)):
        return list(files), None
    per = len(files[0])
    if per == 0 or any(len(row) != per for row in files):
        raise ValueError("decode_png takes a (b, n) list with the same n in every row")
    return [f for row in files for f in row], (len(files), per)


def upload_png(files, device="cuda"):
    """A flat list of files -> what ops.png_decode_u8 takes, after ONE host-to-device copy (from pinned memory, not waited
    for): (streams, files, tab, colour_types, h, w), the three tensors views of the one upload.  A file's stream is its
    IDAT payloads one behind the other, chunk framing stripped; `files` holds per file the stream's offset and length, the
    colour type and, for a file of encode_png's shape, the place in `tab` of its IDAT boundaries (else -1).  Every file is
    parsed, and refused if need be, before anything is allocated."""
    infos = []
    for i, f in enumerate(files):
        if not isinstance(f, (bytes, bytearray, memoryview)):
            raise ValueError("frame %d: a file is `bytes`, got %s" % (i, type(f).__name__))
        infos.append(parse_png(f, frame=i))
    first = infos[0]
    for i, info in enumerate(infos):
        if (info.h, info.w) != (first.h, first.w):
            raise ValueError("frame %d: %d x %d differs from frame 0 (%d x %d); the frames of one call have one geometry"
                             % (i, info.h, info.w, first.h, first.w))
    m = len(files)
    lens = [sum(length for _, length in info.idats) for info in infos]
    ntab = sum(len(info.idats) + 1 for info in infos if info.chunked)
    head = (16 * m + 4 * ntab + 15) // 16 * 16               # files | tab
    total = head + sum(lens)
    if total >= 1 << 31:
        raise ValueError("the streams of one call are at most 2 GiB, got %d bytes" % total)
    device = torch.device(device)
    host = torch.empty(total + 1, dtype=torch.uint8, pin_memory=device.type == "cuda")
    raw = host.numpy()
    table = raw[:16 * m].view("<i4").reshape(m, 4)
    tab = raw[16 * m:16 * m + 4 * ntab].view("<i4")
    at = tab_at = 0
    for i, (f, info) in enumerate(zip(files, infos)):
        table[i] = (at, lens[i], info.colour_type, tab_at if info.chunked else -1)
        src = np.frombuffer(f, dtype=np.uint8)
        rel = 0
        for k, (offset, length) in enumerate(info.idats):
            raw[head + at + rel:head + at + rel + length] = src[offset:offset + length]
            if info.chunked:
                tab[tab_at + k] = rel
            rel += length
        if info.chunked:
            tab[tab_at + len(info.idats)] = rel
            tab_at += len(info.idats) + 1
        at += lens[i]
    dev = host.to(device, non_blocking=True)
    return (dev[head:], dev[:16 * m].view(torch.int32).view(m, 4),
            dev[16 * m:16 * m + 4 * ntab].view(torch.int32) if ntab else None,
            [info.colour_type for info in infos], first.h, first.w)


def _status_text(bits):
    return ", ".join(text for bit, text in O.PNG_DECODE_STATUS if bits & bit) or "status %d" % bits


@torch.no_grad()
def decode_png(files, device="cuda", check=True, chunked=None):
    """A flat list of PNG files (`bytes`) -> uint8 frames (m, H, W, 3) on `device`, a (b, n) nested list -> (b, n, H, W,
    3): `np.asarray(Image.open(f).convert("RGB"))` of every file, byte for byte, decoded on the GPU (colour type 6 drops
    alpha, colour type 0 replicates grey).  One pinned upload and one call into the library per batch.  check=True reads
    the per-frame status back and raises ValueError for the first frame whose stream was broken; check=False does not
    synchronise and returns (frames, status), status int32 (m,) / (b, n) on the device, 0 for a good frame.  chunked=False
    sends every file through the sequential path (ops.png_decode_u8); the frames do not depend on it.  Files of a kind
    that is not built (PNG_INPUT_MODES) raise ValueError before anything is uploaded."""
    flat, nest = _flatten(files)
    streams, table, tab, colour_types, h, w = upload_png(flat, device)
    frames, status, _ = O.png_decode_u8(streams, table, tab, colour_types, h, w, chunked=chunked)
    if check:
        for i, s in enumerate(status.cpu().tolist()):
            if s:
                raise ValueError("frame %d: the stream does not decode: %s" % (i, _status_text(s)))
    if nest is not None:
        frames, status = frames.view(*nest, h, w, 3), status.view(*nest)
    return frames if check else (frames, status)


def load_png(paths, device="cuda", check=True, chunked=None):
    """decode_png of the files at `paths` (flat, or nested (b, n))."""
    def read(p):
        with open(os.fspath(p), "rb") as f:
            return f.read()
    if not len(paths):
        raise ValueError("load_png takes a list of paths, flat or nested (b, n)")
    nested = not isinstance(paths[0], (str, bytes, os.PathLike))
    files = [[read(p) for p in row] for row in paths] if nested else [read(p) for p in paths]
    return decode_png(files, device=device, check=check, chunked=chunked)


class OccCondition:
    """The collate step of the image-mode ORS condition (dataset/utils.py:348-408): the samples' panoramas stacked, each
    of the `views` views cropped from in_hw = (H, W / views) to out_hw = (h, w) as `hd_crop` does — the top H - h rows and
    (W / views - w) // 2 columns on each side dropped — and the views side by side again, as `ToTensor()` values:
    float32 (b, 3, h, views * w) on the device, ready for `ControlNetConditioningEmbedding.run` /
    `BEVControlNetModel.forward(controlnet_cond=...)`.  in_hw = out_hw = None: no crop."""

    def __init__(self, views=6, in_hw=None, out_hw=None):
        if isinstance(views, bool) or not isinstance(views, int) or views <= 0:
            raise ValueError("views must be a positive int, got %r" % (views,))
        if (in_hw is None) != (out_hw is None):
            raise ValueError("in_hw and out_hw come together (or neither: no crop)")
        self.views, self.in_hw, self.out_hw = views, None, None
        if in_hw is not None:
            (ih, iw), (oh, ow) = (int(v) for v in in_hw), (int(v) for v in out_hw)
            if not (0 < oh <= ih and 0 < ow <= iw) or (iw - ow) % 2:
                raise ValueError("out_hw %r must fit in_hw %r, the width difference even (hd_crop asserts the result's shape)"
                                 % (tuple(out_hw), tuple(in_hw)))
            self.in_hw, self.out_hw = (ih, iw), (oh, ow)

    @classmethod
    def from_config(cls, cfg):
        """cfg.dataset.image_size (attributes or mappings) -> the crop collate_fn applies for it."""
        dataset = cfg["dataset"] if isinstance(cfg, dict) else cfg.dataset
        size = [int(v) for v in (dataset["image_size"] if isinstance(dataset, dict) else dataset.image_size)]
        if size in ([224, 400], [432, 768]):
            return cls()                                     # utils.py:392-397
        if size == [256, 704]:
            return cls(in_hw=(432, 768), out_hw=(256, 704))  # crop_hd, utils.py:348-372
        if size == [192, 384]:
            raise NotImplementedError("image_size [192, 384] takes crop_drivewm (dataset/utils.py:374-388), which resizes "
                                      "with torchvision and is not built into OccCondition: occ_condition_from_config(cfg) "
                                      "returns ResizedOccCondition.drivewm() for it")
        raise ValueError("image_size %r: the image-mode ORS condition is defined for [224, 400], [432, 768] and [256, 704]"
                         % (size,))

    def crop(self, h, w):
        """(top, left, oh, ow) for frames of h x w"""
        if w % self.views:
            raise ValueError("a panorama of %d views has a width that %d divides, got %d" % (self.views, self.views, w))
        if self.in_hw is None:
            return 0, 0, h, w // self.views
        if (h, w // self.views) != self.in_hw:
            raise ValueError("the panoramas are %d x %d x %d, the crop is defined for %d x %d x %d"
                             % (h, self.views, w // self.views, self.in_hw[0], self.views, self.in_hw[1]))
        return self.in_hw[0] - self.out_hw[0], (self.in_hw[1] - self.out_hw[1]) // 2, self.out_hw[0], self.out_hw[1]

    @torch.no_grad()
    def __call__(self, files_or_frames, device="cuda"):
        """A flat list of b .png files (`bytes`), or uint8 frames (b, H, W, 3) already on the device -> (b, 3, h, views *
        w) float32, element for element `torch.stack([crop(ToTensor()(Image.open(f).convert("RGB"))) ...])`."""
        frames = files_or_frames if isinstance(files_or_frames, torch.Tensor) else decode_png(files_or_frames, device=device)
        if frames.dim() != 4:
            raise ValueError("OccCondition takes a flat list of files or (b, H, W, 3) frames, got %s" % (tuple(frames.shape),))
        top, left, oh, ow = self.crop(frames.shape[1], frames.shape[2])
        return O.png_condition(frames, views=self.views, top=top, left=left, size=(oh, ow))


class ResizedOccCondition:
    """The collate step of the image-mode ORS condition where it resizes (`crop_drivewm`, dataset/utils.py:355-358,
    374-388, for image_size [192, 384]): each of the `views` views of in_hw = (H, W / views) gets `pad_top` zero rows on
    top, is resized to resize_hw with `transforms.Resize` as the reference's torchvision 0.11.3 applies it to a float
    tensor — bilinear at half-pixel centres, no antialias, per view — and is cropped to out_hw as `hd_crop` does: the top
    rows and (resize_hw[1] - out_hw[1]) // 2 columns on each side dropped.  Same call as OccCondition: float32 (b, 3, h,
    views * w) on the device.  antialias=True — what torchvision from 0.17 on does to a tensor by default — is not built."""

    def __init__(self, views=6, in_hw=None, pad_top=0, resize_hw=None, out_hw=None, antialias=False):
        if antialias:
            raise ValueError("antialias=True is not built: crop_drivewm resizes with torchvision 0.11.3, whose Resize does not "
                             "antialias a tensor (torchvision >= 0.17 does by default and gives another condition)")
        if isinstance(views, bool) or not isinstance(views, int) or views <= 0:
            raise ValueError("views must be a positive int, got %r" % (views,))
        if isinstance(pad_top, bool) or not isinstance(pad_top, int) or pad_top < 0:
            raise ValueError("pad_top must be an int >= 0, got %r" % (pad_top,))
        if in_hw is None or resize_hw is None or out_hw is None:
            raise ValueError("in_hw, resize_hw and out_hw are (h, w) each (ResizedOccCondition.drivewm() has the reference's)")
        try:
            (ih, iw), (rh, rw), (oh, ow) = ([int(v) for v in hw] for hw in (in_hw, resize_hw, out_hw))
        except (TypeError, ValueError):
            raise ValueError("in_hw, resize_hw and out_hw are (h, w) each, got %r, %r, %r" % (in_hw, resize_hw, out_hw))
        if ih <= 0 or iw <= 0 or rh <= 0 or rw <= 0:
            raise ValueError("in_hw %r and resize_hw %r must be positive" % (tuple(in_hw), tuple(resize_hw)))
        if not (0 < oh <= rh and 0 < ow <= rw) or (rw - ow) % 2:
            raise ValueError("out_hw %r must fit resize_hw %r, the width difference even (hd_crop asserts the result's shape)"
                             % (tuple(out_hw), tuple(resize_hw)))
        self.views, self.pad_top, self.in_hw, self.resize_hw, self.out_hw = views, pad_top, (ih, iw), (rh, rw), (oh, ow)

    @classmethod
    def drivewm(cls):
        """224 x 400 -pad_top-> 225 x 400 -resize-> 216 x 384 -top crop-> 192 x 384 (utils.py:375)"""
        return cls(views=6, in_hw=(224, 400), pad_top=1, resize_hw=(216, 384), out_hw=(192, 384))

    def crop(self, h, w):
        """(top, left, oh, ow) in the resized view, for frames of h x w"""
        if w % self.views:
            raise ValueError("a panorama of %d views has a width that %d divides, got %d" % (self.views, self.views, w))
        if (h, w // self.views) != self.in_hw:
            raise ValueError("the panoramas are %d x %d x %d, the resize is defined for %d x %d x %d"
                             % (h, self.views, w // self.views, self.in_hw[0], self.views, self.in_hw[1]))
        return (self.resize_hw[0] - self.out_hw[0], (self.resize_hw[1] - self.out_hw[1]) // 2, self.out_hw[0], self.out_hw[1])

    @torch.no_grad()
    def __call__(self, files_or_frames, device="cuda"):
        """A flat list of b .png files (`bytes`), or uint8 frames (b, H, W, 3) already on the device -> (b, 3, h, views *
        w) float32: `torch.stack([crop_drivewm(ToTensor()(Image.open(f).convert("RGB"))) ...])` in the arithmetic of
        INTEGRATION.md 4o."""
        frames = files_or_frames if isinstance(files_or_frames, torch.Tensor) else decode_png(files_or_frames, device=device)
        if frames.dim() != 4:
            raise ValueError("ResizedOccCondition takes a flat list of files or (b, H, W, 3) frames, got %s"
                             % (tuple(frames.shape),))
        top, left, oh, ow = self.crop(frames.shape[1], frames.shape[2])
        return O.png_condition_resized(frames, views=self.views, pad_top=self.pad_top, resize=self.resize_hw, top=top,
                                       left=left, size=(oh, ow))


def occ_condition_from_config(cfg):
    """cfg.dataset.image_size (attributes or mappings) -> what collate_fn does to the image-mode ORS condition for it
    (dataset/utils.py:390-408): an OccCondition for [224, 400], [432, 768] and [256, 704], ResizedOccCondition.drivewm()
    for [192, 384]; ValueError for any other size."""
    dataset = cfg["dataset"] if isinstance(cfg, dict) else cfg.dataset
    size = [int(v) for v in (dataset["image_size"] if isinstance(dataset, dict) else dataset.image_size)]
    if size == [192, 384]:
        return ResizedOccCondition.drivewm()
    return OccCondition.from_config(cfg)
