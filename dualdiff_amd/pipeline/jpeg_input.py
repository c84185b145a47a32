"""JPEG input on the GPU: camera .jpg files -> the uint8 frames `ImagePreProcess` / `encode_images` take.

Given-view sampling starts from nuScenes camera files, 900 x 1600 baseline JPEGs that the reference opens with PIL
(`LoadMultiViewImageFromFiles`, configs/dataset/Nuscenes.yaml:98,183; `Image.open` at networks/occ3d_proj.py:124 and
tools/fid_score.py:79).  Here the host walks each file's markers — the header bytes only — and the device does the rest
in one call per batch (`ops.jpeg_decode_u8`): Huffman decoding, libjpeg's `islow` inverse DCT, "fancy" chroma upsampling
and colour conversion, all integer arithmetic, so the frames equal `np.asarray(Image.open(f).convert("RGB"))` byte for
byte.

    frames = load_jpeg(paths)                             # (b, n_cam, H, W, 3) uint8 on the GPU; paths nested (b, n_cam)
    frames = decode_jpeg(files)                           # ... from `bytes`
    x = encode_images(vae, frames, pre)                   # pipeline/image_input.py

What is built is JPEG_INPUT_MODES; any other file is turned down on the host with a ValueError that names the frame and
what was found, before anything is uploaded, and is the caller's to decode (with PIL).  This module does not import PIL.
"""
import functools
import os

import numpy as np
import torch

from .. import ops as O

JPEG_INPUT_MODES = ("baseline (SOF0), 8-bit, three components stored as YCbCr in one interleaved scan, 4:2:0 or 4:4:4 sampling, "
                    "8-bit quantisation tables, any Huffman tables, no restart interval, no bytes between the last block and the EOI marker")
SAMPLINGS = {((2, 2), (1, 1), (1, 1)): 420, ((1, 1), (1, 1), (1, 1)): 444}

# natural (row-major) index of the i-th coefficient of the zigzag scan
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
          28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
          47, 55, 62, 63)
_SOF_NAMES = {0xC1: "extended sequential (SOF1)", 0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)",
              0xC5: "differential sequential (SOF5)", 0xC6: "differential progressive (SOF6)",
              0xC7: "differential lossless (SOF7)", 0xC9: "arithmetic sequential (SOF9)",
              0xCA: "arithmetic progressive (SOF10)", 0xCB: "arithmetic lossless (SOF11)",
              0xCD: "arithmetic differential sequential (SOF13)", 0xCE: "arithmetic differential progressive (SOF14)",
              0xCF: "arithmetic differential lossless (SOF15)"}


class JpegInfo:
    """What parse_jpeg found: h, w; sampling (420 / 444); qtables {slot: 64 values in natural order}; huffman {(class,
    slot): (bits, values)}, class 0 DC / 1 AC; components [(id, quantisation slot, DC slot, AC slot)] in scan order;
    scan (start, end): the entropy-coded segment is data[start:end], from the byte behind SOS up to the EOI marker."""
    __slots__ = ("h", "w", "sampling", "qtables", "huffman", "components", "scan")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw[k])


def _refuse(frame, found):
    where = "" if frame is None else "frame %d: " % frame
    raise ValueError("%s%s is not built; available: %s" % (where, found, JPEG_INPUT_MODES))


def _broken(frame, what):
    raise ValueError("%s%s" % ("" if frame is None else "frame %d: " % frame, what))


def parse_jpeg(data, frame=None):
    """A marker walk over the header bytes of one file -> JpegInfo.  The scan bytes are not looked at: the end of the
    segment is the EOI marker found from the end of the file.  Raises ValueError (with `frame`, when given, in front) for a
    file that is not a JPEG, that is cut short, or that is of a kind that is not built."""
    data = data if isinstance(data, (bytes, bytearray)) else bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        _broken(frame, "not a JPEG file (no SOI marker)")
    qtables, huffman, frame_comps, size, dri, adobe, jfif = {}, {}, None, None, 0, None, False
    pos = 2
    while True:
        if pos + 4 > n:
            _broken(frame, "no SOS marker before the end of the file (missing SOS)")
        if data[pos] != 0xFF:
            _broken(frame, "byte %d is not a marker" % pos)
        marker = data[pos + 1]
        if marker == 0xFF:                                   # fill byte
            pos += 1
            continue
        if marker == 0xD9:
            _broken(frame, "EOI before any scan (missing SOS)")
        if marker == 0x01 or 0xD0 <= marker <= 0xD7:         # stand-alone markers
            pos += 2
            continue
        length = (data[pos + 2] << 8) | data[pos + 3]
        body = bytes(data[pos + 4:pos + 2 + length])
        if length < 2 or len(body) != length - 2:
            _broken(frame, "segment %02X at byte %d is cut short" % (marker, pos))
        if marker in _SOF_NAMES:
            _refuse(frame, _SOF_NAMES[marker] + " JPEG")
        if marker == 0xDB:
            at = 0
            while at < len(body):
                precision, slot = body[at] >> 4, body[at] & 15
                if precision:
                    _refuse(frame, "a 16-bit quantisation table")
                vals = body[at + 1:at + 65]
                if len(vals) != 64 or slot > 3:
                    _broken(frame, "bad DQT segment")
                nat = [0] * 64
                for i, v in enumerate(vals):
                    nat[ZIGZAG[i]] = v
                qtables[slot] = tuple(nat)
                at += 65
        elif marker == 0xC4:
            at = 0
            while at < len(body):
                cls, slot = body[at] >> 4, body[at] & 15
                bits = bytes(body[at + 1:at + 17])
                count = sum(bits)
                vals = bytes(body[at + 17:at + 17 + count])
                if len(bits) != 16 or len(vals) != count or count > 256 or cls > 1:
                    _broken(frame, "bad DHT segment")
                if slot > 1:
                    _refuse(frame, "Huffman table slot %d (baseline has 0 and 1)" % slot)
                huffman[cls, slot] = (bits, vals)
                at += 17 + count
        elif marker == 0xC0:
            if len(body) < 6 or len(body) != 6 + 3 * body[5]:
                _broken(frame, "bad SOF0 segment")
            if body[0] != 8:
                _refuse(frame, "%d-bit samples" % body[0])
            size = ((body[1] << 8) | body[2], (body[3] << 8) | body[4])
            frame_comps = [(body[6 + 3 * i], (body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15), body[8 + 3 * i])
                           for i in range(body[5])]
        elif marker == 0xDD:
            dri = (body[0] << 8) | body[1] if len(body) >= 2 else 0
        elif marker == 0xE0 and body[:5] == b"JFIF\x00":
            jfif = True
        elif marker == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]                                 # the colour transform: 0 none (RGB / CMYK), 1 YCbCr, 2 YCCK
        elif marker == 0xDA:
            break
        pos += 2 + length
    if frame_comps is None:
        _broken(frame, "SOS before SOF0")
    if len(frame_comps) == 1:
        _refuse(frame, "a grayscale JPEG (one component)")
    if len(frame_comps) == 4:
        _refuse(frame, "a CMYK / YCCK JPEG (four components)")
    if len(frame_comps) != 3:
        _refuse(frame, "a JPEG of %d components" % len(frame_comps))
    # libjpeg (default_decompress_parms) takes three components as YCbCr if the file has a JFIF segment; without one, an
    # Adobe segment with transform 0 or, with no Adobe segment either, components named R, G, B mean the file is stored RGB
    if not jfif and (adobe == 0 or (adobe is None and bytes(c[0] for c in frame_comps) == b"RGB")):
        _refuse(frame, "an RGB JPEG (no JFIF segment; Adobe transform 0, or components named R, G, B)")
    if dri:
        _refuse(frame, "a restart interval (DRI %d)" % dri)
    factors = tuple(c[1] for c in frame_comps)
    if factors not in SAMPLINGS:
        _refuse(frame, "sampling %s" % ", ".join("%dx%d" % f for f in factors))
    if size[0] == 0 or size[1] == 0:
        _broken(frame, "a frame of %d x %d" % size)
    ns = body[0] if body else 0
    if len(body) != 1 + 2 * ns + 3:
        _broken(frame, "bad SOS segment")
    if ns != 3:
        _refuse(frame, "several scans (the first has %d of 3 components)" % ns)
    components = []
    for i in range(3):
        cid, sel = body[1 + 2 * i], body[2 + 2 * i]
        if cid != frame_comps[i][0]:
            _refuse(frame, "a scan whose components are not in the frame's order")
        tq, td, ta = frame_comps[i][2], sel >> 4, sel & 15
        if tq not in qtables or (0, td) not in huffman or (1, ta) not in huffman:
            _broken(frame, "component %d names a table the file does not define" % cid)
        components.append((cid, tq, td, ta))
    if tuple(body[1 + 2 * ns:]) != (0, 63, 0):
        _refuse(frame, "a scan with spectral selection or successive approximation")
    start = pos + 2 + length
    end = data.rfind(b"\xff\xd9")
    if end < start:
        _broken(frame, "no EOI marker behind the scan (missing EOI)")
    return JpegInfo(h=size[0], w=size[1], sampling=SAMPLINGS[factors], qtables=qtables, huffman=huffman,
                    components=components, scan=(start, end))


@functools.lru_cache(maxsize=64)
def huffman_block(bits, values):
    """One Huffman table (bits[16], values) -> the 904 bytes dd_jpeg_decode_u8 reads (include/dualdiff_hip.h): codes
    assigned as T.81 Annex C does; a look-up of the next 8 bits for the short codes, and per length the limit and the
    offset into the values for the long ones."""
    lut = np.zeros(256, dtype="<u2")
    lim, off = np.zeros(17, dtype="<i4"), np.zeros(17, dtype="<i4")
    vals = np.zeros(256, dtype=np.uint8)
    vals[:len(values)] = np.frombuffer(values, dtype=np.uint8)
    code = k = 0
    for length in range(1, 17):
        off[length] = k - code
        for _ in range(bits[length - 1]):
            if code >= 1 << length:
                raise ValueError("a Huffman table with more codes of length %d than there are" % length)
            if length <= 8:
                lut[code << (8 - length):(code + 1) << (8 - length)] = (length << 8) | values[k]
            code += 1
            k += 1
        lim[length] = code << (16 - length)
        code <<= 1
    return lut.tobytes() + lim.tobytes() + off.tobytes() + vals.tobytes()


def table_block(info):
    """JpegInfo -> the frame's table block, ops.JPEG_DECODE_TABLE_BYTES bytes."""
    q = np.array([info.qtables[c[1]] for c in info.components], dtype="<u2")
    sel = bytes([c[2] for c in info.components] + [c[3] for c in info.components] + [0, 0])
    empty = (bytes(16), b"")
    tabs = b"".join(huffman_block(*info.huffman.get(key, empty)) for key in ((0, 0), (0, 1), (1, 0), (1, 1)))
    out = q.tobytes() + sel + tabs + bytes(8)
    assert len(out) == O.JPEG_DECODE_TABLE_BYTES
    return out


def _flatten(files):
    if isinstance(files, (bytes, bytearray, memoryview)) or not len(files):
        raise ValueError("decode_jpeg takes a list of files (bytes), flat or nested (b, n)")
    if isinstance(files[0], (bytes, bytearray, memoryview)):
        return list(files), None
    per = len(files[0])
    if per == 0 or any(len(row) != per for row in files):
        raise ValueError("decode_jpeg takes a (b, n) list with the same n in every row")
    return [f for row in files for f in row], (len(files), per)


def upload_jpeg(files, device="cuda", lead=0):
    """A flat list of files -> what ops.jpeg_decode_u8 takes, after ONE host-to-device copy (from pinned memory, not
    waited for): (scan, offsets, lengths, tables, h, w, sampling, max_scan_bytes), the four tensors views of the one
    upload.  The segments lie one behind the other as the files' own lengths make them, after `lead` spare bytes (a test
    hook for the byte alignment).  Every file is parsed, and refused if need be, before anything is allocated."""
    infos = []
    for i, f in enumerate(files):
        if not isinstance(f, (bytes, bytearray, memoryview)):
            raise ValueError("frame %d: a file is `bytes`, got %s" % (i, type(f).__name__))
        infos.append(parse_jpeg(f, frame=i))
    first = infos[0]
    for i, info in enumerate(infos):
        if (info.h, info.w, info.sampling) != (first.h, first.w, first.sampling):
            raise ValueError("frame %d: %d x %d sampling %d differs from frame 0 (%d x %d sampling %d); the frames of one "
                             "call have one geometry" % (i, info.h, info.w, info.sampling, first.h, first.w, first.sampling))
    blocks = [table_block(info) for info in infos]
    m = len(files)
    lens = [info.scan[1] - info.scan[0] for info in infos]
    head = (8 * m + 15) // 16 * 16                           # offsets | lengths
    scan_at = head + m * O.JPEG_DECODE_TABLE_BYTES
    total = scan_at + int(lead) + sum(lens)
    device = torch.device(device)
    host = torch.empty(total + 1, dtype=torch.uint8, pin_memory=device.type == "cuda")
    raw = host.numpy()
    meta = raw[:8 * m].view("<i4")
    at = int(lead)
    for i, (f, info) in enumerate(zip(files, infos)):
        meta[i], meta[m + i] = at, lens[i]
        raw[head + i * len(blocks[i]):head + (i + 1) * len(blocks[i])] = np.frombuffer(blocks[i], dtype=np.uint8)
        raw[scan_at + at:scan_at + at + lens[i]] = np.frombuffer(f, dtype=np.uint8, count=lens[i], offset=info.scan[0])
        at += lens[i]
    dev = host.to(device, non_blocking=True)
    offsets, lengths = dev[:4 * m].view(torch.int32), dev[4 * m:8 * m].view(torch.int32)
    tables = dev[head:scan_at].view(m, O.JPEG_DECODE_TABLE_BYTES)
    return dev[scan_at:], offsets, lengths, tables, first.h, first.w, first.sampling, max(max(lens), 1)


def _status_text(bits):
    return ", ".join(text for bit, text in O.JPEG_DECODE_STATUS if bits & bit) or "status %d" % bits


@torch.no_grad()
def decode_jpeg(files, device="cuda", check=True, rounds=None):
    """A flat list of JPEG files (`bytes`) -> uint8 frames (m, H, W, 3) on `device`, a (b, n) nested list -> (b, n, H,
    W, 3): `np.asarray(Image.open(f).convert("RGB"))` of every file, byte for byte, decoded on the GPU.  One pinned
    upload (the files' scan bytes as they are, and one table block per frame) and one call into the library per batch.
    check=True reads the per-frame status back and raises ValueError for the first frame whose stream was broken;
    check=False does not synchronise and returns (frames, status), status int32 (m,) / (b, n) on the device, 0 for a
    good frame.  Files of a kind that is not built (JPEG_INPUT_MODES) raise ValueError before anything is uploaded."""
    flat, nest = _flatten(files)
    scan, offsets, lengths, tables, h, w, sampling, longest = upload_jpeg(flat, device)
    frames, status = O.jpeg_decode_u8(scan, offsets, lengths, tables, h, w, sampling, longest, rounds=rounds)
    if check:
        for i, s in enumerate(status.cpu().tolist()):
            if s:
                raise ValueError("frame %d: the scan does not decode: %s" % (i, _status_text(s)))
    if nest is not None:
        frames, status = frames.view(*nest, h, w, 3), status.view(*nest)
    return frames if check else (frames, status)


def load_jpeg(paths, device="cuda", check=True, rounds=None):
    """decode_jpeg of the files at `paths` (flat, or nested (b, n))."""
    def read(p):
        with open(os.fspath(p), "rb") as f:
            return f.read()
    if not len(paths):
        raise ValueError("load_jpeg takes a list of paths, flat or nested (b, n)")
    nested = not isinstance(paths[0], (str, bytes, os.PathLike))
    files = [[read(p) for p in row] for row in paths] if nested else [read(p) for p in paths]
    return decode_jpeg(files, device=device, check=check, rounds=rounds)
