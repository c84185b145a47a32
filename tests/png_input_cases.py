"""The named inputs of the PNG input tests (tests/test_png_input_cpu.py, tests/test_png_input_gpu.py): a minimal PNG
writer and a deflate bit-writer, the smallest files at which each part of the decoder can go wrong, and one broken stream
per status bit.

Everything is built at test time from fixed seeds.  The expected pixels are known by construction — they are the rows
before filtering — not from a decoder.  The file bytes may differ between zlib builds; the pixels do not.

    cases()     [Case(name, data, pixels (H, W, 3) uint8, colour_type, idats)]: files every decoder accepts
    broken()    [Broken(name, data, status)]: each derived from the 7 x 5 RGBA file, each sets exactly one status bit
"""
import collections
import functools
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
Case = collections.namedtuple("Case", "name data pixels colour_type idats")
Broken = collections.namedtuple("Broken", "name data status")
CHANNELS = {0: 1, 2: 3, 6: 4}
# include/dualdiff_hip.h: DD_PNG_*
TRUNCATED, BAD_BLOCK, BAD_STORED, BAD_LENGTHS, BAD_SYMBOL, BAD_DISTANCE = 1, 2, 4, 8, 16, 32
TOO_LONG, TOO_SHORT, BAD_ADLER, BAD_ZLIB, BAD_FILTER = 64, 128, 256, 512, 1024
RGBA_FILTERS = (4, 2, 3, 1, 0, 4, 3)           # Paeth and Up on the first row, Average on the second


# ---- a minimal PNG writer -----------------------------------------------------------------------------------------------

def chunk(kind, body=b""):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def ihdr(h, w, colour_type, depth=8, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour_type, 0, 0, interlace))


def png_file(h, w, colour_type, stream, cuts=None, before=b"", **head):
    """The file of an (h, w) image whose zlib stream is `stream`, cut into IDATs of the lengths `cuts` (the rest in a last
    one; None: one IDAT), with the chunks `before` between IHDR and the first IDAT."""
    parts, at = [], 0
    for n in (cuts or []):
        parts.append(chunk(b"IDAT", stream[at:at + n]))
        at += n
    parts.append(chunk(b"IDAT", stream[at:]))
    return SIGNATURE + ihdr(h, w, colour_type, **head) + before + b"".join(parts) + chunk(b"IEND")


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def filter_rows(pix, types):
    """(H, W, C) uint8 and one filter type per row -> the filtered bytes, the type byte in front of every row (PNG
    specification, 9: Filtering)."""
    h, w, c = pix.shape
    raw = pix.reshape(h, w * c).astype(np.int64)
    a = np.zeros_like(raw)
    a[:, c:] = raw[:, :-c]
    b = np.zeros_like(raw)
    b[1:] = raw[:-1]
    d = np.zeros_like(raw)
    d[1:, c:] = raw[:-1, :-c]
    out = bytearray()
    for y, t in enumerate(types):
        if t == 4:
            pred = np.array([_paeth(int(a[y, k]), int(b[y, k]), int(d[y, k])) for k in range(w * c)], dtype=np.int64)
        else:
            pred = (0 * raw[y], a[y], b[y], (a[y] + b[y]) >> 1)[t if t < 4 else 0]
        out += bytes([t]) + ((raw[y] - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def rgb(pix):
    """what `Image.open(f).convert("RGB")` makes of the constructed pixels: alpha dropped, grey replicated"""
    return np.ascontiguousarray(np.repeat(pix, 3, axis=2) if pix.shape[2] == 1 else pix[:, :, :3])


def noise(h, w, c, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, c)).astype(np.uint8)


def deflate(data, level=-1, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0):
    """zlib's stream of `data`; flush_every: cut by Z_SYNC_FLUSH and Z_FULL_FLUSH in turn every so many bytes"""
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    if not flush_every:
        return co.compress(data) + co.flush()
    out = b""
    for i, at in enumerate(range(0, len(data), flush_every)):
        out += co.compress(data[at:at + flush_every]) + co.flush(zlib.Z_FULL_FLUSH if i % 2 else zlib.Z_SYNC_FLUSH)
    return out + co.flush()


# ---- a deflate bit-writer -----------------------------------------------------------------------------------------------

class Bits:
    """RFC 1951 3.1.1: values LSB first, Huffman codes MSB first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, n):
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, code, n):
        return self.bits(int(format(code, "0%db" % n)[::-1], 2), n)

    def fixed(self, sym):
        """a literal / length symbol in the fixed code (RFC 1951 3.2.6)"""
        if sym < 144:
            return self.code(0x30 + sym, 8)
        if sym < 256:
            return self.code(0x190 + sym - 144, 9)
        if sym < 280:
            return self.code(sym - 256, 7)
        return self.code(0xC0 + sym - 280, 8)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)
        return self

    def stored(self, data, final=0):
        self.bits(final, 1).bits(0, 2).align()
        self.out += struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data
        return self

    def done(self):
        return bytes(self.align().out)


def zstream(blocks, data):
    """the zlib stream of the deflate bytes `blocks`, with the Adler-32 of `data`"""
    return b"\x78\x9c" + blocks + struct.pack(">I", zlib.adler32(data))


# ---- the good cases -----------------------------------------------------------------------------------------------------

def _case(name, pix, types, colour_type, stream=None, cuts=None, before=b"", **kw):
    h, w, _ = pix.shape
    filt = filter_rows(pix, types)
    stream = deflate(filt, **kw) if stream is None else stream
    assert zlib.decompress(stream) == filt, name
    return Case(name, png_file(h, w, colour_type, stream, cuts, before), rgb(pix), colour_type, 1 + len(cuts or []))


@functools.lru_cache(maxsize=None)
def rgba_7x5():
    """(pixels (7, 5, 4), filtered bytes, zlib's default stream of them)"""
    pix = noise(7, 5, 4, 75)
    filt = filter_rows(pix, RGBA_FILTERS)
    return pix, filt, deflate(filt)


def window_edge():
    """(pixels (130, 85, 3), stream): a stored block of 32768 noise bytes, then a fixed-Huffman block with one match of
    length 258 (symbol 285) at distance 32768 (code 29, 13 extra bits all ones), 254 literals that fill the last row, and
    the end of the block.  Filter type 0 in front of every row of 256 bytes, also where the match copies one."""
    first = bytearray(np.random.RandomState(32768).randint(0, 256, 32768).astype(np.uint8).tobytes())
    first[::256] = bytes(128)
    tail = np.random.RandomState(258).randint(0, 256, 254).astype(np.uint8).tobytes()
    b = Bits().stored(bytes(first[:65535]))
    b.bits(1, 1).bits(1, 2).fixed(285).code(29, 5).bits(8191, 13)
    for v in tail:
        b.fixed(v)
    b.fixed(256)
    filt = bytes(first) + bytes(first[:258]) + tail
    stream = zstream(b.done(), filt)
    assert zlib.decompress(stream) == filt and len(filt) == 130 * 256
    pix = np.frombuffer(filt, dtype=np.uint8).reshape(130, 256)[:, 1:].reshape(130, 85, 3)
    return pix, stream


@functools.lru_cache(maxsize=None)
def cases():
    pix, filt, default = rgba_7x5()
    out = [
        # geometry (H x W)
        _case("1x1_rgb", noise(1, 1, 3, 1), (0,), 2),
        _case("2x3_rgb", noise(2, 3, 3, 2), (1, 4), 2),
        _case("7x5_rgba", pix, RGBA_FILTERS, 6),
        _case("3x9_grey", noise(3, 9, 1, 3), (3, 4, 2), 0),
        _case("5x2_rgb_odd_row", noise(5, 2, 3, 4), (2, 1, 4, 3, 0), 2),                 # rows of 7 bytes
        _case("66x3_rgba_two_bands", noise(66, 3, 4, 5), tuple((3, 4, 2, 1, 0)[y % 5] for y in range(66)), 6),
        # more rows than the unfilter kernel has threads (1024): row 1024 is Paeth-filtered against the sweep before
        _case("1030x2_rgba_two_sweeps", noise(1030, 2, 4, 6), tuple((0, 1, 2, 3, 4)[y % 5] for y in range(1030)), 6),
        # block kinds, on the 7 x 5 RGBA noise
        _case("7x5_stored", pix, RGBA_FILTERS, 6, level=0),
        _case("7x5_fixed", pix, RGBA_FILTERS, 6, strategy=zlib.Z_FIXED),
        _case("7x5_huffman_only", pix, RGBA_FILTERS, 6, strategy=zlib.Z_HUFFMAN_ONLY),
        _case("7x5_rle", pix, RGBA_FILTERS, 6, strategy=zlib.Z_RLE),
        _case("7x5_flushes", pix, RGBA_FILTERS, 6, flush_every=20),
        # a dynamic block zlib does choose: four values, skewed
        _case("7x5_dynamic", np.random.RandomState(7).choice(np.array([0, 1, 2, 255], dtype=np.uint8), (7, 5, 4),
                                                             p=(0.7, 0.15, 0.1, 0.05)), (0,) * 7, 6, level=9),
        # IDAT cuts of one stream
        _case("7x5_one_idat", pix, RGBA_FILTERS, 6, stream=default),
        _case("7x5_byte_idats", pix, RGBA_FILTERS, 6, stream=default, cuts=[1] * (len(default) - 1)),
        _case("7x5_empty_idats", pix, RGBA_FILTERS, 6, stream=default, cuts=[0, 3, 0, 7]),
        # ancillary chunks
        _case("2x3_ancillary", noise(2, 3, 3, 2), (1, 4), 2,
              before=chunk(b"gAMA", struct.pack(">I", 45455)) + chunk(b"tRNS", bytes(6)) + chunk(b"tEXt", b"Comment\x00seven")),
    ]
    # long streams: 300 rows of 256 bytes
    long_pix = noise(300, 85, 3, 85)
    types = tuple((0, 1, 2, 3, 4)[y % 5] for y in range(300))
    out.append(_case("300x85_two_stored", long_pix, types, 2, level=0))                 # 76800 > 65535
    for period in (127, 126):       # 32512 bytes is past zlib's own longest distance (32506), 32256 is not
        rep = long_pix[np.arange(300) % period]
        c = _case("300x85_period_%d" % period, rep, (0,) * 300, 2, level=9)
        out.append(c)
    wp, ws = window_edge()
    out.append(_case("130x85_window_edge", wp, (0,) * 130, 2, stream=ws))
    return tuple(out)


def own_files():
    """[(name, file, pixels)]: tests/png_cases.cases() through the reference encoder of our own format"""
    from tests import png_cases
    return [(c.name, png_cases.reference(c.name)[0], c.img) for c in png_cases.cases()]


def foreign_chunk_shaped():
    """(file, pixels): a PIL-style single stream of a 128 x 85 RGB image, cut into the two IDATs that our own format
    would have — the host precondition holds, the device's verification must not"""
    from tests import png_cases
    img = next(c.img for c in png_cases.cases() if c.name == "128x85_two_chunks")
    stream = deflate(filter_rows(img, tuple((1, 2, 4, 0, 3)[y % 5] for y in range(128))), level=6)
    return png_file(128, 85, 2, stream, cuts=[len(stream) // 3]), np.ascontiguousarray(img)


# ---- the broken streams -------------------------------------------------------------------------------------------------

def _one_bit_lengths(b, lens):
    """a dynamic header whose code-length code has the symbols 0 and 1, one bit each, and the code lengths `lens`"""
    b.bits(1, 1).bits(2, 2).bits(0, 5).bits(0, 5).bits(14, 4)             # 257 literal / length codes, 1 distance code, 18 lengths
    for sym in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1):
        b.bits(1 if sym in (0, 1) else 0, 3)
    for v in lens:
        b.bits(v, 1)
    return b


@functools.lru_cache(maxsize=None)
def broken():
    pix, filt, stream = rgba_7x5()
    assert stream[2] == 1 and len(stream) == 2 + 5 + len(filt) + 4        # zlib stores noise: one final stored block
    pad = bytes(12)

    def file(s, h=7):
        return png_file(h, 5, 6, s)

    def flip(s, at, bit=1):
        s = bytearray(s)
        s[at] ^= bit
        return bytes(s)
    taller, shorter = noise(8, 5, 4, 8), pix[:6]
    bad_filter = bytearray(filt)
    bad_filter[0] = 5
    over = [0] * 258
    over[0] = over[1] = over[256] = 1                                      # three codes of one bit
    out = [
        Broken("cut_6_short", file(stream[:-6]), TRUNCATED),
        Broken("adler_flipped", file(flip(stream, -1)), BAD_ADLER),
        Broken("block_type_3", file(b"\x78\x9c" + Bits().bits(1, 1).bits(3, 2).done() + pad), BAD_BLOCK),
        Broken("nlen_flipped", file(flip(stream, 5)), BAD_STORED),
        Broken("oversubscribed", file(b"\x78\x9c" + _one_bit_lengths(Bits(), over).done() + pad), BAD_LENGTHS),
        Broken("symbol_286", file(b"\x78\x9c" + Bits().bits(1, 1).bits(1, 2).fixed(286).done() + pad), BAD_SYMBOL),
        Broken("distance_code_30", file(b"\x78\x9c" + Bits().bits(1, 1).bits(1, 2).fixed(97).fixed(257).code(30, 5).done() + pad),
               BAD_SYMBOL),
        # the code-length code has the symbols 0 and 16, one bit each; the first length is a repeat
        Broken("repeat_first", file(b"\x78\x9c" + Bits().bits(1, 1).bits(2, 2).bits(0, 5).bits(0, 5).bits(0, 4).bits(1, 3).bits(0, 3)
                                    .bits(0, 3).bits(1, 3).bits(1, 1).bits(0, 2).done() + pad), BAD_SYMBOL),
        Broken("distance_2_first", file(b"\x78\x9c" + Bits().bits(1, 1).bits(1, 2).fixed(257).code(1, 5).done() + pad), BAD_DISTANCE),
        Broken("8_rows_in_7", file(deflate(filter_rows(taller, RGBA_FILTERS + (1,)))), TOO_LONG),
        Broken("6_rows_in_7", file(deflate(filter_rows(shorter, RGBA_FILTERS[:6]))), TOO_SHORT),
        Broken("zlib_78_02", file(flip(stream, 1, stream[1] ^ 0x02)), BAD_ZLIB),
        Broken("filter_5", file(deflate(bytes(bad_filter))), BAD_FILTER),
    ]
    assert len({b.name for b in out}) == 13
    return tuple(out)
