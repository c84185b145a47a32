"""libjpeg's baseline encoder as PIL drives it from `Image.save(name.jpg)`, restated in numpy: quality 1-100, 4:2:0 chroma,
the standard Huffman tables, the `islow` integer DCT.  `encode(rgb, quality)` returns the file's bytes.

Every step is integer arithmetic, so the restatement equals PIL byte for byte (tests/test_jpeg_output_cpu.py holds it to
the fixture minted from PIL and, where PIL imports, to a fresh save).  It shares no code with the package: the tables
below are written out a second time on purpose.
"""
import numpy as np

# ITU-T T.81 Annex K.1, natural (row-major) order
BASE_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
             14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
             49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
BASE_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
               47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
# Annex K.3: (bits[1..16], values) of the DC / AC tables of luma and chroma
DC_LUMA = ("00010501010101010100000000000000", "000102030405060708090a0b")
DC_CHROMA = ("00030101010101010101010000000000", "000102030405060708090a0b")
AC_LUMA = ("0002010303020403050504040000017d",
           "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738"
           "393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5"
           "a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
AC_CHROMA = ("00020102040403040705040400010277",
             "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a3536"
             "3738393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999a"
             "a2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")


def _zigzag():
    order = sorted(range(64), key=lambda k: (k // 8 + k % 8, (k // 8) if (k // 8 + k % 8) % 2 else (k % 8)))
    return np.array(order)


ZIGZAG = _zigzag()                      # ZIGZAG[i] = natural index of the i-th coefficient of the scan


def quant_tables(quality):
    """jpeg_set_quality: -> (luma, chroma) int arrays in natural order."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality must be 1..100")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.array(b) * scale + 50) // 100, 1, 255) for b in (BASE_LUMA, BASE_CHROMA))


def huff_codes(spec):
    """(bits, values) -> {symbol: (code, length)}: codes of a length in increasing order, Annex C."""
    bits, vals = bytes.fromhex(spec[0]), bytes.fromhex(spec[1])
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def header(h, w, quality):
    """The file up to and including SOS, in the layout PIL's save writes."""
    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body
    ql, qc = quant_tables(quality)
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    out += seg(0xDB, b"\x00" + bytes(int(v) for v in ql[ZIGZAG])) + seg(0xDB, b"\x01" + bytes(int(v) for v in qc[ZIGZAG]))
    out += seg(0xC0, b"\x08" + h.to_bytes(2, "big") + w.to_bytes(2, "big") + b"\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01")
    for tc_th, spec in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += seg(0xC4, bytes([tc_th]) + bytes.fromhex(spec[0]) + bytes.fromhex(spec[1]))
    return out + seg(0xDA, b"\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00")


def ycc(rgb):
    """jccolor.c's 16-bit fixed point: -> int64 planes Y, Cb, Cr of the image's own size."""
    r, g, b = (rgb[..., c].astype(np.int64) for c in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(p, rows, cols):
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def planes(rgb):
    """The three component planes as the DCT sees them, each padded to whole blocks by its own rule."""
    h, w = rgb.shape[:2]
    y, cb, cr = ycc(rgb)
    y = _pad(y, 8 * -(-h // 8), 8 * -(-w // 8))
    ch, cw = -(-h // 2), -(-w // 2)
    out = [y]
    for c in (cb, cr):
        c = _pad(c, 2 * ch, 16 * -(-cw // 8))                # even rows; whole chroma blocks of columns, at full size
        bias = np.tile(np.array([1, 2]), c.shape[1] // 4)     # h2v2_downsample: 1, 2, 1, 2, ...
        d = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        out.append(_pad(d, 8 * -(-ch // 8), d.shape[1]))     # then the last CHROMA row down to whole blocks
    return out


def _fdct_1d(d, first):
    """One pass of jfdctint.c over the last axis of d (..., 8)."""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15

    def ds(x, s):
        return (x + (1 << (s - 1))) >> s
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = ds(t10 + t11, 2), ds(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2], o[6] = ds(z1 + t13 * 6270, n), ds(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = ds(t4 + z1 + z3, n), ds(t5 + z2 + z4, n), ds(t6 + z2 + z3, n), ds(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def blocks(plane, q):
    """A padded plane -> quantised coefficients (block rows, block cols, 64) in zigzag order."""
    br, bc = plane.shape[0] // 8, plane.shape[1] // 8
    b = plane.reshape(br, 8, bc, 8).transpose(0, 2, 1, 3) - 128
    b = _fdct_1d(b, True)                                              # rows
    b = _fdct_1d(b.swapaxes(-1, -2), False).swapaxes(-1, -2)           # columns
    d = (q.reshape(8, 8).astype(np.int64)) << 3
    c = np.sign(b) * ((np.abs(b) + (d >> 1)) // d)
    return c.reshape(br, bc, 64)[..., ZIGZAG]


def scan_blocks(rgb, quality):
    """-> list of (component, coefficients[64] in zigzag order) in scan order: Y00 Y01 Y10 Y11 Cb Cr per MCU, MCUs
    row-major, libjpeg's dummy blocks included."""
    h, w = rgb.shape[:2]
    ql, qc = quant_tables(quality)
    py, pcb, pcr = planes(rgb)
    cy, ccb, ccr = blocks(py, ql), blocks(pcb, qc), blocks(pcr, qc)
    out = []
    for my in range(-(-h // 16)):
        for mx in range(-(-w // 16)):
            mcu = []
            for k in range(4):
                by, bx = 2 * my + k // 2, 2 * mx + k % 2
                if by < cy.shape[0] and bx < cy.shape[1]:
                    v = cy[by, bx]
                else:                                  # dummy: no AC, the DC of the block before it (of block 1 in a dummy row)
                    v = np.zeros(64, dtype=np.int64)
                    v[0] = mcu[k - 1 if by < cy.shape[0] else 1][0]
                mcu.append(v)
            out += [(0, v) for v in mcu] + [(1, ccb[my, mx]), (2, ccr[my, mx])]
    return out


class BitWriter:
    """MSB-first bit stream; whole bytes leave the accumulator as they fill."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        if self.n >= 8:
            k = self.n // 8
            self.n -= 8 * k
            self.out += (self.acc >> self.n).to_bytes(k, "big")
            self.acc &= (1 << self.n) - 1

    def bytes(self):
        if self.n:                                                     # the last byte is filled with 1-bits
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)
        return bytes(self.out).replace(b"\xff", b"\xff\x00")


def entropy(scan, stats=None):
    """jchuff.c's encode_one_block over the scan -> the stuffed entropy-coded segment.  stats, when given, collects
    `dc_sizes` (set) and `zrl` (set of ZRL counts in front of a coefficient)."""
    dc = (huff_codes(DC_LUMA), huff_codes(DC_CHROMA), huff_codes(DC_CHROMA))
    ac = (huff_codes(AC_LUMA), huff_codes(AC_CHROMA), huff_codes(AC_CHROMA))
    w, pred = BitWriter(), [0, 0, 0]
    for comp, v in scan:
        diff = int(v[0]) - pred[comp]
        pred[comp] = int(v[0])
        size = abs(diff).bit_length()
        w.put(*dc[comp][size])
        w.put(diff if diff >= 0 else diff - 1, size)
        if stats is not None:
            stats.setdefault("dc_sizes", set()).add(size)
        last = 0
        for k in np.flatnonzero(v[1:]) + 1:
            c, run = int(v[k]), int(k) - last - 1
            last = int(k)
            if stats is not None and run >= 16:
                stats.setdefault("zrl", set()).add(run >> 4)
            for _ in range(run >> 4):
                w.put(*ac[comp][0xF0])
            size = abs(c).bit_length()
            w.put(*ac[comp][((run & 15) << 4) | size])
            w.put(c if c >= 0 else c - 1, size)
        if last != 63:
            w.put(*ac[comp][0x00])
    return w.bytes()


def encode(rgb, quality=75, stats=None):
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.size == 0:
        raise ValueError("encode takes a uint8 (H, W, 3) frame")
    h, w = rgb.shape[:2]
    return header(h, w, quality) + entropy(scan_blocks(rgb, quality), stats) + b"\xff\xd9"
