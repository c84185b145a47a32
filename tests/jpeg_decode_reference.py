"""libjpeg's baseline decoder as PIL drives it from `Image.open(f).convert("RGB")`, restated in numpy: Huffman decoding with
the file's own tables, dequantisation, the `islow` integer inverse DCT, "fancy" h2v2 chroma upsampling, 16-bit fixed-point
colour conversion.  `decode(data)` returns the uint8 (H, W, 3) frame.

Every step is integer arithmetic, so the restatement equals PIL byte for byte (tests/test_jpeg_input_cpu.py holds it to the
fixture minted from PIL and, where PIL imports, to a fresh decode).  It shares no code with the package: the marker walk,
the zigzag order and the constants are written out here a second time on purpose.  Three components, 4:2:0 or 4:4:4, one
scan, no restart interval; anything else raises ValueError.
"""
import numpy as np


def _zigzag():
    order = sorted(range(64), key=lambda k: (k // 8 + k % 8, (k // 8) if (k // 8 + k % 8) % 2 else (k % 8)))
    return np.array(order)


ZIGZAG = _zigzag()                      # ZIGZAG[i] = natural index of the i-th coefficient of the scan


def segments(data):
    """-> ([(marker, body)] up to and including SOS, offset of the first scan byte)"""
    assert data[:2] == b"\xff\xd8", "no SOI"
    out, pos = [], 2
    while True:
        assert data[pos] == 0xFF, pos
        marker = data[pos + 1]
        if marker == 0xFF:
            pos += 1
            continue
        n = int.from_bytes(data[pos + 2:pos + 4], "big")
        out.append((marker, data[pos + 4:pos + 2 + n]))
        pos += 2 + n
        if marker == 0xDA:
            return out, pos


def huffman_lookup(bits, values):
    """{(length, code): symbol}, codes of a length in increasing order (T.81 Annex C)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[length, code] = values[k]
            code += 1
            k += 1
        code <<= 1
    return out


def headers(data):
    """-> dict: h, w, factors [(h, v)] x 3, q [natural-order int64 (64,)] x 3, dc / ac [lookup] x 3, huffman {(class,
    slot): (bits, values)}, scan (the stuffed segment's bytes)."""
    segs, start = segments(data)
    qt, ht, sof, sos = {}, {}, None, None
    for marker, body in segs:
        if marker == 0xDB:
            at = 0
            while at < len(body):
                if body[at] >> 4:
                    raise ValueError("16-bit quantisation table")
                nat = np.zeros(64, dtype=np.int64)
                nat[ZIGZAG] = np.frombuffer(body[at + 1:at + 65], dtype=np.uint8)
                qt[body[at] & 15] = nat
                at += 65
        elif marker == 0xC4:
            at = 0
            while at < len(body):
                bits = body[at + 1:at + 17]
                n = sum(bits)
                ht[body[at] >> 4, body[at] & 15] = (bytes(bits), bytes(body[at + 17:at + 17 + n]))
                at += 17 + n
        elif marker == 0xC0:
            sof = body
        elif 0xC1 <= marker <= 0xCF and marker not in (0xC4, 0xC8, 0xCC):
            raise ValueError("SOF%d" % (marker - 0xC0))
        elif marker == 0xDD and int.from_bytes(body[:2], "big"):
            raise ValueError("restart interval")
        elif marker == 0xDA:
            sos = body
    if sof is None or sof[0] != 8 or sof[5] != 3 or sos[0] != 3:
        raise ValueError("not an 8-bit three-component frame in one scan")
    comps = [(sof[6 + 3 * i], (sof[7 + 3 * i] >> 4, sof[7 + 3 * i] & 15), sof[8 + 3 * i]) for i in range(3)]
    factors = [c[1] for c in comps]
    if factors not in ([(2, 2), (1, 1), (1, 1)], [(1, 1), (1, 1), (1, 1)]):
        raise ValueError("sampling %r" % (factors,))
    end = data.rindex(b"\xff\xd9")
    tables = {k: huffman_lookup(*v) for k, v in ht.items()}
    return {"h": int.from_bytes(sof[1:3], "big"), "w": int.from_bytes(sof[3:5], "big"), "factors": factors,
            "q": [qt[c[2]] for c in comps], "dc": [tables[0, sos[2 + 2 * i] >> 4] for i in range(3)],
            "ac": [tables[1, sos[2 + 2 * i] & 15] for i in range(3)], "huffman": ht, "scan": data[start:end]}


class BitReader:
    """MSB-first reader of the segment without its stuffing bytes.  Python's big-integer shifts are linear in the number's
    size, so the bits are taken from a few bytes at a time."""

    def __init__(self, stuffed):
        self.data = stuffed.replace(b"\xff\x00", b"\xff")
        self.total = 8 * len(self.data)
        self.pos = 0

    def peek(self, n):
        """the next n bits, 1-bits behind the end"""
        first, last = self.pos >> 3, (self.pos + n + 7) >> 3
        piece = self.data[first:last]
        v = int.from_bytes(piece + b"\xff" * (last - first - len(piece)), "big")
        return (v >> (8 * last - self.pos - n)) & ((1 << n) - 1)

    def take(self, n):
        if self.pos + n > self.total:
            raise ValueError("stream exhausted")
        v = self.peek(n) if n else 0
        self.pos += n
        return v

    def symbol(self, table):
        window = self.peek(16)
        for length in range(1, 17):
            hit = table.get((length, window >> (16 - length)))
            if hit is not None:
                self.take(length)
                return hit
        raise ValueError("invalid code")


def _extend(v, size):
    return v - (1 << size) + 1 if size and v < (1 << (size - 1)) else v


def coefficients(info, stats=None):
    """-> int64 (blocks in scan order, 64) in zigzag order, and the component of every block.  stats, when given, collects
    `dc_sizes` (set), `zrl` (count), `eob_only` (blocks with no AC symbol but EOB)."""
    h, w = info["h"], info["w"]
    big = info["factors"][0] == (2, 2)
    mcu = 16 if big else 8
    nmcu = -(-h // mcu) * -(-w // mcu)
    order = [0, 0, 0, 0, 1, 2] if big else [0, 1, 2]
    rd = BitReader(info["scan"])
    out = np.zeros((nmcu * len(order), 64), dtype=np.int64)
    pred = [0, 0, 0]
    b = 0
    for _ in range(nmcu):
        for c in order:
            size = rd.symbol(info["dc"][c])
            if stats is not None:
                stats.setdefault("dc_sizes", set()).add(size)
            pred[c] += _extend(rd.take(size), size)
            out[b, 0] = pred[c]
            k, symbols = 1, 0
            while k < 64:
                rs = rd.symbol(info["ac"][c])
                symbols += 1
                run, size = rs >> 4, rs & 15
                if size == 0:
                    if run != 15:
                        if stats is not None and symbols == 1:
                            stats["eob_only"] = stats.get("eob_only", 0) + 1
                        break
                    if stats is not None:
                        stats["zrl"] = stats.get("zrl", 0) + 1
                    k += 16
                    continue
                k += run
                if k > 63:
                    raise ValueError("run past 63")
                out[b, k] = _extend(rd.take(size), size)
                k += 1
            b += 1
    return out, order


def _idct_1d(d, shift):
    """One pass of jidctint.c over the last axis of d (..., 8)."""
    i = [d[..., k] for k in range(8)]
    z1 = (i[2] + i[6]) * 4433
    t2, t3 = z1 - i[6] * 15137, z1 + i[2] * 6270
    t0, t1 = (i[0] + i[4]) << 13, (i[0] - i[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = (z3 + z4) * 9633
    o0, o1, o2, o3 = o0 * 2446, o1 * 16819, o2 * 25172, o3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    r = 1 << (shift - 1)
    out = [t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3]
    return np.stack([(v + r) >> shift for v in out], axis=-1)


def samples(coef, q):
    """(n, 64) zigzag coefficients of one component -> (n, 8, 8) samples 0..255."""
    nat = np.zeros_like(coef)
    nat[:, ZIGZAG] = coef
    d = (nat * q).reshape(-1, 8, 8)
    d = _idct_1d(d.swapaxes(-1, -2), 11).swapaxes(-1, -2)      # columns first
    d = _idct_1d(d, 18)                                         # then rows
    return np.clip(d + 128, 0, 255)


def _fancy(p):
    """jdsample.c's h2v2 upsampling of the true chroma plane p (rows, cols) -> (2 rows, 2 cols): h2v2_fancy_upsample, edges
    replicating themselves, for a plane more than two columns wide; plain 2 x 2 replication (h2v2_upsample) otherwise."""
    if p.shape[1] <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    up, down = np.vstack([p[:1], p[:-1]]), np.vstack([p[1:], p[-1:]])
    rows = np.empty((2 * p.shape[0], p.shape[1]), dtype=np.int64)
    rows[0::2], rows[1::2] = 3 * p + up, 3 * p + down
    left, right = np.hstack([rows[:, :1], rows[:, :-1]]), np.hstack([rows[:, 1:], rows[:, -1:]])
    out = np.empty((rows.shape[0], 2 * rows.shape[1]), dtype=np.int64)
    out[:, 0::2], out[:, 1::2] = (3 * rows + left + 8) >> 4, (3 * rows + right + 7) >> 4
    return out


def decode(data, stats=None):
    info = headers(bytes(data))
    h, w = info["h"], info["w"]
    coef, order = coefficients(info, stats)
    big = len(order) == 6
    mcu = 16 if big else 8
    mh, mw = -(-h // mcu), -(-w // mcu)
    coef = coef.reshape(mh, mw, len(order), 64)
    planes = []
    for c in range(3):
        idx = [k for k, o in enumerate(order) if o == c]
        s = samples(coef[:, :, idx].reshape(-1, 64), info["q"][c]).reshape(mh, mw, len(idx), 8, 8)
        if len(idx) == 4:
            s = s.reshape(mh, mw, 2, 2, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(mh * 16, mw * 16)
        else:
            s = s[:, :, 0].transpose(0, 2, 1, 3).reshape(mh * 8, mw * 8)
        planes.append(s)
    y, cb, cr = planes
    if big:
        ch, cw = -(-h // 2), -(-w // 2)
        cb, cr = _fancy(cb[:ch, :cw]), _fancy(cr[:ch, :cw])
    y, cb, cr = y[:h, :w], cb[:h, :w] - 128, cr[:h, :w] - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)
