"""The PNG format of INTEGRATION.md 4n restated in numpy / Python from the PNG specification and RFC 1950 / 1951, and a
decoder-side checker that trusts nothing but zlib: the oracle of the device encoder (dualdiff_amd/csrc/png.hip), which must
produce these bytes.

    encode(img)            (H, W, 3) uint8 -> the .png file
    check(data)            -> (pixels, filter types): parses the chunks, verifies every CRC with zlib.crc32, inflates the
                           joined IDAT payloads with zlib.decompress, unfilters in numpy; raises AssertionError
    choose_filters(img)    the per-row filter choice

The rules: per row the filter type 0..4 with the smallest sum of `b if b < 128 else 256 - b`, ties to the lowest type; the
filtered stream in chunks of 16384 bytes; per chunk, per run of equal bytes: one literal, then matches (distance 1) of 258,
then a match of the rest if it is at least 3, else literals; one dynamic-Huffman block per chunk (code lengths limited to 15,
the code-length code to 7, one distance code of length 1, the header's code lengths with the repeat codes 16..18 per run
of equal lengths) followed by an empty stored block that aligns the chunk and carries BFINAL in the last chunk, or one
stored block where the dynamic form has more bytes; one IDAT per chunk, the zlib header in the first, the Adler-32 in the
last.
"""
import collections
import struct
import zlib

import numpy as np

CHUNK = 16384
SIGNATURE = b"\x89PNG\r\n\x1a\n"
FILE_FIXED = 8 + 25 + 12 + 2 + 4                 # signature, IHDR, IEND, zlib header, Adler-32
CHUNK_FIXED = 12 + 5                             # IDAT length / type / CRC, a stored block's header
# RFC 1951 3.2.5: length codes 257..285
LENGTH_BASE = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
                        227, 258])
LENGTH_EXTRA = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0])
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def worst_case(h, w):
    """The file's length with every chunk stored."""
    n = h * (1 + 3 * w)
    return FILE_FIXED + CHUNK_FIXED * (-(-n // CHUNK)) + n


# ---- filtering ----------------------------------------------------------------------------------------------------------

def _neighbours(raw):
    a = np.zeros_like(raw)
    a[:, 3:] = raw[:, :-3]
    b = np.zeros_like(raw)
    b[1:] = raw[:-1]
    c = np.zeros_like(raw)
    c[1:, 3:] = raw[:-1, :-3]
    return a, b, c


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_candidates(img):
    """-> (5, H, 3 W) uint8: every row filtered by every type, the row above being the raw row."""
    h, w, _ = img.shape
    raw = img.reshape(h, 3 * w).astype(np.int64)
    a, b, c = _neighbours(raw)
    return np.stack([(raw - p) & 255 for p in (0 * raw, a, b, (a + b) >> 1, _paeth(a, b, c))]).astype(np.uint8)


def choose_filters(img, cand=None):
    cand = filter_candidates(img) if cand is None else cand
    v = cand.astype(np.int64)
    cost = np.where(v < 128, v, 256 - v).sum(axis=2)
    return np.argmin(cost, axis=0)                       # the first minimum: ties to the lowest type


def filtered_stream(img):
    cand = filter_candidates(img)
    types = choose_filters(img, cand)
    rows = cand[types, np.arange(img.shape[0])]
    return np.concatenate([types[:, None].astype(np.uint8), rows], axis=1).reshape(-1)


# ---- tokens -------------------------------------------------------------------------------------------------------------

def tokens(chunk):
    """The tokens of one chunk in stream order -> (symbol, extra bits, extra value, is a match), and the `rest` (run length
    minus the first literal) of every run."""
    chunk = np.asarray(chunk, dtype=np.uint8)
    n = len(chunk)
    starts = np.flatnonzero(np.concatenate([[True], chunk[1:] != chunk[:-1]]))
    rest = np.diff(np.concatenate([starts, [n]])) - 1
    full, rem = rest // 258, rest % 258
    pos, length = [starts], [np.zeros(len(starts), dtype=np.int64)]
    # matches of 258
    run = np.repeat(np.arange(len(starts)), full)
    k = np.arange(len(run)) - np.repeat(np.cumsum(full) - full, full)
    pos.append(starts[run] + 1 + 258 * k)
    length.append(np.full(len(run), 258, dtype=np.int64))
    # the rest: one match, or literals
    tail = starts + 1 + 258 * full
    m = rem >= 3
    pos.append(tail[m])
    length.append(rem[m])
    few = np.where(m, 0, rem)
    run = np.repeat(np.arange(len(starts)), few)
    k = np.arange(len(run)) - np.repeat(np.cumsum(few) - few, few)
    pos.append(tail[run] + k)
    length.append(np.zeros(len(run), dtype=np.int64))
    pos, length = np.concatenate(pos), np.concatenate(length)
    order = np.argsort(pos, kind="stable")
    pos, length = pos[order], length[order]
    match = length > 0
    idx = np.searchsorted(LENGTH_BASE, np.where(match, length, 3), side="right") - 1
    sym = np.where(match, 257 + idx, chunk[pos])
    eb = np.where(match, LENGTH_EXTRA[idx], 0)
    ev = np.where(match, length - LENGTH_BASE[idx], 0)
    return sym, eb, ev, match.astype(np.int64), rest


# ---- Huffman codes ------------------------------------------------------------------------------------------------------

def tree_depths(hist):
    """Huffman's algorithm with two queues over the used symbols sorted by (count, symbol), a leaf before an internal node
    on equal weight -> [(symbol, depth)] in that sorted order (the depths are NOT limited)."""
    used = sorted((int(f), s) for s, f in enumerate(hist) if f)
    if len(used) == 1:
        return [(used[0][1], 1)]
    leaves = collections.deque((f, i) for i, (f, _) in enumerate(used))
    inner = collections.deque()
    parent = {}
    nxt = len(used)

    def take():
        if not inner or (leaves and leaves[0][0] <= inner[0][0]):
            return leaves.popleft()
        return inner.popleft()
    while len(leaves) + len(inner) > 1:
        (fa, a), (fb, b) = take(), take()
        parent[a] = parent[b] = nxt
        inner.append((fa + fb, nxt))
        nxt += 1
    out = []
    for i, (_, s) in enumerate(used):
        d, node = 0, i
        while node in parent:
            node = parent[node]
            d += 1
        out.append((s, d))
    return out


def code_lengths(hist, limit):
    """-> the code length of every symbol (0: unused).  The tree's leaves per depth, depths above the limit folded into it;
    while the Kraft sum is too large, one code of the limit is dropped and the deepest shorter code is split in two; the
    lengths then go to the sorted symbols, longest first."""
    depths = tree_depths(hist)
    count = [0] * (limit + 1)
    for _, d in depths:
        count[min(d, limit)] += 1
    total = sum(count[d] << (limit - d) for d in range(1, limit + 1))
    while total > 1 << limit:
        count[limit] -= 1
        d = max(d for d in range(1, limit) if count[d])
        count[d] -= 1
        count[d + 1] += 2
        total -= 1
    lens = [0] * len(hist)
    at = 0
    for d in range(limit, 0, -1):
        for _ in range(count[d]):
            lens[depths[at][0]] = d
            at += 1
    assert at == len(depths)
    return lens


def canonical_codes(lens):
    """RFC 1951 3.2.2 -> every symbol's code, bit-reversed: as a value whose bit 0 goes first into the LSB-first stream."""
    limit = max(lens)
    count = [0] * (limit + 1)
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * (limit + 1)
    for d in range(1, limit + 1):
        code = (code + count[d - 1]) << 1
        nxt[d] = code
    out = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            out[s] = int(format(nxt[l], "0%db" % l)[::-1], 2)
            nxt[l] += 1
    return out


def header_lengths(seq):
    """The code lengths of a block header as RFC 1951 3.2.7 codes them -> [(symbol 0..18, extra value, extra bits)].  Per run
    of equal lengths: zeros as repeats of up to 138 while at least 3 are left (symbol 18 for 11..138, symbol 17 for
    3..10), then single zeros; another length once, then repeats of up to 6 (symbol 16) while at least 3 are left, then
    the length itself."""
    out, i = [], 0
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        i += r
        if v:
            out.append((v, 0, 0))
            r -= 1
        while r >= 3:
            t = min(r, 6 if v else 138)
            out.append((16, t - 3, 2) if v else ((18, t - 11, 7) if t >= 11 else (17, t - 3, 3)))
            r -= t
        out += [(v, 0, 0)] * r
    return out


# ---- blocks -------------------------------------------------------------------------------------------------------------

def _bits(values, nbits):
    """values[i]'s low nbits[i] bits, LSB first, one after another -> uint8 array of bits"""
    values, nbits = np.asarray(values, dtype=np.uint64), np.asarray(nbits, dtype=np.int64)
    start = np.cumsum(nbits) - nbits
    tok = np.repeat(np.arange(len(nbits)), nbits)
    k = np.arange(int(nbits.sum())) - np.repeat(start, nbits)
    return ((values[tok] >> k.astype(np.uint64)) & np.uint64(1)).astype(np.uint8)


def deflate_chunk(chunk, last, stats=None):
    """One chunk's bytes of the deflate stream."""
    n = len(chunk)
    sym, eb, ev, match, rest = tokens(chunk)
    hist = np.bincount(sym, minlength=286)
    hist[256] = 1
    lens = code_lengths(hist, 15)
    codes = canonical_codes(lens)
    nlit = max(257, int(np.flatnonzero(hist).max()) + 1)
    listed = header_lengths(lens[:nlit] + [1])           # ... and the one distance code, of length 1
    cl_hist = np.bincount([s for s, _, _ in listed], minlength=19)
    cl_lens = code_lengths(cl_hist, 7)
    cl_codes = canonical_codes(cl_lens)
    hclen = max(4, max(k + 1 for k in range(19) if cl_lens[CL_ORDER[k]]))
    lens_a, codes_a = np.array(lens, dtype=np.int64), np.array(codes, dtype=np.int64)
    values = [0, 2, nlit - 257, 0, hclen - 4] + [cl_lens[CL_ORDER[k]] for k in range(hclen)]
    nbits = [1, 2, 5, 5, 4] + [3] * hclen
    for s, extra, xbits in listed:
        values += [cl_codes[s], extra]
        nbits += [cl_lens[s], xbits]
    tok_values = codes_a[sym] | (ev << lens_a[sym])      # the distance code is a 0 bit behind the extra bits
    tok_bits = lens_a[sym] + eb + match
    bits = np.concatenate([_bits(values, nbits), _bits(tok_values, tok_bits), _bits([codes[256]], [lens[256]]),
                           _bits([1 if last else 0, 0], [1, 2])])
    bits = np.concatenate([bits, np.zeros(-len(bits) % 8, dtype=np.uint8)])
    dynamic = np.packbits(bits, bitorder="little").tobytes() + b"\x00\x00\xff\xff"
    stored = bytes([1 if last else 0]) + struct.pack("<HH", n, n ^ 0xFFFF) + bytes(chunk)
    use = stored if len(dynamic) > len(stored) else dynamic
    if stats is not None:
        stats.setdefault("chunks", []).append({"stored": use is stored, "bytes": len(use), "hist": hist, "cl_hist": cl_hist,
                                               "lens": lens, "cl_lens": cl_lens, "rest": rest, "matches": int(match.sum())})
    return use


def _png_chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload))


def encode(img, stats=None):
    img = np.ascontiguousarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3 and img.size
    h, w, _ = img.shape
    stream = filtered_stream(img)
    pieces = [stream[i:i + CHUNK] for i in range(0, len(stream), CHUNK)]
    out = SIGNATURE + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
    for i, piece in enumerate(pieces):
        last = i == len(pieces) - 1
        payload = (b"\x78\x01" if i == 0 else b"") + deflate_chunk(piece, last, stats)
        if last:
            payload += struct.pack(">I", zlib.adler32(stream.tobytes()))
        out += _png_chunk(b"IDAT", payload)
    return out + _png_chunk(b"IEND", b"")


def model_size(img):
    """What the issue compares a file's length with: zlib's own Z_RLE deflate of every chunk of the same filtered bytes,
    plus this format's fixed bytes (per file FILE_FIXED; per chunk the IDAT's 12 and the aligning block's LEN / NLEN)."""
    stream = filtered_stream(img).tobytes()
    total = FILE_FIXED
    for i in range(0, len(stream), CHUNK):
        z = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
        total += len(z.compress(stream[i:i + CHUNK]) + z.flush()) + 12 + 4
    return total


# ---- the checker --------------------------------------------------------------------------------------------------------

def parse(data):
    """-> [(type, payload)], every length and CRC verified, nothing behind IEND"""
    assert data[:8] == SIGNATURE, "signature"
    at, chunks = 8, []
    while at < len(data):
        assert at + 12 <= len(data), "a chunk is cut off"
        n, = struct.unpack(">I", data[at:at + 4])
        kind, payload = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        assert len(payload) == n and at + 12 + n <= len(data), "a chunk is cut off"
        crc, = struct.unpack(">I", data[at + 8 + n:at + 12 + n])
        assert crc == zlib.crc32(kind + payload), "CRC of chunk %d (%r)" % (len(chunks), kind)
        chunks.append((kind, payload))
        at += 12 + n
        if kind == b"IEND":
            break
    assert at == len(data), "bytes behind IEND"
    return chunks


def unfilter(types, rows):
    """types (H,), rows (H, W, 3) filtered -> pixels, along the anti-diagonals x + y (a pixel needs its left, upper and
    upper-left neighbours only)."""
    h, w, _ = rows.shape
    rec = np.zeros((h + 1, w + 1, 3), dtype=np.int64)
    f = np.asarray(types)[:, None]
    for d in range(h + w - 1):
        ys = np.arange(max(0, d - w + 1), min(h - 1, d) + 1)
        xs = d - ys
        a, b, c = rec[ys + 1, xs], rec[ys, xs + 1], rec[ys, xs]
        t = f[ys]
        pred = np.where(t == 1, a, np.where(t == 2, b, np.where(t == 3, (a + b) >> 1, np.where(t == 4, _paeth(a, b, c), 0))))
        rec[ys + 1, xs + 1] = (rows[ys, xs] + pred) & 255
    return rec[1:, 1:].astype(np.uint8)


def check(data):
    """-> (pixels (H, W, 3) uint8, filter types (H,)) of a file of this format's kind: 8-bit RGB, no interlace, IHDR then
    IDATs then IEND."""
    chunks = parse(bytes(data))
    kinds = [k for k, _ in chunks]
    assert kinds[0] == b"IHDR" and kinds[-1] == b"IEND" and len(kinds) >= 3 and set(kinds[1:-1]) == {b"IDAT"}, kinds
    assert len(chunks[0][1]) == 13 and chunks[-1][1] == b""
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 2, 0, 0, 0) and w > 0 and h > 0
    z = b"".join(p for _, p in chunks[1:-1])
    assert (z[0] & 15) == 8 and (z[0] >> 4) <= 7 and not z[1] & 32 and (z[0] * 256 + z[1]) % 31 == 0, "zlib header"
    d = zlib.decompressobj()
    raw = d.decompress(z)
    assert d.eof and d.unused_data == b"" and len(raw) == h * (1 + 3 * w), "inflated length"
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(h, 1 + 3 * w)
    types = rows[:, 0].astype(np.int64)
    assert types.max() <= 4
    return unfilter(types, rows[:, 1:].reshape(h, w, 3).astype(np.int64)), types
