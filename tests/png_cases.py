"""The named inputs of the PNG tests (tests/test_png_output_cpu.py, tests/test_png_output_gpu.py), the smallest at which
each part of the encoder can go wrong, and the size margins of the format.

    python -m tests.png_cases --margins      recomputes MARGINS on the CPU from the reference encoder alone

A case is (name, frame (H, W, 3) uint8, noise).  `noise` marks the inputs no deflate can shrink: uniform noise, and the
frames of a few pixels; the size conditions are about the others.  The two natural crops come from the fixture
(tests/golden/png_output.npz, minted by tests/golden/mint_png.py); everything else is generated here and the fixture pins it.

The size condition: a file may exceed the model (tests/png_reference.py: model_size — zlib's own Z_RLE deflate of the same
filtered chunks plus the format's fixed bytes) by at most MARGINS[name] percent.  The margins are what the REFERENCE encoder
needs, rounded up to a whole percentage point and one more added: they come from the format (its Huffman codes are built
per chunk like zlib's, by another tie rule and another length limiting; the aligning block costs a byte more than the
model counts; a distance code is always listed), not from the device code.
"""
import collections
import functools
import os
import sys

import numpy as np

from tests import png_reference as R
from tests.golden import mint_jpeg as MJ

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_output.npz")
CROPS = ("crop_object", "crop_road")           # 64 x 96 crops of the reference's media/day_object_case.png, day_road_case.png
Case = collections.namedtuple("Case", "name img noise")
RUN_RESTS = (3, 4, 259, 260, 261, 262, 517)    # run lengths behind the first literal that the `runs` case holds
FIB = (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181)

# percent over the model, per non-noise case: `python -m tests.png_cases --margins`
MARGINS = {
    '64x85_one_chunk': 1,
    '128x85_two_chunks': 1,
    '113x48_one_over': 1,
    '129x42_one_under': 1,
    '1x5461_row_is_chunk': 1,
    '2x5461_row_is_chunk': 1,
    '2x5462_row_straddles': 2,
    'runs': 1,
    'zeros_64x100': 3,
    'flat_64x100': 1,
    'tiles_40x72': 1,
    'single_symbol': 17,
    'fibonacci': 1,
    'cl_fibonacci': 1,
    'gradient_224x400': 1,
    'crop_object': 1,
    'crop_road': 1,
    'large': 1,
}


def _by_cost():
    """byte values, the cheapest for the filter heuristic first: 0, 1, 255, 2, 254, ..."""
    return sorted(range(256), key=lambda v: (min(v, 256 - v), v))


def _mixed(h, w, seed):
    """a smooth gradient with flat patches and a band of noise: literals, short and long runs in one frame"""
    rs = np.random.RandomState(seed)
    img = MJ.content("smooth", h, w, seed).copy()
    img[h // 3:h // 3 + max(h // 6, 1), w // 4:w // 4 + max(w // 5, 1)] = rs.randint(0, 256, 3)
    y0 = (2 * h) // 3
    img[y0:y0 + max(h // 8, 1), : max(w // 3, 1)] = rs.randint(0, 256, (max(h // 8, 1), max(w // 3, 1), 3))
    return img


def _row_from_sub(stream):
    """A one-row frame whose filtered row is `stream` under the Sub filter, and for which the rule does choose Sub."""
    d = np.asarray(stream, dtype=np.int64).reshape(-1, 3)
    img = (np.cumsum(d, axis=0) % 256).astype(np.uint8)[None]
    if int(R.choose_filters(img)[0]) != 1:
        return None
    return img


def _spread(counts, seed=None):
    """A sequence that holds value v counts[v] times with no four equal bytes in a row (so the rule finds no match): always
    the value with the most copies left that would not make a fourth; seed: a random order instead."""
    left = dict(counts)
    if seed is not None:
        seq = np.repeat(list(left), list(left.values()))
        np.random.RandomState(seed).shuffle(seq)
        return seq
    out = []
    while left:
        order = sorted(left, key=lambda v: (-left[v], v))
        v = order[0]
        if len(out) >= 3 and out[-1] == out[-2] == out[-3] == v:
            v = order[1]
        out.append(v)
        left[v] -= 1
        if not left[v]:
            del left[v]
    return np.array(out)


def _from_histogram(counts):
    """A one-row frame whose one chunk (the filter byte 1 included) holds value v counts[v] times, all as literals."""
    counts = dict(counts)
    assert counts.get(1, 0) >= 1                             # the filter type byte is one of them
    counts[1] -= 1
    assert sum(counts.values()) % 3 == 0
    for seed in [None] + list(range(40)):
        seq = _spread({v: c for v, c in counts.items() if c}, seed)
        img = _row_from_sub(seq)
        if img is not None and not any(c["matches"] for c in _stats(img)["chunks"]):
            return img
    raise AssertionError("no arrangement found")


def _stats(img):
    stats = {}
    R.encode(img, stats)
    return stats


def _runs():
    """zero runs of 1 + r bytes for r in RUN_RESTS, one non-zero byte between them"""
    parts = [[1, 1]]
    for i, r in enumerate(RUN_RESTS):
        parts += [[0] * (1 + r), [1 + i % 2]]
    seq = [v for p in parts for v in p]
    seq += [2] * (-len(seq) % 3)
    return _row_from_sub(seq)


def _fibonacci():
    """16384 bytes, 18 values with the counts 1, 2, 3, 5, 8, ... (the rest on the most frequent one); the end-of-block
    symbol is the other 1 of the Fibonacci sequence.  Every merge of Huffman's algorithm then joins the tree so far and
    the next leaf, also with the leaf taken first on equal weight: the unconstrained tree is 18 deep"""
    values = _by_cost()
    counts = {values[len(FIB) - 1 - i]: f for i, f in enumerate(FIB)}
    counts[values[0]] += R.CHUNK - sum(FIB)
    return _from_histogram(counts)


def _cl_fibonacci():
    """1024 bytes whose Huffman code has 2, 5, 1, 8, 21, 3, 13 codes of the lengths 3..9 and 82 of length 10 (dyadic counts
    2^(10 - length), the end-of-block symbol being one of the 82; one more on one of the most frequent values), on byte
    values scattered so that few equal lengths are neighbours.  The header then lists the symbols 1, 5, 3, 8 with the
    counts 1, 1, 2, 3 and seven more with 5, 8, 13, 14, 21, 72, 82: the unconstrained code-length tree is 9 deep."""
    top = [0, 2, 254, 4, 252, 6, 250, 8, 248, 10, 246, 12]       # cheap for the filter rule: Sub wins the row
    values = top + [v for v in np.random.RandomState(1207).permutation(256).tolist() if v not in top]
    per_length = dict(zip(range(3, 10), (2, 5, 1, 8, 21, 3, 13)))
    per_length[10] = 81
    counts, at = {}, 0
    for length in sorted(per_length):
        for _ in range(per_length[length]):
            counts[values[at]] = 1 << (10 - length)
            at += 1
    counts[values[0]] += 1
    return _from_histogram(counts)


def _uniform256():
    return _from_histogram({v: R.CHUNK // 256 for v in range(256)})


def large():
    """900 x 1600: the upper half a smooth gradient, the lower half noise"""
    return _large()


@functools.lru_cache(maxsize=None)
def _large():
    h, w = 900, 1600
    img = MJ.content("smooth", h, w, 0).copy()
    img[h // 2:] = np.random.RandomState(2).randint(0, 256, (h - h // 2, w, 3))
    img.setflags(write=False)
    return img


def batch():
    """7 frames of 37 x 53 with mixed content"""
    kinds = ("uniform", "smooth", "flat", "tiles", "lone", "saturated")
    return np.stack([MJ.content(k, 37, 53, 700 + i) for i, k in enumerate(kinds)] + [_mixed(37, 53, 706)])


def synthetic():
    """Everything but the crops, generated: [Case]"""
    noise = lambda h, w, seed: MJ.content("uniform", h, w, seed)        # noqa: E731
    out = [
        # geometry (H x W)
        Case("1x1", noise(1, 1, 1), True), Case("1x7", noise(1, 7, 2), True), Case("7x1", noise(7, 1, 3), True),
        Case("5x3", noise(5, 3, 4), True),
        Case("64x85_one_chunk", _mixed(64, 85, 5), False),               # rows of 256 bytes, 16384 filtered bytes
        Case("128x85_two_chunks", _mixed(128, 85, 6), False),            # 2 x 16384
        Case("113x48_one_over", _mixed(113, 48, 7), False),              # 16385
        Case("129x42_one_under", _mixed(129, 42, 8), False),             # 16383
        Case("1x5461_row_is_chunk", _mixed(1, 5461, 9), False),
        Case("2x5461_row_is_chunk", _mixed(2, 5461, 10), False),
        Case("2x5462_row_straddles", _mixed(2, 5462, 11), False),
        # runs
        Case("runs", _runs(), False),
        Case("zeros_64x100", np.zeros((64, 100, 3), dtype=np.uint8), False),      # one run across the chunk end
        Case("flat_64x100", MJ.content("flat", 64, 100, 0), False),
        Case("tiles_40x72", MJ.content("tiles", 40, 72, 0), False),
        # Huffman
        Case("single_symbol", np.zeros((1, 100, 3), dtype=np.uint8), False),
        Case("uniform256", _uniform256(), True),
        Case("fibonacci", _fibonacci(), False),
        Case("cl_fibonacci", _cl_fibonacci(), False),
        # stored fallback
        Case("noise_64x100", noise(64, 100, 12), True),
        Case("gradient_224x400", MJ.content("smooth", 224, 400, 0), False),
    ]
    for c in out:
        assert c.img is not None, c.name
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """[Case]: the synthetic cases and the two natural crops of the fixture; shared, read-only"""
    z = np.load(GOLDEN)
    out = synthetic() + [Case(name, z["in_" + name], False) for name in CROPS]
    for c in out:
        c.img.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(the reference encoder's file, its statistics) of a case, or of "large"; computed once"""
    img = _large() if name == "large" else next(c.img for c in cases() if c.name == name)
    stats = {}
    return R.encode(img, stats), stats


def margin(img, data=None):
    """percent by which the reference's file exceeds the model, rounded up, plus one"""
    data = R.encode(img) if data is None else data
    over = 100.0 * (len(data) / R.model_size(img) - 1.0)
    return max(int(np.ceil(over)), 0) + 1


def main():
    if sys.argv[1:] != ["--margins"]:
        raise SystemExit(__doc__)
    got = {c.name: margin(c.img) for c in cases() if not c.noise}
    got["large"] = margin(_large())
    print("MARGINS = {")
    for name, m in got.items():
        print("    %r: %d," % (name, m))
    print("}")
    if got != MARGINS:
        raise SystemExit("the recorded MARGINS differ: %r" % {k: (MARGINS.get(k), v) for k, v in got.items() if MARGINS.get(k) != v})
    print("the recorded MARGINS are reproduced")


if __name__ == "__main__":
    main()
