"""Nearest upsample + 3x3 conv as a 2 x 2-tap conv on the SOURCE image (the sub-pixel decomposition), host side.

Under torch's nearest map the three taps of an output coordinate o read at most two distinct source pixels whenever
in / out <= 1 leaves no coordinate that sees s - 1, s, s + 1.  With s = src(o) a coordinate is of

    class 0   taps read (s-1 | s  s)     slot weights (W-1      | W0 + W1)
    class 1   taps read (s  s | s+1)     slot weights (W-1 + W0 | W1)
    class 2   taps read (s-1 | s), tap +1 outside the output (last coordinate of an odd size): (W-1 | W0)

and a tap outside the output needs nothing where its slot lies outside the source image (coordinate 0 of class 0, the
last one of class 1): the kernel's gather delivers zeros there, exactly like the zero padding of the upsampled image.  A
pixel's class is (row class, column class); each non-empty class has its own weight matrix [cout][2][2][cin], the 3x3 tap
slices that read one source pixel summed in fp32 and rounded once.  csrc/gemm.hip classifies with the same arithmetic
(upfold_class) and refuses a descriptor whose map has a coordinate without a class.
"""
import functools

import numpy as np
import torch

MAX_OUT = 64                                              # kUpfoldMax of csrc/gemm_tiles.h
SLOT_TAPS = (((0,), (1, 2)), ((0, 1), (2,)), ((0,), (1,)))      # class -> (taps summed into slot 0, into slot 1)


def src(o, n_in, n_out):
    """torch nearest with a float scale, as the kernels compute it: min(floor(o * (float)(in / out)), in - 1)."""
    scale = np.float32(n_in) / np.float32(n_out)
    return min(int(np.floor(np.float32(o) * scale)), n_in - 1)


def axis_class(o, n_in, n_out):
    """Class of output coordinate o, or None where no class reproduces its taps."""
    s = src(o, n_in, n_out)
    for c in range(3):
        ok = True
        for t in (-1, 0, 1):
            tap_in = 0 <= o + t < n_out
            if c == 2 and t == 1:
                ok = not tap_in
            else:
                pos = (s if c == 1 else s - 1) + ((t == 1) if c == 1 else (t >= 0))
                src_in = 0 <= pos < n_in
                ok = (src_in and src(o + t, n_in, n_out) == pos) if tap_in else not src_in
            if not ok:
                break
        if ok:
            return c
    return None


@functools.lru_cache(maxsize=None)
def _axis_classes(n_in, n_out):
    if n_in <= 0 or n_out <= n_in or n_out > MAX_OUT:
        return None
    cls = tuple(axis_class(o, n_in, n_out) for o in range(n_out))
    return None if None in cls else cls


def axis_classes(n_in, n_out):
    """[class of every output coordinate], or None where the fold does not apply to this axis (memoised per size pair:
    the layers ask on every call)."""
    cls = _axis_classes(int(n_in), int(n_out))
    return None if cls is None else list(cls)


@functools.lru_cache(maxsize=None)
def _classes(hin, win, hv, wv):
    ycls, xcls = _axis_classes(hin, hv), _axis_classes(win, wv)
    if ycls is None or xcls is None:
        return None
    return ycls, xcls, tuple((rc, cc) for rc in range(3) for cc in range(3) if rc in ycls and cc in xcls)


def classes(hin, win, hv, wv):
    """(row classes, column classes, [(row class, column class) of every non-empty pixel class, in weight order]) or None."""
    c = _classes(int(hin), int(win), int(hv), int(wv))
    return None if c is None else (list(c[0]), list(c[1]), list(c[2]))


def num_classes(hin, win, hv, wv):
    """Non-empty pixel classes of the map (the folded weight holds one matrix per class), 0 where the fold does not apply."""
    c = _classes(int(hin), int(win), int(hv), int(wv))
    return 0 if c is None else len(c[2])


def ok(hin, win, hv, wv, cin=64, stride=1):
    """The dispatch predicate: stride 1, whole 64-channel K steps, both sizes within the kernel's coordinate lists, and
    every output row and column with a class."""
    return stride == 1 and cin % 64 == 0 and num_classes(hin, win, hv, wv) > 0


def fold_weight(w, hin, win, hv, wv, sum_dtype=torch.float32, out_dtype=None):
    """w: packed [cout][ky][kx][cin] as (cout, 9 * cin).  Returns (ncls * cout, 4 * cin): one [cout][sy][sx][cin] matrix
    per non-empty class, summed in `sum_dtype` and rounded once to `out_dtype` (default: w's)."""
    cl = classes(hin, win, hv, wv)
    if cl is None:
        raise ValueError("no folded form for the nearest map %dx%d -> %dx%d" % (hin, win, hv, wv))
    cout = w.shape[0]
    w9 = w.detach().reshape(cout, 3, 3, -1).to(sum_dtype)
    mats = []
    for rc, cc in cl[2]:
        f = w9.new_zeros((cout, 2, 2, w9.shape[3]))
        for sy in range(2):
            for sx in range(2):
                for ky in SLOT_TAPS[rc][sy]:
                    for kx in SLOT_TAPS[cc][sx]:
                        f[:, sy, sx] += w9[:, ky, kx]
        mats.append(f.reshape(cout, -1))
    return torch.cat(mats, 0).to(out_dtype or w.dtype).contiguous()
