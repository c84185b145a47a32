"""Run-time tile / split-K selection of the GEMM / conv launches, and the tracked table it starts from.

The step touches a finite set of GEMM / conv shapes.  On first (eager, non-captured) use of a shape every tile config x
split-K candidate of dd_gemm is timed with HIP events on a scratch output and the fastest is cached; graph capture then
records the tuned launches.  DD_AUTOTUNE=0 falls back to the built-in heuristic of csrc/gemm.hip.

The tuned table of the shapes the denoising step touches is TRACKED (dualdiff_amd/tuned/gfx950.json, written by
`bench.py --retune`) and loaded on first use, so every process launches the same kernels for the same shapes and the
bench's roofline line can be recomputed from profiles/.  Only shapes that are not in the table are timed at run time.
DD_TUNE_TABLE=0 ignores the tracked table, DD_TUNE_TABLE=<path> loads another one.
"""
import ast
import collections
import ctypes
import json
import os

import torch

from . import _workspace
from ._native import DD_EPI_GEGLU
from ._timer import _stream

_AUTOTUNE = os.environ.get("DD_AUTOTUNE", "1") != "0"
_COLD = os.environ.get("DD_AUTOTUNE_COLD", "1") != "0"
# DD_TUNE_CHALLENGE=52[,..]: tiles added after the tracked table was written are timed against every entry's incumbent
# the first time its shape is met (bench.py --challenge-tiles writes the table back).  The value in force is the one of
# the ops module (bench.py assigns it there); ops hands it to tune() with every call.
CHALLENGE_TILES = tuple(int(t) for t in os.environ.get("DD_TUNE_CHALLENGE", "").split(",") if t.strip())
TUNE_TABLE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned", "gfx950.json")
# The folded-upsample conv's own tracked table (conv_upfold_key -> tile, split-K): a row with tile 0 records a shape on which
# the folded form was measured no faster than the 9-tap launch, which the layer then keeps (upfold_tuned).
UPFOLD_TABLE_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned", "gfx950_upfold.json")
_UPFOLD = None
_TUNED = {}
_TABLE_LOADED = False
_CHALLENGED = set()
_FLUSH = {}
_TILES = None           # filled from the library (dd_gemm_tile_id) on first use
_SPLITS = (1, 2, 3, 4, 5, 6, 8, 12, 16)


# ---- the keys of the table: each kind's tuple is spelled here and nowhere else ------------------------------------
def gemm_key(rows, n, k, epilogue, dtype, a2=False, ln=False, *, out_f32=False, stats_out=False, stats_in=False,
             head_major=None, res=False, acc=False):
    """Dense call: dtype is the DD_* code, a2 / ln whether a second source / the LayerNorm fold is present, head_major
    the head dimension D of a head-major output; the flags follow in this fixed order."""
    return (("g", rows, n, k, epilogue, dtype, bool(a2), bool(ln))
            + (("f32",) if out_f32 else ()) + (("so",) if stats_out else ()) + (("si",) if stats_in else ())
            + (("hm", head_major) if head_major is not None else ())
            + (("res",) if res else ()) + (("acc",) if acc else ()))


def conv_key(m, hin, win, cin, cout, stride, hv, wv, dtype):
    """3x3 / pad 1 conv of m images hin x win (hv x wv after the nearest upsample)."""
    return ("c", m, hin, win, cin, cout, stride, hv, wv, dtype)


def conv_pad0_key(m, hin, win, cin, cout, stride, hv, wv, dtype):
    """conv3x3(pad=0): its own entries, the pad-1 keys are untouched."""
    return conv_key(m, hin, win, cin, cout, stride, hv, wv, dtype) + ("p0",)


def conv_upfold_key(m, hin, win, cin, cout, hv, wv, dtype):
    """conv3x3(upfold=...): the folded-upsample form, its own entries beside the 9-tap key of the same layer."""
    return conv_key(m, hin, win, cin, cout, 1, hv, wv, dtype) + ("uf",)


def upfold_tuned(key):
    """The tracked row (tile, split-K, 0) of a conv_upfold_key, or None; DD_TUNE_TABLE=0 ignores this table too."""
    global _UPFOLD
    if _UPFOLD is None:
        _UPFOLD = {}
        if os.environ.get("DD_TUNE_TABLE") != "0" and os.path.exists(UPFOLD_TABLE_PATH):
            with open(UPFOLD_TABLE_PATH) as f:
                blob = json.load(f)
            if blob.get("arch") != "gfx950":
                raise RuntimeError("tune cache %s is not for gfx950" % UPFOLD_TABLE_PATH)
            _UPFOLD = {ast.literal_eval(k): _entry(v) for k, v in blob["entries"]}
    return _UPFOLD.get(key)


# ---- the table -----------------------------------------------------------------------------------------------------
def _entry(v):
    """(tile, split-K, 0): the third value is a retired field every row carries as 0; the oldest tables have two."""
    return (int(v[0]), int(v[1]), int(v[2]) if len(v) > 2 else 0)


def tuned_table():
    return dict(_TUNED)


def save_tuned(path, merge=True):
    """Persist the tuned (tile, split-K) table so a later process skips the timing sweep.  merge: entries of
    an existing file that this process did not touch (other dtype, other batch) are kept."""
    entries = {}
    if merge and os.path.exists(path):
        with open(path) as f:
            for k, v in json.load(f).get("entries", []):
                entries[ast.literal_eval(k)] = _entry(v)
    entries.update(_TUNED)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"arch": "gfx950", "entries": [[repr(k), list(v)] for k, v in sorted(entries.items(), key=repr)]}, f, indent=0)


def load_tuned(path):
    """Load a table written by save_tuned(); entries for shapes already tuned here are kept."""
    with open(path) as f:
        blob = json.load(f)
    if blob.get("arch") != "gfx950":
        raise RuntimeError("tune cache %s is not for gfx950" % path)
    n = 0
    for k, v in blob["entries"]:
        key = ast.literal_eval(k)
        if key not in _TUNED:
            _TUNED[key] = _entry(v)
            n += 1
    return n


def _load_default_table():
    global _TABLE_LOADED
    if _TABLE_LOADED:
        return
    _TABLE_LOADED = True
    path = os.environ.get("DD_TUNE_TABLE", TUNE_TABLE_PATH)
    if path != "0" and os.path.exists(path):
        load_tuned(path)


def forget_tuned():
    """Drop every tuned entry (bench.py --retune) and do not read the tracked table again."""
    global _TABLE_LOADED
    _TUNED.clear()
    _TABLE_LOADED = True


# ---- the tuner -----------------------------------------------------------------------------------------------------
class Launcher(collections.namedtuple("Launcher", "lib pad_lo launch ws_bytes kernel_name")):
    """How a GemmDesc is launched for a given top / left padding: launch(d, stream) -> rc, ws_bytes(d), kernel_name(d)
    -> plan string.  What the tuner times is what the caller launches afterwards."""


def launcher(lib, pad_lo=1):
    """pad_lo 1: dd_gemm (every dense call, nn.Conv2d(padding=1)); 0: the dd_gemm_conv_pad launches of conv3x3(pad=0)."""
    if pad_lo == 1:
        return Launcher(lib, 1, lambda d, st: lib.dd_gemm(ctypes.byref(d), st),
                        lambda d: lib.dd_gemm_workspace_bytes(ctypes.byref(d)),
                        lambda d: lib.dd_gemm_kernel_name(ctypes.byref(d)).decode())
    return Launcher(lib, pad_lo, lambda d, st: lib.dd_gemm_conv_pad(ctypes.byref(d), pad_lo, st),
                    lambda d: lib.dd_gemm_conv_pad_workspace_bytes(ctypes.byref(d), pad_lo),
                    lambda d: lib.dd_gemm_conv_pad_kernel_name(ctypes.byref(d), pad_lo).decode())


def tune_candidates(lib, d):
    """(tile id, split-K) pairs the run-time tuner times for the call described by `d` — every tile of the library,
    split-K only where the K loop keeps >= 4 steps per slab and the slabs stay within 4096 128x128 blocks.  The planner
    may still turn a pair down (dd_gemm_kernel_name: "unsupported") or launch it in a normalised form."""
    global _TILES
    if _TILES is None:
        _TILES = tuple(lib.dd_gemm_tile_id(i) for i in range(lib.dd_gemm_num_tiles()))
    kt = (d.k + 63) // 64
    blocks128 = ((d.rows + 127) // 128) * ((d.n + 127) // 128)
    return [(tile, split) for tile in _TILES for split in _SPLITS
            if split == 1 or not (d.epilogue == DD_EPI_GEGLU or kt < 4 * split or blocks128 * split > 4096)]


def _capturing():
    return torch.cuda.is_current_stream_capturing()


def _flush_and_warm(device, warm):
    """Puts the caches in the state a launch sees inside the step: weights COLD (a step streams
    ~3.3 GB of them, far more than L2 + the 256 MiB Infinity Cache hold), activations just produced
    by the previous kernel and therefore WARM."""
    buf = _FLUSH.get(device)
    if buf is None:
        buf = _FLUSH[device] = torch.empty(320 << 20, dtype=torch.uint8, device=device)
    buf.zero_()
    for t in warm:
        if t is not None:
            t.sum()


def _time_launch(L, d, device, warm, tile, split, iters):
    """ms of one launch of `d` as (tile, split): the median of `iters` cold launches, or the mean of `iters` back-to-back
    ones with DD_AUTOTUNE_COLD=0; None when the library turns the pair down."""
    d.tile, d.split_k = tile, split
    _workspace.attach(d, device, lambda: L.ws_bytes(d))
    stream = _stream()
    if L.launch(d, stream) != 0:
        return None
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if not _COLD:
        e0.record()
        for _ in range(iters):
            L.launch(d, stream)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / iters
    samples = []
    for _ in range(iters):
        _flush_and_warm(device, warm)
        e0.record()
        L.launch(d, stream)
        e1.record()
        e1.synchronize()
        samples.append(e0.elapsed_time(e1))
    samples.sort()
    return samples[len(samples) // 2]         # median: one slow launch (clock ramp, a neighbour's burst) must not decide


def tune(L, d, key, out_shape, dtype, device, warm=(), challenge_tiles=()):
    """The table row (tile, split-K, 0) of `key`, timing the candidates of descriptor `d` through launcher `L` on a
    scratch output when the table has none; (0, 0, 0) — the library's own plan — when it may not time (DD_AUTOTUNE=0,
    graph capture) or no candidate launched.  `d` comes back as it was."""
    _load_default_table()
    hit = _TUNED.get(key)
    if hit is not None and (not challenge_tiles or key in _CHALLENGED or _capturing()):
        return hit
    if hit is None and (not _AUTOTUNE or _capturing()):
        return 0, 0, 0
    saved = (d.out, d.ldc, d.accumulate, d.tile, d.split_k, d.ws, d.ws_bytes)
    scratch = torch.empty(out_shape, dtype=dtype, device=device)
    d.out, d.ldc, d.accumulate = scratch.data_ptr(), scratch.stride(0), 0
    try:
        best = _challenge(L, d, key, hit, device, warm, challenge_tiles) if hit is not None else _sweep(L, d, device, warm)
    finally:
        (d.out, d.ldc, d.accumulate, d.tile, d.split_k, d.ws, d.ws_bytes) = saved
    if best[0] != 0:
        # (no candidate launched: the call is one no kernel can run.  Caching (0, 0, 0) would let save_tuned() write
        # it into the tracked table; the call itself goes on to the library's own plan and raises from there.)
        _TUNED[key] = best
    return best


def _sweep(L, d, device, warm):
    best, best_t = (0, 0, 0), float("inf")
    cands = []
    excl = {int(t) for t in os.environ.get("DD_TUNE_EXCLUDE", "").split(",") if t.strip()}   # A/B experiments
    for tile, split in tune_candidates(L.lib, d):
        if tile in excl:
            continue
        t = _time_launch(L, d, device, warm, tile, split, 3)            # >= 3 samples per candidate, cold or hot
        if t is not None:
            cands.append((t, tile, split))
    # the coarse pass is noisy: re-time the front-runners with more launches
    cands.sort()
    for t, tile, split in cands[:8]:
        t2 = _time_launch(L, d, device, warm, tile, split, 15 if _COLD else 12)
        if t2 is not None and t2 < best_t:
            best, best_t = (tile, split, 0), t2
    return best


def _challenge(L, d, key, hit, device, warm, challenge_tiles):
    """A new tile asks for the shapes of the tracked table: time the incumbent against the challengers only."""
    _CHALLENGED.add(key)
    t_inc = _time_launch(L, d, device, warm, hit[0], hit[1], 21)
    best, best_t = tuple(hit), (t_inc if t_inc is not None else float("inf"))
    for tile in challenge_tiles:
        for split in sorted({1, max(1, int(hit[1]))}):
            if (tile, split) == tuple(hit[:2]):
                continue
            t = _time_launch(L, d, device, warm, tile, split, 5)
            if t is None or t > 1.1 * best_t:
                continue
            t = _time_launch(L, d, device, warm, tile, split, 21)
            if t is not None and t < 0.97 * best_t:          # a challenger must win by 3 %: the medians carry ~2 % of noise
                best, best_t = (tile, split, 0), t
    if best != tuple(hit):
        print("[tune] %s: %s -> %s (%.1f -> %.1f us)" % (key, tuple(hit), best, t_inc * 1e3, best_t * 1e3), flush=True)
    return best
