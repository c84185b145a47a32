"""Mints tests/golden/fgm_mask.npz by running the REFERENCE'S OWN `create_heatmap_gt(..., resolution)` (magicdrive/networks/
utils.py, with its own scipy `ConvexHull` and matplotlib `Polygon.contains_point`) and `hd_crop` (the function nested in
`collate_fn`, dataset/utils.py:348-353, taken out of `collate_fn`'s own code object) on seeded scenes, a hand-made set and
a cropped case, so that tests/fgm_reference.py stays pinned to the reference where the reference, scipy and matplotlib are
not installed.  Inputs and outputs are recorded, and the truncated integer points the reference hands to `ConvexHull` (a
recording wrapper around the name in the reference module's namespace); no reference text is copied.  It also times the
reference's lines on this machine's CPU at 6 views x 40 boxes (printed; profiles/fgm_mask.txt quotes them).

Runs only where the reference tree is (REF of tests/golden/mint_box_input.py); no test imports this module.  What the
reference's files import and this machine lacks is a name-only stand-in IN MEMORY (those of mint_box_input.py), and
`np.int = int` is set in memory: the reference's line uses the alias current numpy no longer has.

The hand-made set goes through the projection with exactly representable numbers: grid (16, 9), so that the scale factors
are 16 / 1600 and 9 / 900, both the double next above 0.01; matrix A maps a corner (X, Y, Z) to x = 100 X, y = 100 Y, z = Z,
so that a corner (p Z, q Z, Z) with Z a power of two lands on pixel (p, q) exactly (100 p * fl(0.01) >= p, truncated: p);
matrix B is the identity, for corners given in hundredths of a pixel (X = -70: -0.7, truncated toward zero to 0).

Usage:  python -m tests.golden.mint_fgm_mask
"""
import contextlib
import io
import os
import time
import types

import numpy as np
import torch

from tests import fgm_reference as R
from tests.golden import mint_box_input as MB

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "fgm_mask.npz")
SEED = 20277
GRID = (12, 9)
COUNTS = ((0, 5), (70, 33))
HAND_GRID = (16, 9)
CROP_GRID, CROP = (96, 54), (32, 88)
MAT_A = np.array([[100, 0, 0, 0], [0, 100, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float32)
MAT_B = np.eye(4, dtype=np.float32)
OFF = (0, 0, 0)                                            # a corner with z = 0: dropped


def on(p, q, z=1):
    return (p * z, q * z, z)


def box(*pts):
    """up to 8 corners, filled up with dropped ones"""
    pts = list(pts) + [OFF] * (8 - len(pts))
    assert len(pts) == 8
    return pts


TRIANGLE = [on(2, 1), on(10, 1), on(2, 7)]
# name, matrix, boxes of the view (each 8 corners), index of the box that is past the bound (or None)
HAND = [
    ("triangle", MAT_A, [box(*TRIANGLE)], None),
    ("triangle_reversed", MAT_A, [box(*TRIANGLE[::-1])], None),
    ("triangle_between_dropped", MAT_A, [[OFF, on(2, 1), (5, 5, -1), on(10, 1, 2), OFF, on(2, 7, 4), OFF, OFF]], None),
    ("collinear_on_hull_edge", MAT_A, [[on(1, 1), on(4, 1), on(7, 1), on(7, 5), on(1, 5), on(4, 5), on(3, 3), on(1, 3)]], None),
    ("line_horizontal", MAT_A, [box(on(1, 2), on(5, 2), on(9, 2), on(13, 2))], None),
    ("line_vertical", MAT_A, [box(on(4, 1), on(4, 3), on(4, 7))], None),
    ("line_diagonal", MAT_A, [box(on(1, 1), on(3, 3), on(5, 5), on(7, 7))], None),
    ("line_antidiagonal", MAT_A, [box(on(9, 1), on(7, 3), on(5, 5), on(3, 7))], None),
    ("line_not_monotone", MAT_A, [box(on(1, 1), on(7, 7), on(3, 3), on(5, 5))], None),
    ("line_not_monotone_flat", MAT_A, [box(on(9, 4), on(2, 4), on(12, 4), on(5, 4), on(2, 4))], None),
    ("one_point", MAT_A, [box(on(5, 4))], None),
    ("two_points", MAT_A, [box(on(3, 2), on(9, 6))], None),
    ("two_points_flat", MAT_A, [box(on(3, 4), on(9, 4))], None),
    ("all_behind", MAT_A, [[(p, q, z) for p, q, z in ((1, 1, 0), (5, 1, -1), (5, 5, 0), (1, 5, -2), (2, 2, 0), (3, 3, -1),
                                                      (4, 4, 0), (6, 6, -4))]], None),
    ("duplicates", MAT_A, [[on(3, 3), on(3, 3), on(8, 3), on(5, 7), on(8, 3), on(3, 3), on(5, 7), on(5, 7)]], None),
    ("all_the_same", MAT_A, [[on(6, 4)] * 8], None),
    ("whole_grid", MAT_A, [[on(-1, -1), on(16, -1), on(16, 9), on(-1, 9), on(0, 0), on(15, 8), on(3, 3), on(8, 4)]], None),
    ("grid_corners", MAT_A, [box(on(0, 0), on(15, 0), on(15, 8), on(0, 8))], None),
    ("negative_truncation", MAT_B, [box((-70, -70, 1), (650, -30, 1), (690, 410, 1), (-99, 399, 1)),
                                    box((-170, 250, 1), (420, -130, 1), (1234, 777, 1))], None),
    ("partly_off_grid", MAT_A, [[on(-5, -3), on(6, -4), on(20, 4), on(7, 12), on(-2, 6), on(3, 3), on(4, 1), on(1, 4)]], None),
    ("overlap_max", MAT_A, [box(on(1, 1), on(12, 1), on(12, 8), on(1, 8)), box(on(4, 2), on(8, 2), on(8, 5), on(4, 5))], None),
    ("past_the_bound", MAT_A, [box(on(2, 2), on(1 << 26, 2), on(2, 6)), box(on(9, 1), on(13, 1), on(11, 6))], 0),
]


def recorder(utils):
    """wraps the names `ConvexHull` and `process_one_instance_test` of the reference module: the integer points of every
    masked box as the reference's own `@` and truncation give them, and what the box paints"""
    log = {"pts": [], "peak": [], "count": []}
    hull, inst = utils.ConvexHull, utils.process_one_instance_test

    def convex_hull(coords):
        log["pts"].append(np.array(coords, np.int64).reshape(-1, 2))
        return hull(coords)

    def one_instance(corners, is_foreground, *a):
        before = len(log["pts"])
        out = inst(corners, is_foreground, *a)
        if not is_foreground:
            log["pts"].append(None)
        assert len(log["pts"]) == before + 1
        log["peak"].append(float(out.max()))
        log["count"].append(int((out != 0).sum()))
        return out

    utils.ConvexHull, utils.process_one_instance_test = convex_hull, one_instance
    return log


def run(utils, log, bboxes, masks, l2i, grid):
    """-> the reference's map (b, n, H, W) and, per box, the integer points (padded), their number (-1: mask false), the
    painted value and the number of non-zero pixels"""
    for v in log.values():
        del v[:]
    b, n, m = masks.shape
    metas = [MB.Held({"token": "scene%d" % i}) for i in range(b)]
    with contextlib.redirect_stdout(io.StringIO()):        # the reference prints a line per box with no point left
        heat = utils.create_heatmap_gt({"bboxes": torch.from_numpy(bboxes), "masks": torch.from_numpy(masks)},
                                       torch.from_numpy(l2i), metas, resolution=grid)
    assert heat.dtype == torch.float32 and tuple(heat.shape) == (b, n, grid[1], grid[0])
    assert len(log["pts"]) == b * n * m
    pts, cnt = np.zeros((b * n * m, 8, 2), np.int64), np.full((b * n * m,), -1, np.int64)
    for i, p in enumerate(log["pts"]):
        if p is not None:
            cnt[i] = len(p)
            pts[i, :len(p)] = p
    return (heat.numpy(), pts.reshape(b, n, m, 8, 2), cnt.reshape(b, n, m),
            np.array(log["peak"], np.float32).reshape(b, n, m), np.array(log["count"], np.int64).reshape(b, n, m))


def store(out, name, bboxes, masks, l2i, res):
    heat, pts, cnt, peak, count = res
    out.update({name + "_bboxes": bboxes, name + "_masks": masks, name + "_l2i": l2i, name + "_heat": heat,
                name + "_pts": pts.astype(np.int32), name + "_npts": cnt.astype(np.int8), name + "_peak": peak,
                name + "_count": count.astype(np.int32)})


def main():
    import matplotlib.patches  # noqa: F401  (the reference says `matplotlib.patches.Polygon` after `import matplotlib`)
    MB.install_stubs()
    np.int = int
    from magicdrive.dataset.utils import collate_fn
    from magicdrive.networks import utils
    code = next(c for c in collate_fn.__code__.co_consts if isinstance(c, types.CodeType) and c.co_name == "hd_crop")
    assert not code.co_freevars
    hd_crop = types.FunctionType(code, collate_fn.__globals__, "hd_crop")
    log = recorder(utils)
    out = {"grid": np.array(GRID), "hand_grid": np.array(HAND_GRID), "crop_grid": np.array(CROP_GRID), "crop": np.array(CROP)}

    # seeded scenes
    cap = 72
    bboxes, masks, l2i = R.scenes(SEED, COUNTS, cap)
    assert R.heatmap(bboxes, masks, l2i, GRID)["flagged"] == 0
    store(out, "seeded", bboxes, masks, l2i, run(utils, log, bboxes, masks, l2i, GRID))

    # the hand-made set: one view per case
    n, m = len(HAND), max(len(h[2]) for h in HAND)
    bboxes, masks, l2i = np.zeros((1, n, m, 8, 3), np.float32), np.zeros((1, n, m), bool), np.zeros((1, n, 4, 4), np.float32)
    run_masks = masks.copy()
    for j, (_, mat, bxs, past) in enumerate(HAND):
        l2i[0, j] = mat
        for k, bx in enumerate(bxs):
            bboxes[0, j, k] = np.array(bx, np.float32)
            masks[0, j, k] = True
            run_masks[0, j, k] = k != past                 # the box past the bound is not run through the reference
    assert bboxes.max() == float(1 << 26)
    store(out, "hand", bboxes, masks, l2i, run(utils, log, bboxes, run_masks, l2i, HAND_GRID))
    out["hand_names"] = np.array([h[0] for h in HAND])
    out["hand_flagged"] = np.array(int((masks & ~run_masks).sum()))
    assert int(out["hand_flagged"]) == 1 and R.heatmap(bboxes, masks, l2i, HAND_GRID)["flagged"] == 1

    # (96, 54) cropped to (32, 88)
    bboxes, masks, l2i = R.scenes(SEED + 1000, ((5, 5),), 6, visible=CROP_GRID)
    assert R.heatmap(bboxes, masks, l2i, CROP_GRID)["flagged"] == 0
    res = run(utils, log, bboxes, masks, l2i, CROP_GRID)
    store(out, "crop", bboxes, masks, l2i, res)
    out["crop_heat_full"] = res[0]
    out["crop_heat"] = np.ascontiguousarray(hd_crop(torch.from_numpy(res[0]), (CROP_GRID[1], CROP_GRID[0]), CROP).numpy())
    assert out["crop_heat"].shape[-2:] == CROP

    np.savez_compressed(PATH, **out)
    print("wrote %s (%d arrays, %d bytes)" % (PATH, len(out), os.path.getsize(PATH)))

    # the reference's lines on this CPU: 6 views x 40 boxes
    bboxes, masks, l2i = R.scenes(SEED + 2000, ((40,) * 6,), 40, visible=(50, 28))
    for grid in ((50, 28), (96, 54)):
        t0 = time.perf_counter()
        run(utils, log, bboxes, masks, l2i, grid)
        t1 = time.perf_counter()
        R.heatmap(bboxes, masks, l2i, grid)
        t2 = time.perf_counter()
        print("create_heatmap_gt, 6 views x 40 boxes at %s: %.2f s (the numpy restatement: %.3f s)" % (grid, t1 - t0, t2 - t1))


if __name__ == "__main__":
    main()
