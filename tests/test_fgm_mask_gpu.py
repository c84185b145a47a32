"""FGM loss mask and loss on the GPU (`FgmMask`, `fgm_loss`; `ops.fgm_mask`: dd_fgm_box_records + dd_fgm_mask, `ops.fgm_loss`:
dd_fgm_loss) against the fixture minted from the reference's own `create_heatmap_gt` / `hd_crop` and the numpy restatement
tests/fgm_reference.py, which tests/test_fgm_mask_cpu.py pins to the reference and to scipy / matplotlib.  No scipy, no
matplotlib, no reference tree here.  The mask comparisons are `torch.equal`.

The loss bounds (nothing fitted to a measurement, u = 2^-24):
  * value: every term (p - t)^2 (1 + heat) is non-negative, so the error of the fp32 sum is RELATIVE to the sum:
    |v - ref| <= gamma_k ref with k = tests.fgm_reference.loss_roundings(N) fp32 roundings on the longest path through
    the fixed reduction tree (include/dualdiff_hip.h) and gamma_k = k u / (1 - k u); fp16 / bf16 inputs convert to fp32
    exactly, and the reference takes the same rounded inputs in float64.
  * gradient, per element: (p - t), (1 + heat), float32(2 / N), their two products: five roundings, |g - ref| <= 6 u |ref| for
    the fp32 value, plus one unit of the output type at |ref| for the cast (tests/gemm_reference.ulp, subnormal spacing
    included: at N = 33600 the fp16 gradients are subnormal).
"""
import collections

import numpy as np
import pytest
import torch

from dualdiff_amd import ops
from dualdiff_amd.pipeline import FgmMask
from dualdiff_amd.pipeline.fgm_mask import fgm_loss
from tests import fgm_reference as R
from tests.gemm_reference import ulp

pytestmark = pytest.mark.gpu

GOLD = __file__.replace("test_fgm_mask_gpu.py", "golden/fgm_mask.npz")
SETS = {"seeded": ("grid", None), "hand": ("hand_grid", None), "crop": ("crop_grid", "crop")}
U = 2.0 ** -24
Views = collections.namedtuple("Views", "bboxes classes masks counts max_len_dev")      # BoxViews' fields


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def case(gold, name, dev):
    grid_key, crop_key = SETS[name]
    grid = tuple(int(v) for v in gold[grid_key])
    crop = None if crop_key is None else tuple(int(v) for v in gold[crop_key])
    want = gold["crop_heat"] if name == "crop" else gold[name + "_heat"]
    arrays = tuple(torch.from_numpy(gold[name + k]).to(dev) for k in ("_bboxes", "_masks", "_l2i"))
    return arrays, grid, crop, torch.from_numpy(want).to(dev)


@pytest.mark.parametrize("name", list(SETS))
def test_mask_equals_the_reference(gpu, gold, name):
    """every element of every fixture view — the hand-made families one view each, the 70-box view (more boxes than a wave
    has lanes), the cropped case — and the flagged count; two calls give the same bits"""
    (bboxes, masks, l2i), grid, crop, want = case(gold, name, gpu)
    fm = FgmMask(grid, crop=crop)
    heat = fm(bboxes, masks, l2i)
    assert heat.dtype == torch.float32 and heat.shape == want.shape
    bad = (heat != want).nonzero()
    assert torch.equal(heat, want), "first differing elements (scene, view, y, x): %s" % bad[:8].tolist()
    flagged = int(gold["hand_flagged"]) if name == "hand" else 0
    assert fm.flags.dtype == torch.int32 and int(fm.flags.item()) == flagged
    again = fm(bboxes, masks, l2i)
    assert torch.equal(again, heat) and int(fm.flags.item()) == flagged
    if flagged:
        with pytest.raises(ValueError, match="%d box" % flagged):
            fm(bboxes, masks, l2i, check=True)
    else:
        assert torch.equal(fm(bboxes, masks, l2i, check=True), heat)


@pytest.mark.parametrize("name", list(SETS))
def test_box_records_equal_the_restatement(gpu, gold, name):
    """what the map cannot show (a box of weight 0, a box under a heavier one): every box's area, weight, flag, vertex count
    and ring, read out of the workspace"""
    (bboxes, masks, l2i), grid, crop, _ = case(gold, name, gpu)
    b, n, m = masks.shape
    ws = torch.full((ops.fgm_workspace_bytes(b * n * m) + 64,), 0xAB, dtype=torch.uint8, device=gpu)
    ops.fgm_mask(bboxes, masks, l2i, grid, crop, workspace=ws)
    rec = ws[:b * n * m * 4 * ops.FGM_REC_WORDS].view(torch.int32).reshape(b, n, m, ops.FGM_REC_WORDS).cpu().numpy()
    assert bool((ws[-64:] == 0xAB).all())
    res = R.heatmap(gold[name + "_bboxes"], gold[name + "_masks"], gold[name + "_l2i"], grid)
    assert np.array_equal(rec[..., ops.FGM_REC_FLAGGED], res["unsupported"].astype(np.int32))
    assert np.array_equal(rec[..., ops.FGM_REC_AREA], res["area"])
    live = gold[name + "_masks"] & ~res["unsupported"]
    assert np.array_equal(rec[..., ops.FGM_REC_WEIGHT].view(np.float32)[live], res["weight"][live])
    for (i, j, k), ring in res["rings"].items():
        assert rec[i, j, k, ops.FGM_REC_NV] == len(ring)
        got = rec[i, j, k, :2 * len(ring)].reshape(-1, 2).tolist()
        if len(R.hull(ring)) >= 3:                         # a hull: the same cycle, whatever vertex it starts from
            s = got.index(list(ring[0]))
            got = got[s:] + got[:s]
        assert got == [list(p) for p in ring], (i, j, k)
    assert (rec[..., ops.FGM_REC_NV][~live] == 0).all()


def test_both_layouts_and_no_boxes(gpu, gold):
    """the synced dict (rows up to the batch maximum) and the BoxViews capacity layout (more rows, mask False, whatever their
    contents) give the same map; None gives zeros"""
    (bboxes, masks, l2i), grid, _, want = case(gold, "seeded", gpu)
    fm = FgmMask(grid)
    longest = int(masks.sum(-1).max())
    assert longest == 70 < masks.shape[2]
    synced = {"bboxes": bboxes[:, :, :longest].contiguous(), "masks": masks[:, :, :longest].contiguous()}
    assert torch.equal(fm(synced["bboxes"], synced["masks"], l2i), want)
    assert torch.equal(fm(synced, None, l2i), want)
    cap = 96
    big = torch.full(bboxes.shape[:2] + (cap, 8, 3), float("nan"), device=gpu)
    big[:, :, :bboxes.shape[2]] = bboxes
    big_masks = torch.zeros(masks.shape[:2] + (cap,), dtype=torch.bool, device=gpu)
    big_masks[:, :, :masks.shape[2]] = masks
    views = Views(big, None, big_masks, masks.sum(-1).int(), None)
    assert torch.equal(fm(views, lidar2image=l2i, check=True), want) and int(fm.flags.item()) == 0
    none = fm(None, None, l2i, check=True)
    assert none.shape == want.shape and not none.any() and int(fm.flags.item()) == 0
    empty = fm(bboxes[:, :, :0].contiguous(), masks[:, :, :0].contiguous(), l2i, check=True)
    assert torch.equal(empty, none)


def test_not_finite_corners_are_flagged(gpu, gold):
    (bboxes, masks, l2i), grid, _, want = case(gold, "seeded", gpu)
    bboxes = bboxes.clone()
    view = (1, 1)
    idx = 3
    assert bool(masks[view + (idx,)])
    bboxes[view + (idx, 5, 1)] = float("inf")
    fm = FgmMask(grid)
    heat = fm(bboxes, masks, l2i)
    assert int(fm.flags.item()) == 1
    host_masks = gold["seeded_masks"].copy()
    host_masks[view + (idx,)] = False                      # not painted: as if the box were not there
    ref = R.heatmap(gold["seeded_bboxes"], host_masks, gold["seeded_l2i"], grid)["heat"]
    assert torch.equal(heat.cpu(), torch.from_numpy(ref))


def test_from_box_preprocess(gpu):
    """`for_mask` as BoxPreProcess(use_3d_filter=False) makes it, in both of its layouts, at the (50, 28) grid of 224 x 400"""
    from dualdiff_amd.pipeline.box_input import BoxPreProcess, compose_transforms
    from tests import box_input_reference as RB
    data = RB.batch(RB.GOLDEN_SEED, (0, 5, 70))
    pre = BoxPreProcess("all-xyz", view_shared=False, use_3d_filter=False, canvas_size=RB.CANVAS)
    trans = compose_transforms(data["lidar2image"], data["img_aug_matrix"])
    synced = pre(data["filter_corners"], data["labels"], trans)
    views = pre(data["filter_corners"], data["labels"], trans, sync=False)
    l2i = torch.from_numpy(data["lidar2image"]).to(gpu)
    fm = FgmMask.from_config({"dataset": {"image_size": list(RB.CANVAS)}})
    heat = fm(synced["bboxes"], synced["masks"], l2i, check=True)
    assert heat.shape == (3, 6, 28, 50) and torch.equal(fm(views, lidar2image=l2i), heat)
    ref = R.heatmap(synced["bboxes"].cpu().numpy(), synced["masks"].cpu().numpy(), data["lidar2image"], (50, 28))
    assert ref["flagged"] == 0 and (ref["heat"] != 0).any()
    assert torch.equal(heat.cpu(), torch.from_numpy(ref["heat"]))


# ---- the loss -----------------------------------------------------------------------------------------------------------

SHAPES = ((2, 2, 4, 9, 12), (1, 6, 4, 28, 50))
DTYPES = (torch.float16, torch.bfloat16, torch.float32)


def loss_inputs(shape, dtype, dev):
    g = torch.Generator().manual_seed(sum(shape))
    pred = torch.randn(shape, generator=g).to(dtype)
    target = (torch.randn(shape, generator=g) * 0.7 + 0.1).to(dtype)
    heat = torch.rand(shape[:2] + shape[3:], generator=g)
    heat = torch.where(heat < 0.6, torch.zeros_like(heat), heat)         # most of a map is background
    ref = R.loss(pred.double().numpy(), target.double().numpy(), heat.numpy())
    plain = R.loss(pred.double().numpy(), target.double().numpy(), None)
    return pred.to(dev), target.to(dev), heat.to(dev), ref, plain


def value_bound(count):
    k = R.loss_roundings(count)
    return k * U / (1.0 - k * U)


def check_grad(grad, ref, dtype, what):
    ref = torch.from_numpy(ref)
    bound = 6 * U * ref.abs() + ulp(ref, dtype)
    err = (grad.double().cpu() - ref).abs()
    worst = float((err / bound).max())
    print("%s: gradient error at most %.3f of the bound" % (what, worst))
    assert grad.dtype == dtype and bool((err <= bound).all()), (what, worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_loss_value_and_gradient(gpu, shape, dtype):
    pred, target, heat, (ref, ref_grad), (plain, plain_grad) = loss_inputs(shape, dtype, gpu)
    count = pred.numel()
    loss, grad = ops.fgm_loss(pred, target, heat, want_grad=True)
    assert loss.dtype == torch.float32 and loss.shape == ()
    rel = abs(float(loss) - ref) / ref
    print("%s %s: loss %.9g, reference %.9g, relative error %.3g, bound %.3g" % (shape, dtype, float(loss), ref, rel,
                                                                                value_bound(count)))
    assert rel <= value_bound(count)
    check_grad(grad, ref_grad, dtype, "%s %s" % (shape, dtype))
    # the value does not depend on whether the gradient is asked for; two calls give the same bits
    only, none = ops.fgm_loss(pred, target, heat)
    assert none is None and torch.equal(only, loss)
    loss2, grad2 = ops.fgm_loss(pred, target, heat, want_grad=True)
    assert torch.equal(loss2, loss) and torch.equal(grad2, grad)
    # heat=None: the plain mean
    mean, mean_grad = ops.fgm_loss(pred, target, None, want_grad=True)
    assert abs(float(mean) - plain) / plain <= value_bound(count)
    check_grad(mean_grad, plain_grad, dtype, "%s %s plain" % (shape, dtype))
    assert torch.equal(fgm_loss(pred, target), mean)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_backward_is_the_fused_gradient(gpu, dtype):
    pred, target, heat, _, _ = loss_inputs(SHAPES[0], dtype, gpu)
    want_loss, want_grad = ops.fgm_loss(pred, target, heat, want_grad=True)
    p = pred.clone().requires_grad_(True)
    loss = fgm_loss(p, target, heat)
    assert loss.requires_grad and torch.equal(loss.detach(), want_loss)
    loss.backward()
    assert p.grad.dtype == dtype and torch.equal(p.grad, want_grad)
    with torch.no_grad():
        assert torch.equal(fgm_loss(pred, target, heat), want_loss)
    # a non-contiguous pred goes through a copy, not through a wrong stride
    q = pred.transpose(3, 4).contiguous().transpose(3, 4)
    assert not q.is_contiguous() and torch.equal(fgm_loss(q, target, heat), want_loss)
