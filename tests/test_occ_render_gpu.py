"""ORS panorama on the GPU (`dd_ors_first_hit`, `dd_ors_overlay_u8`) against the fixture minted from the reference's own
lines (tests/golden/occ_render.npz) and the CPU restatement (tests/occ_render_reference.py).  Integer work: every class
and every byte must be EQUAL.  Each reference is computed once per module."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import occ_render_reference as R
from tests.golden import cases as C

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "occ_render.npz")
K_EDGE = torch.tensor([[1260.0, 0.0, 800.0], [0.0, 1260.0, 450.0], [0.0, 0.0, 1.0]])
# (h, w, samples, step, cameras): no ray count per camera is a multiple of 64, and 130 and 65 samples are none either
GEOMETRIES = [(14, 25, 320, 0.2, 3), (9, 13, 130, 0.5, 4), (5, 7, 65, 1.0, 5), (56, 100, 320, 0.2, 2)]
# seeds picked with the oracle alone: cameras inside and outside the volume, and for the first case a first hit beyond 200
SEEDS = [4203, 4202, 4207, 4221]


def projector(h, w, samples, step):
    from dualdiff_amd.networks.occ3d_proj import OccupancyRay
    ratio = w / 1600
    proj = OccupancyRay(image_shape=(h / ratio + 0.5, 1600), sample_point=samples, sample_step=step, compress_ratio=ratio,
                        device="cuda")
    assert proj.image_shape_compress == [h, w]
    return proj


@functools.lru_cache(maxsize=None)
def gold():
    return dict(np.load(GOLD))


@functools.lru_cache(maxsize=None)
def fixture_labels():
    from oracle import ors_projection as P
    occ, Ks, Rts = C.ors_inputs()
    return P.ors_project(occ, Ks, Rts, C.ORS_H, C.ORS_W, C.ORS_RATIO, C.ORS_S, 0.2)


@functools.lru_cache(maxsize=None)
def random_case(k):
    """volume and rig as test_ors_projection_random_rigs makes them, and the oracle's labels for GEOMETRIES[k]"""
    from oracle import ors_projection as P
    h, w, s, step, n = GEOMETRIES[k]
    g = torch.Generator().manual_seed(SEEDS[k])
    occ = torch.randint(0, 18, (200, 200, 16), generator=g)
    Ks, Rts = R.random_rig(g, n)
    return occ, Ks, Rts, P.ors_project(occ, Ks, Rts, h, w, w / 1600, s, step)


def restate(labels, mode):
    cls, idx = R.first_hit(labels, mode)
    return cls.numpy().astype(np.uint8), R.paint(cls), idx.numpy()


def same(t, arr):
    got = t.cpu().numpy()
    return got.shape == arr.shape and np.array_equal(got, arr)


@torch.no_grad()
@pytest.mark.parametrize("mode", R.MODES)
def test_fixture_geometry_equals_the_reference_lines(mode):
    from dualdiff_amd.networks.occ3d_proj import OccupancyRay
    occ, Ks, Rts = C.ors_inputs()
    proj = OccupancyRay(image_shape=(896, 1600), sample_point=C.ORS_S, sample_step=0.2, compress_ratio=C.ORS_RATIO,
                        device="cuda")
    want_cls, want_pan = gold()["classes_" + mode], gold()["frames_" + mode]
    cls_r, pan_r, _ = restate(fixture_labels(), mode)
    assert np.array_equal(cls_r, want_cls) and np.array_equal(pan_r, want_pan)
    frames, cls = proj.render_volume(occ, Ks, Rts, mode=mode, want_classes=True)          # both outputs in one call
    assert frames.dtype == torch.uint8 and cls.dtype == torch.uint8
    assert same(cls, want_cls), "%d classes differ" % (cls.cpu().numpy() != want_cls).sum()
    assert same(frames, want_pan)
    assert same(proj.render_volume(occ, Ks, Rts, mode=mode), want_pan)                    # frames alone
    only = proj.render_batch([occ], [(Ks, Rts)], mode=mode, want_frames=False, want_classes=True)
    assert only[0] is None and same(only[1][0], want_cls)                                 # classes alone


@torch.no_grad()
@pytest.mark.parametrize("k", range(len(GEOMETRIES)), ids=["%dx%dx%d" % g[:3] for g in GEOMETRIES])
def test_other_geometries_equal_the_restatement(k):
    h, w, s, step, n = GEOMETRIES[k]
    assert (h * w) % 64                                       # 130 and 65 samples also end inside a group of four
    occ, Ks, Rts, labels = random_case(k)
    proj = projector(h, w, s, step)
    for mode in R.MODES:
        want_cls, want_pan, _ = restate(labels, mode)
        assert (want_cls != 17).any() and (want_cls == 17).any()
        frames, cls = proj.render_volume(occ, Ks, Rts, mode=mode, want_classes=True)
        assert same(cls, want_cls), (mode, int((cls.cpu().numpy() != want_cls).sum()))
        assert same(frames, want_pan), mode


@torch.no_grad()
def test_early_exits_change_no_byte_and_visit_less():
    """exits: bit 0 stop at the hit, bit 1 stop once out of the volume for good; every combination gives the same panorama,
    and the counts of samples looked up are ordered as the rules promise"""
    h, w, s, step, n = GEOMETRIES[0]
    occ, Ks, Rts, labels = random_case(0)
    proj = projector(h, w, s, step)
    want_cls, want_pan, _ = restate(labels, "bg")
    seen = {}
    for exits in (0, 1, 2, 3):
        frames, cls, visited = proj.render_batch([occ], [(Ks, Rts)], mode="bg", want_classes=True, want_visited=True,
                                                 exits=exits)
        assert same(cls[0], want_cls) and same(frames[0], want_pan), exits
        seen[exits] = visited.cpu().numpy().astype(np.int64)
    assert (seen[0] == s).all()
    assert (seen[3] <= seen[1]).all() and (seen[3] <= seen[2]).all() and seen[3].sum() < min(seen[1].sum(), seen[2].sum())


@torch.no_grad()
def test_loop_bounds_at_the_deepest_hit():
    h, w, s, step, n = GEOMETRIES[0]
    occ, Ks, Rts, labels = random_case(0)
    want_cls, _, idx = restate(labels, "all")
    deepest = int(idx[want_cls != 17].max())
    at = (idx == deepest) & (want_cls != 17)
    assert 64 < deepest < s - 1 and at.any()
    hit = projector(h, w, deepest + 1, step).render_volume(occ, Ks, Rts, mode="all", want_classes=True)[1].cpu().numpy()
    miss = projector(h, w, deepest, step).render_volume(occ, Ks, Rts, mode="all", want_classes=True)[1].cpu().numpy()
    assert np.array_equal(hit, want_cls)                      # nothing lies deeper: samples = D + 1 sees every hit
    assert (miss[at] == 17).all() and np.array_equal(miss[~at], want_cls[~at])
    assert np.array_equal(miss, restate(labels[..., :deepest], "all")[0])


@torch.no_grad()
@pytest.mark.parametrize("t", [(-60.0, 3.0, 1.5), (-45.0, -7.0, 4.0), (0.0, 0.0, 8.0)], ids=["behind", "corner", "above"])
def test_leaving_rule_does_not_fire_before_entry(t):
    """a camera outside the fixture volume looking in: its rays are out of range on the near side for many samples"""
    from oracle import ors_projection as P
    occ = C.ors_inputs()[0]
    Rt = R.looking_in(t)
    labels = P.ors_project(occ, [K_EDGE], [Rt], C.ORS_H, C.ORS_W, C.ORS_RATIO, C.ORS_S, 0.2)
    assert (labels[..., 0] == 17).all()                       # every ray starts outside
    proj = projector(C.ORS_H, C.ORS_W, C.ORS_S, 0.2)
    for mode in R.MODES[:2]:
        want_cls, want_pan, idx = restate(labels, mode)
        share = float((want_cls != 17).mean())
        print(t, mode, "hit share %.3f, first hit at %d" % (share, int(idx[want_cls != 17].min())))
        assert share > 0.1
        frames, cls = proj.render_volume(occ, [K_EDGE], [Rt], mode=mode, want_classes=True)
        assert same(cls, want_cls) and same(frames, want_pan)


@torch.no_grad()
def test_edge_volumes():
    proj = projector(16, 9, 64, 0.5)
    inside = R.looking_in((0.0, 0.0, 1.0))
    empty = torch.full((200, 200, 16), 17)
    for mode in R.MODES:
        frames, cls = proj.render_volume(empty, [K_EDGE], [inside], mode=mode, want_classes=True)
        assert (cls == 17).all() and (frames == 0).all()
    full = torch.full((200, 200, 16), 5)
    frames, cls, visited = proj.render_batch([full], [([K_EDGE], [inside])], mode="all", want_classes=True,
                                             want_visited=True)
    assert (cls == 5).all() and (frames.view(-1, 3).cpu() == torch.tensor(R.PALETTE[5])).all()
    assert (visited == 4).all()                               # the hit is sample 0: one group of four samples
    assert (proj.render_volume(full, [K_EDGE], [inside], mode="bg", want_classes=True)[1] == 17).all()
    # a class-0 voxel in front of a class-4 wall, the camera at the centre of the volume looking along +x
    two = torch.full((200, 200, 16), 17)
    two[110:113] = 0                                          # three voxels thick: a 0.5 m step cannot jump it
    two[120:123] = 4
    got = {m: proj.render_volume(two, [K_EDGE], [inside], mode=m, want_classes=True) for m in R.MODES}
    mid = (0, 2, 4)                                           # the principal point: 450 * 9 / 1600, 800 * 9 / 1600
    assert got["all"][1][mid] == 0 and (got["all"][0][2, 4] == 0).all()
    assert got["bg"][1][mid] == 17 and got["fg"][1][mid] == 0
    from oracle import ors_projection as P
    labels = P.ors_project(two, [K_EDGE], [inside], 16, 9, 9 / 1600, 64, 0.5)
    for m in R.MODES:
        assert same(got[m][1], restate(labels, m)[0]) and same(got[m][0], restate(labels, m)[1])


@torch.no_grad()
def test_batch_is_one_launch_over_shared_rigs():
    h, w, s, step, n = GEOMETRIES[1]
    occ, Ks, Rts, _ = random_case(1)
    g = torch.Generator().manual_seed(77)
    occ2 = torch.randint(0, 18, (200, 200, 16), generator=g)
    Ks2, Rts2 = R.random_rig(g, n)
    proj = projector(h, w, s, step)
    vols, rigs = [occ, occ2, occ2], [(Ks, Rts), (Ks2, Rts2), (Ks, Rts)]
    frames, cls = proj.render_batch(vols, rigs, mode="bg", want_classes=True)
    assert frames.shape == (3, h, n * w, 3) and cls.shape == (3, n, h, w)
    assert len(proj._ray_cache) == 2                          # rig_of_sample = [0, 1, 0]: two tables for three samples
    for i in range(3):
        one_f, one_c = proj.render_volume(vols[i], *rigs[i], mode="bg", want_classes=True)
        assert torch.equal(frames[i], one_f) and torch.equal(cls[i], one_c), i
    assert not torch.equal(cls[1], cls[2])
    from dualdiff_amd import ops as O
    origin, direction = proj.rays(Ks, Rts)
    with pytest.raises(ValueError, match=r"rig_of_sample must lie in \[0, 1\)"):
        O.ors_first_hit(proj._volumes([occ]), origin[None], direction[None], [1], (h, w), s, step, palette=R.PALETTE)


@torch.no_grad()
def test_overlay_equals_the_reference_lines():
    from dualdiff_amd.pipeline.occ_render import OccRender
    render = OccRender((896, 1600), C.ORS_RATIO)
    cam = R.camera_panorama(R.camera_pictures())
    pans = np.stack([gold()["frames_" + m] for m in R.MODES])
    cams = np.stack([cam, 255 - cam, cam // 2 + 17])           # three samples, three ranges: min and max are per sample
    out = render.overlay(torch.from_numpy(pans).cuda(), torch.from_numpy(cams).cuda()).cpu().numpy()
    assert np.array_equal(out[0], gold()["overlay_all"])
    for i in range(3):
        assert np.array_equal(out[i], R.overlay(pans[i], cams[i])), i
    one = render.overlay(torch.from_numpy(pans[1:2]).cuda(), torch.from_numpy(cam[None]).cuda()).cpu().numpy()
    assert np.array_equal(one[0], gold()["overlay_bg"])
    fg = render.overlay(torch.from_numpy(pans[2:3]).cuda(), torch.from_numpy(cam[None]).cuda()).cpu().numpy()
    assert np.array_equal(fg[0], gold()["overlay_fg"])


@torch.no_grad()
def test_overlay_sizes_off_the_vector_width():
    """h * W * 3 = 315 and 1083 are no multiple of 4 (bytewise path); 2 x 1083 bytes put the second sample off alignment"""
    from dualdiff_amd import ops as O
    g = torch.Generator().manual_seed(5)
    for b, h, w in ((1, 5, 21), (2, 19, 19), (2, 20, 57)):
        colour = torch.randint(0, 256, (b, h, w, 3), generator=g, dtype=torch.uint8)
        colour[torch.rand((b, h, w, 3), generator=g) < 0.4] = 0
        cam = torch.randint(3, 250, (b, h, w, 3), generator=g, dtype=torch.uint8)
        out, flags = O.ors_overlay(colour.cuda(), cam.cuda())
        assert int(flags.item()) == 0
        for i in range(b):
            assert np.array_equal(out[i].cpu().numpy(), R.overlay(colour[i].numpy(), cam[i].numpy())), (b, h, w, i)


@torch.no_grad()
def test_overlay_reports_a_constant_camera_picture():
    from dualdiff_amd.pipeline.occ_render import OccRender
    render = OccRender((896, 1600), C.ORS_RATIO)
    pan = torch.from_numpy(gold()["frames_bg"][None]).cuda()
    flat = torch.full_like(pan, 90)
    with pytest.raises(ValueError, match="constant"):
        render.overlay(pan, flat)
    assert render.overlay(pan, flat, check=False).shape == pan.shape
    with pytest.raises(ValueError, match="shape"):
        render.overlay(pan, flat[:, :, :-6])


@torch.no_grad()
def test_panorama_feeds_the_condition_and_the_png_writer(tmp_path):
    from dualdiff_amd.pipeline.image_output import save_png
    from dualdiff_amd.pipeline.occ_render import OccRender
    from dualdiff_amd.pipeline.png_input import OccCondition, occ_condition_from_config
    cfg = {"dataset": {"image_size": [224, 400]}}
    occ, Ks, Rts = C.ors_inputs()
    render = OccRender.for_image_size([224, 400], compress_ratio=C.ORS_RATIO)
    frames = render([occ, occ], (Ks, Rts))
    assert frames.shape == (2, C.ORS_H, 6 * C.ORS_W, 3) and same(frames[0], gold()["frames_bg"])
    assert same(render.classes([occ], [(Ks, Rts)])[0], gold()["classes_bg"])
    cond = occ_condition_from_config(cfg)(frames)
    paths = [str(tmp_path / "occ_bg" / ("%d.png" % i)) for i in range(2)]
    save_png(frames, paths)
    files = [open(p, "rb").read() for p in paths]
    again = OccCondition()(files)
    assert cond.shape == (2, 3, C.ORS_H, 6 * C.ORS_W) and torch.equal(cond, again)
