"""CPU restatement of the image-mode ORS panorama — TEST INFRASTRUCTURE ONLY.

Restates the `__main__` block of magicdrive/networks/occ3d_proj.py:156-203 on the labels of
`oracle.ors_projection.ors_project` (itself pinned bit for bit to the reference's `project()`): the optional
foreground / background filter (:157, :160), the first label that is not 17 by the reference's `argmax` rule (:165-169:
an all-17 ray gives index 0 and value 17), the palette (:171-194), the views side by side (:197) and the blend over
the camera pictures (:196-203) in numpy / torch float32, call for call.  PINNED: tests/golden/mint_occ_render.py
executes the reference's own lines and tests/test_occ_render_cpu.py compares this file with what they gave, byte for byte.
"""
import numpy as np
import torch

from oracle import ors_projection as P

# colors_map[:, :3] of occ3d_proj.py:171-191, class -> (r, g, b)
PALETTE = np.array([[0, 0, 0], [255, 120, 50], [255, 192, 203], [255, 255, 0], [0, 150, 245], [0, 255, 255], [255, 127, 0],
                    [255, 0, 0], [255, 240, 150], [135, 60, 0], [160, 32, 240], [255, 0, 255], [139, 137, 137], [75, 0, 75],
                    [150, 240, 80], [230, 230, 250], [0, 175, 0], [0, 0, 0]], dtype=np.uint8)
MODES = ("all", "bg", "fg")


def filter_labels(labels, mode):
    """:157 ("bg": foregrounds, classes <= 10, become 17) / :160 ("fg": backgrounds, classes >= 11, become 17)"""
    if mode == "bg":
        return torch.where(labels <= 10, 17, labels)
    if mode == "fg":
        return torch.where(11 <= labels, 17, labels)
    if mode != "all":
        raise ValueError(mode)
    return labels


def first_hit(labels, mode="all"):
    """labels (n, h, w, S) int64 -> (classes (n, h, w) int64, index (n, h, w) int64 of the sample taken), :165-169"""
    lab = filter_labels(labels, mode)
    flat = lab.reshape(-1, lab.shape[-1])
    idx = (flat != 17).float().argmax(dim=1)
    val = flat[torch.arange(flat.size(0)), idx]
    return val.view(lab.shape[:-1]), idx.view(lab.shape[:-1])


def paint(classes, palette=PALETTE):
    """classes (n, h, w) -> the colour panorama (h, n * w, 3) uint8, :192-197"""
    cls = classes.numpy()
    img = np.zeros(cls.shape + (3,), dtype=np.uint8)
    for i in range(18):
        img[cls == i] = palette[i]
    return np.concatenate([img[i] for i in range(len(img))], axis=-2)


def render(occ, intrinsics, extrinsics, h, w, compress_ratio, sample_point=320, sample_step=0.2, mode="all",
           palette=PALETTE):
    """-> (classes (n, h, w) uint8, panorama (h, n * w, 3) uint8, first-hit sample index (n, h, w))"""
    labels = P.ors_project(occ, intrinsics, extrinsics, h, w, compress_ratio, sample_point, sample_step)
    cls, idx = first_hit(labels, mode)
    return cls.numpy().astype(np.uint8), paint(cls, palette), idx.numpy()


def camera_values(camera_u8):
    """get_img, :126-129: uint8 (h, W, 3) -> float32 in [-1, 1]"""
    t = torch.tensor(np.asarray(camera_u8)) / 255
    return (t * 2 - 1).numpy()


def overlay(colour, camera_u8):
    """colour, camera_u8: (h, W, 3) uint8 panoramas of one sample -> the blend, uint8 (:196-203 and the cast of :206).
    The minimum and maximum run over the whole sample, as they run over all six views there."""
    x = camera_values(camera_u8)
    d = (x - np.min(x)) / (np.max(x) - np.min(x)) * 255
    c, d = torch.tensor(np.asarray(colour)), torch.tensor(d)
    fg, bg = c == 0, c != 0
    res = c.masked_fill(fg, 0) * 0.7 + d.masked_fill(fg, 0) * 0.3 + d.masked_fill(bg, 0)
    return res.numpy().astype(np.uint8)


def camera_pictures(h=28, w=50, views=6, seed=4107):
    """seeded uint8 (views, h, w, 3) camera pictures: a ramp plus noise, so that the blend sees its whole range (what
    tests/golden/mint_occ_render.py fed the reference's get_img at the fixture's size)"""
    g = torch.Generator().manual_seed(seed)
    ramp = torch.linspace(8, 240, w).view(1, 1, w, 1).expand(views, h, w, 3)
    noise = torch.randint(-8, 16, (views, h, w, 3), generator=g)
    return (ramp + noise).clamp(0, 255).to(torch.uint8).numpy()


def camera_panorama(pictures):
    """(views, h, w, 3) -> (h, views * w, 3), the views side by side (:198)"""
    return np.concatenate([pictures[i] for i in range(len(pictures))], axis=-2)


def random_rig(g, n_cam):
    """rigs as tests/test_ops_gpu.py:test_ors_projection_random_rigs makes them"""
    Ks, Rts = [], []
    for i in range(n_cam):
        q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
        Rt = torch.eye(4, dtype=torch.float64)
        Rt[:3, :3] = q
        Rt[:3, 3] = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * torch.tensor([90.0, 90.0, 8.0])
        Rt[2, 3] += 2.0
        Ks.append(torch.tensor([[1260.0 + 10 * i, 0.0, 800.0], [0.0, 1255.0, 450.0 + 5 * i], [0.0, 0.0, 1.0]]))
        Rts.append(Rt.float())
    return Ks, Rts


def looking_in(t):
    """A camera at t with the axes of tests/test_ops_gpu.py:test_ors_projection_edge_cases: z forward = +x of the ego
    frame, x right = -y, y down = -z."""
    Rt = torch.eye(4)
    Rt[:3, :3] = torch.tensor([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])
    Rt[:3, 3] = torch.tensor(t)
    return Rt
