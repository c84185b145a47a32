"""Mints tests/golden/occ_render.npz by executing the REFERENCE'S OWN LINES (LEVEL 1).

Runs only where the reference checkout is present; nothing here is used at test time, and no reference text is
copied: the lines are read from the reference's file when this script runs and executed on prepared locals.

  * labels: the reference's `OccupancyRay.project` on `cases.ors_inputs()`, set up exactly as `mint.mint_ors` does;
  * camera pictures: the reference's `get_img` (networks/occ3d_proj.py:118-131) over a stand-in `nusc` and a stand-in
    `Image.open` that hand back seeded uint8 pictures of the render's size (no file, no resize);
  * the panorama and the blend: lines 156-203 of networks/occ3d_proj.py, with the filter line of the mode (:157 for
    "bg", :160 for "fg") un-commented, and the uint8 cast of :206.

Usage:  python tests/golden/mint_occ_render.py      (rewrites tests/golden/occ_render.npz)
"""
import os
import sys
import tempfile
import textwrap

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.golden import cases as C          # noqa: E402
from tests.golden import mint as M           # noqa: E402
from tests import occ_render_reference as R  # noqa: E402

FIRST, LAST = 156, 203                       # the lines executed, 1-based, inclusive
FILTER_LINE = {"all": None, "bg": 157, "fg": 160}


def reference_block(path, mode):
    lines = open(path).read().split("\n")
    block = lines[FIRST - 1:LAST]
    if FILTER_LINE[mode] is not None:
        k = FILTER_LINE[mode] - FIRST
        assert block[k].lstrip().startswith("# project_feat = torch.where("), block[k]
        block[k] = block[k].replace("# project_feat", "project_feat", 1)
    return textwrap.dedent("\n".join(block))


def main():
    M.install_stubs()
    M._mod("cv2")

    class Quaternion:
        def __init__(self, rot):
            self.rotation_matrix = np.asarray(rot, dtype=np.float64)
    M._mod("pyquaternion", Quaternion=Quaternion)
    from magicdrive.networks import occ3d_proj as ref_ors
    occ, Ks, Rts = C.ors_inputs()
    tok = "seeded-sample"
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, "scene"))
        np.savez(os.path.join(root, "scene", "labels.npz"), semantics=occ.numpy().astype(np.uint8))
        proj = object.__new__(ref_ors.OccupancyRay)               # skip __init__: it unpickles data files
        proj.camera_data = {tok: {v: {"translation": Rts[i][:3, 3].tolist(), "rotation": Rts[i][:3, :3].numpy(),
                                      "intrinsic": Ks[i].tolist()} for i, v in enumerate(C.ORS_VIEWS)}}
        proj.occ3d_idx = {tok: "scene"}
        proj.device = "cpu"
        proj.dataroot = root
        proj.image_shape = (896, 1600)
        proj.sample_point = C.ORS_S
        proj.sample_step = 0.2
        proj.compress_ratio = C.ORS_RATIO
        proj.image_shape_compress = [int(896 * C.ORS_RATIO), int(1600 * C.ORS_RATIO)]
        labels = proj.project(tok)                                 # (6, 28, 50, 320) int64
    assert tuple(labels.shape) == (6, C.ORS_H, C.ORS_W, C.ORS_S), labels.shape

    cams = R.camera_pictures()                                     # seeded uint8 (6, 28, 50, 3)

    class Picture:                                                 # what get_img asks of PIL
        def __init__(self, arr):
            self.arr = arr

        def resize(self, size):
            assert tuple(size) == (C.ORS_W, C.ORS_H), size
            return self.arr

    class Nusc:
        def get(self, table, key):
            return {"data": {v: v for v in C.ORS_VIEWS}} if table == "sample" else {"filename": key}

    class Image:
        @staticmethod
        def open(path):
            return Picture(cams[C.ORS_VIEWS.index(os.path.basename(path))])
    ref_ors.Image = Image                                          # the reference imports PIL's under `__main__` only
    h, w = 896, 1600
    img = ref_ors.get_img(Nusc(), tok, nuscroot="", w=int(w * C.ORS_RATIO), h=int(h * C.ORS_RATIO))   # (6, 3, 28, 50)
    assert tuple(img.shape) == (6, 3, C.ORS_H, C.ORS_W) and img.dtype == torch.float32

    out = {}
    path = os.path.join(os.path.dirname(ref_ors.__file__), "occ3d_proj.py")
    for mode in ("all", "bg", "fg"):
        env = {"torch": torch, "np": np, "img": img.clone(), "project_feat": labels.clone(), "sample_point": C.ORS_S,
               "h": h, "w": w, "compress_ratio": C.ORS_RATIO}
        exec(compile(reference_block(path, mode), "occ3d_proj.py:%d-%d" % (FIRST, LAST), "exec"), env)
        out["classes_" + mode] = env["result_occ"].numpy().astype(np.uint8)            # (6, 28, 50)
        out["frames_" + mode] = env["colored_image"].numpy()                           # (28, 300, 3) uint8
        out["overlay_" + mode] = env["res"].numpy().astype(np.uint8)                   # the cast of :206
        assert out["frames_" + mode].dtype == np.uint8 and out["frames_" + mode].shape == (C.ORS_H, 6 * C.ORS_W, 3)
        print(mode, "hit share %.3f" % float((out["classes_" + mode] != 17).mean()))
    dst = os.path.join(HERE, "occ_render.npz")
    np.savez_compressed(dst, **out)
    print("wrote %s (%.1f KB)" % (dst, os.path.getsize(dst) / 1024))


if __name__ == "__main__":
    main()
