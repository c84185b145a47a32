"""Mints tests/golden/fid.npz from the reference's tools/fid_score.py:

    python tests/golden/mint_fid.py <path to MD_txt_con_fusion/tools/fid_score.py>

The file is loaded by path.  The modules it imports at its top and that are not installed here (omegaconf, hydra,
torchvision, the reference's own packages) get name-only stand-ins of our own: nothing of them is called by the two
functions used, `calculate_frechet_distance` and `top_center_crop`.  The fixture stores data only — inputs, the
reference's results and the reference's own noise — and no text of the reference.

Frechet cases (tests/test_fid_cpu.py):
  full_<d>   d = 8, 64: statistics of N = 4 d seeded samples each (full rank, well conditioned); `d12`, `d21` are
             the reference's value with the arguments in both orders: |d12 - d21| is its own noise.
  diag_<d>   diagonal covariances: the value is known in closed form, |dmu|^2 + sum (sqrt a - sqrt b)^2.
Crop cases: for the four image_size / augment2d.resize pairs of the reference's dataset configs, the resize size of
fid_score.py:478-479 and the box `top_center_crop` cuts, read back from an image whose pixels hold their own index.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# (image_size, augment2d.resize): configs/dataset/Nuscenes.yaml (the active pair and the commented devfusion pair),
# configs/exp-hd/256x704.yaml, configs/exp-hd/432x768.yaml
CROP_CASES = [((224, 400), [[0.25, 0.25]]), ((256, 704), [[0.38, 0.55], [0.48, 0.48]]),
              ((256, 704), [[0.48, 0.48]]), ((432, 768), [[0.48, 0.48]])]


def _stand_in(name, **attrs):
    mod = types.ModuleType(name)
    mod.__dict__.update(attrs)
    sys.modules[name] = mod
    return mod


def load_reference(path):
    def passthrough(*_a, **_k):
        return lambda fn: fn

    names = ["omegaconf", "hydra", "hydra.utils", "hydra.core", "hydra.core.hydra_config", "torchvision",
             "torchvision.transforms", "magicdrive", "magicdrive.misc", "magicdrive.misc.inception", "perception",
             "perception.common", "perception.common.nuscenes_utils"]
    missing = []
    for n in names:
        try:
            importlib.import_module(n)
        except ImportError:
            missing.append(n)
    for n in missing:
        _stand_in(n)
    if "omegaconf" in missing:
        sys.modules["omegaconf"].OmegaConf = None
    if "hydra" in missing:
        sys.modules["hydra"].main = passthrough
        sys.modules["hydra.utils"].to_absolute_path = None
        sys.modules["hydra.core.hydra_config"].HydraConfig = None
    if "torchvision" in missing:
        sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    if "magicdrive.misc.inception" in missing:
        sys.modules["magicdrive.misc.inception"].InceptionV3 = None
    if "perception.common.nuscenes_utils" in missing:
        sys.modules["perception.common.nuscenes_utils"].sample_token_from_scene = None
    spec = importlib.util.spec_from_file_location("reference_fid_score", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(path):
    from PIL import Image
    ref = load_reference(path)
    out = {}
    rng = np.random.RandomState(20260)
    for d in (8, 64):
        n = 4 * d
        mix1, mix2 = rng.randn(d, d) / np.sqrt(d) + np.eye(d), rng.randn(d, d) / np.sqrt(d) + np.eye(d)
        a1 = rng.randn(n, d) @ mix1 + rng.randn(d)
        a2 = rng.randn(n, d) @ mix2 * 1.3 + rng.randn(d)
        mu1, mu2 = np.mean(a1, axis=0), np.mean(a2, axis=0)
        s1, s2 = np.cov(a1, rowvar=False), np.cov(a2, rowvar=False)
        out["full_%d_mu1" % d], out["full_%d_mu2" % d] = mu1, mu2
        out["full_%d_s1" % d], out["full_%d_s2" % d] = s1, s2
        out["full_%d_d12" % d] = np.float64(ref.calculate_frechet_distance(mu1, s1, mu2, s2))
        out["full_%d_d21" % d] = np.float64(ref.calculate_frechet_distance(mu2, s2, mu1, s1))
        a, b = rng.rand(d) * 2 + 0.1, rng.rand(d) * 2 + 0.1
        m1, m2 = rng.randn(d), rng.randn(d)
        out["diag_%d_a" % d], out["diag_%d_b" % d], out["diag_%d_mu1" % d], out["diag_%d_mu2" % d] = a, b, m1, m2
        out["diag_%d_d12" % d] = np.float64(ref.calculate_frechet_distance(m1, np.diag(a), m2, np.diag(b)))
        out["diag_%d_d21" % d] = np.float64(ref.calculate_frechet_distance(m2, np.diag(b), m1, np.diag(a)))
    crops = []
    for image_size, resize in CROP_CASES:
        ratio = np.mean(resize[0])                                       # fid_score.py:478
        size = (int(900 * ratio), int(1600 * ratio))                     # :479 with IN_SIZE = (900, 1600)
        index = np.arange(size[0] * size[1], dtype=np.int32).reshape(size)
        cut = np.asarray(ref.top_center_crop(Image.fromarray(index, mode="I"), target_size=list(image_size)))
        top, left = divmod(int(cut[0, 0]), size[1])
        bottom, right = divmod(int(cut[-1, -1]), size[1])
        assert cut.shape == tuple(image_size)
        crops.append([image_size[0], image_size[1], resize[0][0], resize[0][1], size[0], size[1],
                      left, top, right + 1, bottom + 1])
    out["crop_cases"] = np.asarray(crops, dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "fid.npz"), **out)
    for k in sorted(out):
        print(k, out[k].shape if out[k].ndim else float(out[k]))


if __name__ == "__main__":
    main(sys.argv[1])
