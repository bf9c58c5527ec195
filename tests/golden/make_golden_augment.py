#!/usr/bin/env python3
"""Generate tests/golden/augment.npz by running the REFERENCE's own datasets/kitti_dataset_15_aug.py (imported by path; nothing is
copied): every item of augment_cases.py is written as KITTI-layout PNG files (8-bit views and label, 16-bit disparity) and read back
through the real KITTIDataset.__getitem__, training branch.  Runs only where the reference is mounted (REF below, as in
make_golden_data.py); the tests elsewhere read the committed file.

cv2 and torchvision are not installed where this runs; PIL is.  Stand-ins are installed before the import: those of make_golden_data.py
(cv2.resize INTER_NEAREST, torchvision.transforms.ToTensor / Normalize / Compose) and
  torchvision.transforms.functional   the four calls torchvision's PIL backend makes: ImageEnhance.Brightness / Contrast / Color
                                      (...).enhance(factor), and Image.point() with the table
                                      [int((255 + 1 - 1e-3) * gain * pow(e / 255.0, gamma)) for e in range(256)] * 3 for adjust_gamma
The reference draws with np.random.uniform, np.random.binomial and random.randint; the generator wraps the three in its own process,
records what they return and stores the draws next to the outputs:
  <case>/factors    float64 [B,4,2]   brightness, gamma, contrast, saturation of (left, right)
  <case>/origin     int64 [B,2]       (y1, x1) of RandomCrop
  <case>/occluder   int64 [B,4]       (row centre, row half-size, column centre, column half-size), -1 without one -- the reference
                                      names the row pair (cx, sx) and the column pair (cy, sy)
  <case>/left, right   uint8 [B,3,th,tw]   the codes u with view_table()[ch][u] == the reference's float, the table's exact inverse
                                      (every value is asserted to be in the table)
  <case>/disparity, label   float32 [B,th,tw];  <case>/disparity_low float32 [B,th/4,tw/4] where the image is at least the crop
Before anything is written the generator asserts that the reference's occluder colour equals the integer floor of the exact mean on
every committed item, that at least MIN_OCCLUDERS items carry an occluder, and that no output holds a NaN.  Numeric arrays only, fixed
member dates: the same arrays give the same file.

    python tests/golden/make_golden_augment.py            # writes tests/golden/augment.npz
"""
import importlib
import os
import random
import sys
import tempfile
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_golden_data as mgd  # noqa: E402
from golden import augment_cases as gc  # noqa: E402

REF = mgd.REF
OUT = os.path.join(HERE, "augment.npz")
DRAWS = {"uniform": [], "binomial": [], "randint": []}


def install_stand_ins():
    from PIL import ImageEnhance
    mgd.install_stand_ins()
    F = types.ModuleType("torchvision.transforms.functional")
    F.adjust_brightness = lambda im, f: ImageEnhance.Brightness(im).enhance(f)
    F.adjust_contrast = lambda im, f: ImageEnhance.Contrast(im).enhance(f)
    F.adjust_saturation = lambda im, f: ImageEnhance.Color(im).enhance(f)
    F.adjust_gamma = lambda im, gamma, gain=1: im.point([int((255 + 1 - 1e-3) * gain * pow(e / 255.0, gamma)) for e in range(256)] * 3)
    sys.modules["torchvision.transforms"].functional = F
    sys.modules["torchvision.transforms.functional"] = F


def record_draws():
    uniform, binomial, randint = np.random.uniform, np.random.binomial, random.randint

    def _uniform(lo, hi, size=None):
        v = uniform(lo, hi, size)
        DRAWS["uniform"].append(np.array(v, dtype=np.float64).copy())
        return v

    def _binomial(n, p):
        v = binomial(n, p)
        DRAWS["binomial"].append(int(v))
        return v

    def _randint(a, b):
        v = randint(a, b)
        DRAWS["randint"].append(int(v))
        return v
    np.random.uniform, np.random.binomial, random.randint = _uniform, _binomial, _randint


def load_ref():
    """datasets/kitti_dataset_15_aug.py of the reference, imported from its own folder as the package `datasets`."""
    install_stand_ins()
    pkg = types.ModuleType("datasets")
    pkg.__path__ = [os.path.join(REF, "datasets")]
    sys.modules["datasets"] = pkg
    return importlib.import_module("datasets.kitti_dataset_15_aug")


def codes_of(view):
    """uint8 [3,h,w] with view_table()[ch][code] == view: the table's exact inverse."""
    from semstereo_amd.data import view_table
    table = view_table().numpy()
    out = np.empty(view.shape, dtype=np.uint8)
    for ch in range(3):
        assert np.all(np.diff(table[ch]) > 0)
        idx = np.searchsorted(table[ch], view[ch])
        assert idx.max() < 256 and np.array_equal(table[ch][idx], view[ch]), "a value that is not in the view table"
        out[ch] = idx
    return out


def run_item(kitti, folder, name, seed):
    from PIL import Image
    left, right, disp, label = gc.item(name, seed)
    for sub, a in (("image_2", left), ("image_3", right), ("disp_occ_0", disp), ("semantic", label)):
        os.makedirs(os.path.join(folder, "x", sub), exist_ok=True)
        Image.fromarray(a).save(os.path.join(folder, "x", sub, "0.png"))
    lst = os.path.join(folder, "list.txt")
    with open(lst, "w") as f:
        f.write("x/image_2/0.png x/image_3/0.png x/disp_occ_0/0.png\n")
    np.random.seed(seed)
    random.seed(seed)
    for v in DRAWS.values():
        v.clear()
    sample = kitti.KITTIDataset(folder, lst, True)[0]
    U, (x1, y1) = DRAWS["uniform"], DRAWS["randint"]
    assert len(DRAWS["binomial"]) == 2 and len(U) in (4, 8)
    occluder = (-1, -1, -1, -1)
    if DRAWS["binomial"][1]:
        occluder = (int(U[6]), int(U[4]), int(U[7]), int(U[5]))
    rec = {"factors": np.stack(U[:4]), "origin": np.array([y1, x1], dtype=np.int64), "occluder": np.array(occluder, dtype=np.int64)}
    rec["left"], rec["right"] = codes_of(sample["left"].numpy()), codes_of(sample["right"].numpy())
    rec["disparity"], rec["label"] = sample["disparity"], sample["label"]
    th, tw = gc.crop_of(name)
    assert rec["left"].shape == (3, th, tw) and rec["disparity"].shape == (th, tw) and rec["disparity"].dtype == np.float32
    if gc.compares_low(name):
        rec["disparity_low"] = sample["disparity_low"]
    if occluder[1] > 0:
        # the reference paints uint8(numpy's two-stage float64 mean); the definition is floor(exact sum / (th tw)).  Outside the
        # rectangle the right view is what the sums run over, inside it is the colour: recover the colour and compare both ways
        cy, sy, cx, sx = occluder
        painted = rec["right"][:, cy, cx]
        assert np.all(rec["right"][:, cy - sy:cy + sy, cx - sx:cx + sx] == painted.reshape(3, 1, 1))
        rec["_painted"] = painted
    return rec


def generate(path=OUT):
    warnings.filterwarnings("ignore")
    from semstereo_amd.augment import augment_sample
    record_draws()
    kitti = load_ref()
    out, occluders = {}, 0
    with tempfile.TemporaryDirectory() as folder:
        for name, c in gc.CASES.items():
            items = [run_item(kitti, folder, name, s) for s in c["seeds"]]
            for k in items[0]:
                if not k.startswith("_"):
                    out[f"{name}/{k}"] = np.stack([it[k] for it in items])
            # the occluder colour: the integer floor, from the un-occluded right view of the composition with the recorded draws
            arrays = {k: v for k, v in out.items() if k.startswith(name + "/")}
            P = gc.params_of(name, arrays)
            P.occluder[:] = -1
            th, tw = gc.crop_of(name)
            clean = augment_sample(gc.raw_of(name), P, ("right",))["right"].numpy()
            for i, it in enumerate(items):
                if "_painted" in it:
                    occluders += 1
                    exact = codes_of(clean[i]).astype(np.int64).reshape(3, -1).sum(1) // (th * tw)
                    assert np.array_equal(exact, it["_painted"].astype(np.int64)), (name, i, exact, it["_painted"])
    assert occluders >= gc.MIN_OCCLUDERS, occluders
    for k, a in out.items():
        assert not np.isnan(a.astype(np.float64)).any(), k
    mgd.save_deterministic(path, out)
    return out, occluders


if __name__ == "__main__":
    assert os.path.isdir(REF), "the reference is only mounted in the build container"
    res, n = generate()
    for k in sorted(res):
        print(k, res[k].dtype, res[k].shape)
    print("augment.npz:", len(res), "arrays,", n, "items with an occluder,", os.path.getsize(OUT) // 1024, "KiB")
