"""Closed-form raw inputs of the sample-preparation fixture (tests/golden/data.npz): shared by make_golden_data.py, which writes them to
image files and runs the reference's own datasets/us3d_.py and datasets/whu_dataset.py on those, and by the tests, which feed them to
semstereo_amd.data.  Values come from oracle.detdata and integer numpy arithmetic, so they are the same bits wherever they are built.

Also here, because both test files need it: `ulp_distance`, the float32 criterion of the gx / gy comparisons."""
import os

import numpy as np
import torch

from oracle import detdata as dd

# name: dataset kind, items, height, width, seed, how the views are filled, whether the pyramid levels are recorded and compared
CASES = {
    "random_32x48": dict(kind="us3d", B=1, H=32, W=48, seed=7100, fill="random", pyramids=True),
    "odd_37x53": dict(kind="us3d", B=1, H=37, W=53, seed=7110, fill="random", pyramids=False),       # odd sizes: views and gradients only
    "halves_32x32": dict(kind="us3d", B=1, H=32, W=32, seed=7120, fill="halves", pyramids=True),     # left half 255, right half 0
    "constant_16x16": dict(kind="us3d", B=1, H=16, W=16, seed=7130, fill="constant", pyramids=True),  # std = 0: gx, gy are NaN everywhere
    "batch_2x16x32": dict(kind="us3d", B=2, H=16, W=32, seed=7140, fill="two_statistics", pyramids=True),
    "row_1x5": dict(kind="us3d", B=1, H=1, W=5, seed=7150, fill="random", pyramids=False),            # the test branch only
    "whu_16x48": dict(kind="whu", B=1, H=16, W=48, seed=7160, fill="random", pyramids=True),
}
NAN_CASE = "constant_16x16"
VIEW_KEYS, GRAD_KEYS = ("left", "right"), ("gx", "gy")
DISP_LEVEL_KEYS, LABEL_LEVEL_KEYS = ("disparity_4", "disparity_8", "disparity_16"), ("label_2", "label_4")


def _bytes(shape, seed, lo=0.0, hi=256.0):
    return np.clip(np.floor(dd.uniform(shape, seed, lo, hi)), 0, 255).astype(np.uint8)


def has_training_branch(name):
    """cv2.resize refuses an empty destination: the training branch needs h // 16 and w // 16 of at least 1."""
    c = CASES[name]
    return c["H"] >= 16 and c["W"] >= 16


def level_keys(name):
    c = CASES[name]
    if not c["pyramids"]:
        return ()
    return DISP_LEVEL_KEYS + (LABEL_LEVEL_KEYS if c["kind"] == "us3d" else ())


def raw_inputs(name):
    """The raw arrays a RawStereoDataset item holds, stacked over the case's items: `left_u8`, `right_u8` uint8 [B,H,W,3]; `disparity`
    float32 [B,H,W] (US3D, with -999 holes) or int32 [B,H,W] (WHU: the integers of a 16-bit file); `label` uint8 [B,H,W] (US3D)."""
    c = CASES[name]
    B, H, W, s = c["B"], c["H"], c["W"], c["seed"]
    if c["fill"] == "random":
        left = _bytes((B, H, W, 3), s)
    elif c["fill"] == "halves":
        left = np.zeros((B, H, W, 3), dtype=np.uint8)
        left[:, :, :W // 2] = 255
    elif c["fill"] == "constant":
        left = np.empty((B, H, W, 3), dtype=np.uint8)
        left[...] = np.array([90, 120, 30], dtype=np.uint8)
    else:                                                   # item 0: dark and flat; item 1: the full range
        left = np.concatenate([_bytes((1, H, W, 3), s, 20.0, 44.0), _bytes((1, H, W, 3), s + 5)], axis=0)
    right = _bytes((B, H, W, 3), s + 1)
    out = {"left_u8": torch.from_numpy(left), "right_u8": torch.from_numpy(right)}
    if c["kind"] == "us3d":
        d = dd.uniform((B, H, W), s + 2, -60.0, 60.0).copy()
        d[dd.uniform((B, H, W), s + 3) < -0.8] = -999.0
        out["disparity"] = torch.from_numpy(d)
        out["label"] = torch.from_numpy(np.minimum(np.floor(dd.uniform((B, H, W), s + 4, 0.0, 6.0)), 5).astype(np.uint8))
    else:
        out["disparity"] = torch.from_numpy(np.floor(dd.uniform((B, H, W), s + 2, 0.0, 65536.0)).clip(0, 65535).astype(np.int32))
    return out


def write_case(name, folder):
    """The case's items as image files under `folder` and a list file in the reference's format; returns the list file's path."""
    from PIL import Image
    c, raw = CASES[name], raw_inputs(name)
    lines = []
    for i in range(c["B"]):
        names = [f"{name}_{i}_left.tif", f"{name}_{i}_right.tif"]
        Image.fromarray(raw["left_u8"][i].numpy(), "RGB").save(os.path.join(folder, names[0]))
        Image.fromarray(raw["right_u8"][i].numpy(), "RGB").save(os.path.join(folder, names[1]))
        if c["kind"] == "us3d":
            names += [f"{name}_{i}_disp.tif", f"{name}_{i}_label.tif"]
            Image.fromarray(raw["disparity"][i].numpy()).save(os.path.join(folder, names[2]))                # mode F
            Image.fromarray(raw["label"][i].numpy()).save(os.path.join(folder, names[3]))                    # mode L
        else:
            names += [f"{name}_{i}_disp.png"]
            Image.fromarray(raw["disparity"][i].numpy().astype(np.uint16)).save(os.path.join(folder, names[2]))   # mode I;16
        lines.append(" ".join(names))
    path = os.path.join(folder, name + ".txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def ulp_distance(a, b):
    """int64 tensor: the distance of float32 tensors `a` and `b` in units in the last place (+0 and -0 are 0 apart).  Where exactly one
    of the two is NaN the distance is 2^40; where both are, 0."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.shape == b.shape

    def ordered(t):
        i = t.view(torch.int32).long()
        return torch.where(i >= 0, i, -(i & 0x7FFFFFFF))
    d = (ordered(a) - ordered(b)).abs()
    na, nb = torch.isnan(a), torch.isnan(b)
    d = torch.where(na & nb, torch.zeros_like(d), d)
    return torch.where(na ^ nb, torch.full_like(d, 2 ** 40), d)


def assert_gradients(got, want, what):
    """The criterion of the gx / gy comparisons: NaN in the same places, every other pixel within 1 float32 ulp."""
    d = ulp_distance(got, want)
    unequal = int((d != 0).sum())
    assert int(d.max()) <= 1, f"{what}: {unequal} of {d.numel()} pixels unequal, the worst {int(d.max())} ulp apart"
    return unequal
