"""The cases of tests/golden/augment.npz: synthetic KITTI-layout items that make_golden_augment.py writes as PNG files and reads back
through the reference's own KITTIDataset.__getitem__ (training branch), and that the tests rebuild from the same seeds as raw arrays.
Blocky content: it compresses, and every photometric step is pointwise, so the outputs stay blocky too."""
import numpy as np
import torch

CROP = (256, 512)          # datasets/kitti_dataset_15_aug.py:101
BLOCK = 16
#: name -> image size and the seeds of its items (np.random.seed / random.seed of the reference's draws, and the content's).  "large"
#: exceeds the crop in both axes: the origin, disparity_low and a full-size rectangle are the reference's.  With H < 256 the crop shrinks
#: to the image and disparity_low is not compared (the reference resizes to a fixed 64 x 128 there).  The seeds are chosen so that at
#: least three items carry an occluder (the generator asserts it).
CASES = {
    "large": dict(image=(272, 528), seeds=(3, 11, 16, 22)),
    "short": dict(image=(208, 544), seeds=(5, 16, 28)),
    "short_narrow": dict(image=(240, 520), seeds=(2, 22)),
}
KEYS = ("left", "right", "disparity", "label")
MIN_OCCLUDERS = 3


def crop_of(name):
    H, W = CASES[name]["image"]
    return min(CROP[0], H), min(CROP[1], W)


def compares_low(name):
    return CASES[name]["image"][0] >= CROP[0] and CASES[name]["image"][1] >= CROP[1]


def item(name, seed):
    """(left uint8 [H,W,3], right uint8 [H,W,3], disparity uint16 [H,W] in 1/256 px, label uint8 [H,W]) of one item."""
    H, W = CASES[name]["image"]
    rng = np.random.default_rng(1000 * (sorted(CASES).index(name) + 1) + seed)
    h, w = -(-H // BLOCK), -(-W // BLOCK)

    def blocks(lo, hi, channels=()):
        a = rng.integers(lo, hi, (h, w) + channels)
        return np.kron(a, np.ones((BLOCK, BLOCK) + (1,) * len(channels), dtype=np.int64))[:H, :W]
    ramp = (np.arange(W) // 4 % 8).reshape(1, W, 1)                              # a little structure inside a block
    left = np.clip(blocks(0, 256, (3,)) + ramp, 0, 255).astype(np.uint8)
    right = np.clip(blocks(0, 256, (3,)) - ramp, 0, 255).astype(np.uint8)
    return left, right, blocks(0, 60 * 256).astype(np.uint16), blocks(0, 34).astype(np.uint8)


def raw_of(name):
    """prepare_sample's `raw` of a case: the arrays as RawStereoDataset(kind="whu")-style decoding delivers them, plus the label."""
    items = [item(name, s) for s in CASES[name]["seeds"]]
    return {"left_u8": torch.from_numpy(np.stack([i[0] for i in items])), "right_u8": torch.from_numpy(np.stack([i[1] for i in items])),
            "disparity": torch.from_numpy(np.stack([i[2] for i in items]).astype(np.int32)),
            "label": torch.from_numpy(np.stack([i[3] for i in items]))}


def params_of(name, arrays):
    """AugmentParams of a case from the recorded draws in `arrays` (the loaded npz)."""
    from semstereo_amd.augment import AugmentParams
    f = arrays[f"{name}/factors"]                                                # [B,4,2]: brightness, gamma, contrast, saturation
    return AugmentParams(crop_of(name), CASES[name]["image"], arrays[f"{name}/origin"], occluder=arrays[f"{name}/occluder"],
                         brightness=f[:, 0], gamma=f[:, 1], contrast=f[:, 2], saturation=f[:, 3])
