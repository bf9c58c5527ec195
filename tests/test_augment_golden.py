"""CPU: semstereo_amd.augment against the reference's own KITTIDataset.__getitem__ (datasets/kitti_dataset_15_aug.py, training branch),
recorded in tests/golden/augment.npz by tests/golden/make_golden_augment.py together with the draws the reference made.  The test feeds
the recorded draws to AugmentParams and the composition must give the recorded left, right, disparity and label bit for bit, and
disparity_4 the recorded disparity_low where the image is at least the crop (no GPU and no reference needed)."""
import functools
import os

import numpy as np
import pytest

from golden import augment_cases as gc

NPZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment.npz")


@functools.lru_cache(maxsize=None)
def arrays():
    with np.load(NPZ) as f:
        return {k: f[k] for k in f.files}


def keys_of(name):
    return ("left", "right", "disparity") + (("disparity_4",) if gc.compares_low(name) else ()) + ("label",)      # the sample's order


def expected(name):
    """{key: float32 array} of a case: the views through the view table, disparity_low under the name the sample gives it."""
    from semstereo_amd.data import view_table
    a, table = arrays(), view_table().numpy()
    out = {k: np.stack([table[ch][a[f"{name}/{k}"][:, ch]] for ch in range(3)], axis=1) for k in ("left", "right")}
    out.update(disparity=a[f"{name}/disparity"], label=a[f"{name}/label"])
    if gc.compares_low(name):
        out["disparity_4"] = a[f"{name}/disparity_low"]
    return out


def check(name, sample):
    want = expected(name)
    assert tuple(sample) == keys_of(name)
    for k in want:
        got = sample[k].cpu().numpy()
        assert got.dtype == np.float32 and got.shape == want[k].shape and np.array_equal(got, want[k]), (name, k)


def test_the_fixture_is_what_the_docstring_says():
    a = arrays()
    assert os.path.getsize(NPZ) < 1 << 20
    assert any(gc.compares_low(n) for n in gc.CASES) and sum(gc.CASES[n]["image"][0] < gc.CROP[0] for n in gc.CASES) >= 2
    assert sum(int((a[f"{n}/occluder"][:, 1] > 0).sum()) for n in gc.CASES) >= gc.MIN_OCCLUDERS
    for n, c in gc.CASES.items():
        assert a[f"{n}/factors"].shape == (len(c["seeds"]), 4, 2) and a[f"{n}/left"].shape == (len(c["seeds"]), 3) + gc.crop_of(n)
        assert (f"{n}/disparity_low" in a) == gc.compares_low(n)


@pytest.mark.parametrize("name", tuple(gc.CASES))
def test_composition_equals_the_reference(name):
    from semstereo_amd.augment import augment_sample
    check(name, augment_sample(gc.raw_of(name), gc.params_of(name, arrays()), keys_of(name)))
