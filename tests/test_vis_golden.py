"""CPU: the PyTorch composition of semstereo_amd.visualization against the record of the reference's own utils/visualization.py and
utils/mask_vis.py (tests/golden/vis.npz, written by tests/golden/make_golden_vis.py from the inputs of tests/golden/vis_cases.py).

Bounds: none.  The error map is a selection among ten float32 colours by comparisons of a float32 number formed by IEEE operations in the
reference's order, the class colours are integers: every picture is EQUAL to the record (torch.equal, atol 0)."""
import os

import numpy as np
import pytest
import torch

from golden import vis_cases as vc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "vis.npz"))


@pytest.fixture(scope="module")
def V():
    from semstereo_amd import visualization
    return visualization


def test_the_inputs_are_what_the_generator_asserted(V):
    vc.check_error_inputs()
    pix = vc.threshold_pixels()
    assert len(pix) == 9 and np.array_equal(V.error_colormap[:, 0], vc.BOUNDS)
    for (g, e), t in zip(pix, V.error_colormap[1:, 0]):          # a pixel ON each finite lower bound of the module's own table ...
        assert g > 0 and vc.error_measure(g, e) == t
    for i, (g, e) in enumerate(pix):                             # ... which the module colours with the row that starts there
        got = V.disp_error_image_func.apply(torch.tensor([[[float(e)]]]), torch.tensor([[[float(g)]]]), legend=False)
        assert torch.equal(got[0, :, 0, 0], torch.from_numpy(V.error_colormap[i + 1, 2:5])), i


def test_colormap_equals_the_reference_table(fx, V):
    assert V.error_colormap.dtype == np.float32 and np.array_equal(V.error_colormap, fx["colormap"])
    assert np.array_equal(V.gen_error_colormap(), fx["colormap"]) and np.array_equal(V.error_colormap[:, 0], vc.BOUNDS)


@pytest.mark.parametrize("name", list(vc.ERROR_CASES))
def test_error_map_equals_the_fixture(fx, V, name):
    d = vc.error_inputs(name)
    want = torch.from_numpy(fx[f"err/{name}"])
    got = V.disp_error_image_func.apply(d["est"], d["gt"])
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got, want), f"{name}: {(got != want).sum().item()} values differ"
    c = vc.ERROR_CASES[name]
    if c["specials"]:
        cols = torch.from_numpy(fx["colormap"][:, 2:5])
        for i in range(9):                       # a pixel ON threshold i + 1 belongs to the row above it (lo <= e < hi)
            assert torch.equal(got[0, :, 10, 2 + 4 * i], cols[i + 1]), i
        for x in (1, 6, 11, 16, 21, 26):         # NaN / +inf / -inf estimate, NaN / zero / inf ground truth: black
            assert not got[0, :, 11, x].any(), x
        assert torch.equal(got[0, :, 11, 31], cols[0])                # e = 0
    # the colour key also covers pixels whose ground truth is not valid, and stops at the picture's edge
    hh, ww = min(10, c["H"]), min(200, c["W"])
    key = torch.from_numpy(fx["colormap"][:, 2:5])[torch.arange(ww) // 20].t()
    assert torch.equal(got[:, :, :hh, :ww], key.reshape(1, 3, 1, ww).expand(c["B"], 3, hh, ww))
    if name == "clip_h_1x7x201":
        assert not torch.equal(got[0, :, :, 200], key[:, -1:].expand(3, 7))          # column 200 is picture, not key


def test_error_map_variants(V):
    d = vc.error_inputs("ragged_3x75x203")
    est, gt = d["est"], d["gt"]
    full = V.disp_error_image_func.apply(est, gt)
    bare = V.disp_error_image_func.apply(est, gt, legend=False)
    assert torch.equal(bare[:, :, 10:], full[:, :, 10:]) and torch.equal(bare[:, :, :, 200:], full[:, :, :, 200:])
    assert not torch.equal(bare[:, :, :10, :200], full[:, :, :10, :200])
    # float64 inputs: the same comparisons on exact values; a picture in float32
    assert V.disp_error_image_func.apply(est.double(), gt.double()).dtype == torch.float32
    # signed: on a ground truth that is positive wherever it is valid, an all-embracing range reproduces the default away from gt = inf
    fin = torch.where(torch.isinf(gt), torch.zeros_like(gt), gt)
    assert torch.equal(V.disp_error_image_func.apply(est, fin.clamp(min=0), signed=True), V.disp_error_image_func.apply(est, fin.clamp(min=0)))
    # ... and a negative ground truth is coloured by its own size: the mirror image of the positive case
    a = V.disp_error_image_func.apply(-est, -fin, signed=True, legend=False)
    b = V.disp_error_image_func.apply(est, fin, signed=True, legend=False)
    assert torch.equal(a, b) and bool((b.sum(1)[fin < 0] > 0).any())
    ranged = V.disp_error_image_func.apply(est, fin, signed=True, valid_range=(-5.0, 5.0), legend=False)
    outside = (fin < -5.0) | (fin >= 5.0)
    assert not ranged.permute(0, 2, 3, 1)[outside].any() and torch.equal(ranged.permute(0, 2, 3, 1)[~outside], b.permute(0, 2, 3, 1)[~outside])
    # other thresholds are honoured
    assert not torch.equal(V.disp_error_image_func.apply(est, gt, abs_thres=1., rel_thres=0.01), full)


@pytest.mark.parametrize("name", list(vc.LOGIT_CASES))
def test_feature_vis_equals_the_fixture(fx, V, name):
    z = vc.logit_inputs(name)["logits"]
    want = fx[f"logits/{name}"]
    got = V.feature_vis(z)
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32
    assert np.array_equal(got.numpy().astype(np.float64), want.astype(np.float64))       # the reference returns float64
    assert torch.equal(V.feature_vis(z, dtype=torch.uint8), torch.from_numpy(want))
    # the edge cases of row 0 by hand: ties -> first, NaN -> first NaN
    C = z.shape[1]
    pal = torch.tensor(V.PALETTE, dtype=torch.float32)
    for x, cls in ((0, 0), (1, 1), (2, 1), (3, C - 1), (4, 1), (5, 0), (6, 0)):
        assert torch.equal(got[0, :, 0, x], pal[cls]), (x, cls)


@pytest.mark.parametrize("name", list(vc.LABEL_CASES))
def test_label_vis_equals_the_reference_on_the_one_hot_tensor(fx, V, name):
    d = vc.label_inputs(name)
    want = torch.from_numpy(fx[f"labels/{name}"])
    assert d["labels"].dtype == vc.LABEL_CASES[name]["dtype"]
    assert torch.equal(V.label_vis(d["labels"], dtype=torch.uint8), want)
    assert torch.equal(V.label_vis(d["labels"]), want.float())
    assert torch.equal(V.label_vis(d["inside"]), want.float())
    onehot = torch.nn.functional.one_hot(d["inside"], vc.NCLS).permute(0, 3, 1, 2).float()
    assert torch.equal(V.feature_vis(onehot), want.float())


def test_departures_labels_outside_and_more_than_six_channels(V):
    y = torch.tensor([[[0, 5, 6, -1, 255, 3]]])
    pal = torch.tensor(V.PALETTE + ((0, 0, 0),), dtype=torch.float32)
    assert torch.equal(V.label_vis(y)[0, :, 0].t(), pal[torch.tensor([0, 5, 6, 6, 6, 3])])
    f = torch.tensor([[[float("nan"), -0.5, 5.99, 6.0, -1.0, float("inf")]]])
    assert torch.equal(V.label_vis(f)[0, :, 0].t(), pal[torch.tensor([6, 0, 5, 6, 6, 6])])
    z = torch.zeros(1, 8, 1, 3)
    z[0, 7, 0, 0], z[0, 2, 0, 1] = 1.0, 1.0
    assert torch.equal(V.feature_vis(z)[0, :, 0].t(), pal[torch.tensor([6, 2, 0])])


def test_normalize_image_is_the_stated_formula(V):
    x = torch.from_numpy(vc.dd.uniform((2, 3, 9, 13), 77, -3.0, 9.0))
    lo, hi = x.reshape(2, -1).amin(1).view(2, 1, 1, 1), x.reshape(2, -1).amax(1).view(2, 1, 1, 1)
    assert torch.equal(V.normalize_image(x), (x.clamp(lo, hi) - lo) / (hi - lo).clamp(min=1e-5))
    one = V.normalize_image(x[:, 0])                                  # [B,H,W]: one channel, returned as three equal ones
    assert one.shape == (2, 3, 9, 13) and torch.equal(one[:, 0], one[:, 1]) and torch.equal(one[:, 0], one[:, 2])
    flat = V.normalize_image(torch.full((1, 1, 4, 4), 2.5))           # a constant picture: 0 / 1e-5
    assert flat.shape == (1, 3, 4, 4) and not flat.any()
