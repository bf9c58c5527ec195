"""CPU: the PyTorch composition of semstereo_amd.losses (what CPU, float64 and unsupported inputs run) against tests/golden/loss.npz,
the record of the reference's own models/loss.py on the same closed-form inputs (tests/golden/make_golden_loss.py).

float64 run: loss and gradients within 1e-9 of the reference's float64 values, relative to each tensor's largest magnitude, for the
disparity and LRSC losses; within 1e-7 for the label loss (the reference casts its softmax with .float(), models/loss.py:55, so its Dice
term is fp32 even in a float64 run).  float32 run: the loss within 5e-6 of the reference's float32 loss.  The warped labels of LRSC_loss
equal the reference's exactly, in both precisions."""
import os

import numpy as np
import pytest
import torch

from golden import loss_cases

HERE = os.path.dirname(os.path.abspath(__file__))
NPZ = os.path.join(HERE, "golden", "loss.npz")
TOL64 = {"train": 1e-9, "test": 1e-9, "lrsc": 1e-9, "label": 1e-7}


@pytest.fixture(scope="module")
def fx():
    return np.load(NPZ)


@pytest.fixture(scope="module")
def losses():
    import semstereo_amd
    return semstereo_amd.losses


def _close(a, ref, tol, what):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    assert np.array_equal(np.isnan(a), np.isnan(ref)), (what, "NaN pattern")
    if np.isnan(ref).all():
        return
    scale = float(np.nanmax(np.abs(ref)))
    err = float(np.nanmax(np.abs(a - ref)))
    print(f"{what}: error {err:.3e}, scale {scale:.3e}, bound {tol * scale:.3e}")
    assert err <= tol * scale, (what, err, scale)


def test_the_fixture_holds_every_case_and_stays_small(fx):
    assert os.path.getsize(NPZ) < 2 ** 20
    for name in loss_cases.CASES:
        for fn in loss_cases.FUNCTIONS:
            assert f"{name}/{fn}/loss64" in fx.files and f"{name}/{fn}/loss32" in fx.files and f"{name}/{fn}/grad64/0" in fx.files
    assert 0.5 <= float(fx["b2_48x80/mask_kept"]) <= 0.95
    d = loss_cases.inputs("b2_48x80")
    assert sorted(torch.unique(d["labels"]).tolist()) == list(range(6))
    d = loss_cases.inputs("b2_16x32_noclass")
    assert 3 not in torch.unique(d["labels"]).tolist() and bool((d["labels"][1] == 5).all())
    # the edge case separates an fp32 from a float64 evaluation of x - disp
    assert int((fx["lrsc_edges/lrsc/warped32"] != fx["lrsc_edges/lrsc/warped64"]).sum()) > 0


@pytest.mark.parametrize("name", list(loss_cases.CASES))
def test_float64_against_the_reference(fx, losses, name):
    import semstereo_amd as sa
    before = dict(sa.modules.PATH_COUNTS)
    res = loss_cases.run(losses, name, torch.float64)
    assert sa.modules.PATH_COUNTS.get("loss_torch", 0) == before.get("loss_torch", 0) + 4
    assert sa.modules.PATH_COUNTS.get("loss_hip", 0) == before.get("loss_hip", 0)
    for fn in loss_cases.FUNCTIONS:
        loss, grads = res[fn]
        _close(loss.numpy(), fx[f"{name}/{fn}/loss64"], TOL64[fn], f"{name}/{fn}/loss")
        for i, g in enumerate(grads):
            _close(g.numpy(), fx[f"{name}/{fn}/grad64/{i}"], TOL64[fn], f"{name}/{fn}/grad{i}")


@pytest.mark.parametrize("name", list(loss_cases.CASES))
def test_float32_against_the_reference(fx, losses, name):
    res = loss_cases.run(losses, name, torch.float32)
    for fn in loss_cases.FUNCTIONS:
        _close(res[fn][0].numpy(), fx[f"{name}/{fn}/loss32"], 5e-6, f"{name}/{fn}/loss32")


@pytest.mark.parametrize("name", list(loss_cases.CASES))
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_warped_labels_equal_the_reference(fx, losses, name, dtype):
    d = loss_cases.inputs(name)
    got = losses.warp_labels(d["ests"][0].to(dtype), d["labels"])
    key = "warped32" if dtype == torch.float32 else "warped64"
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), fx[f"{name}/lrsc/{key}"].astype(np.int64))
    out = torch.empty_like(d["labels"])
    losses.LRSC_loss(d["logits_r"].to(dtype), [d["ests"][0].to(dtype)], d["labels"], warped=out)
    assert torch.equal(out, got)


def test_train_objective_is_the_sum_of_the_three(fx, losses):
    name = "b2_48x80"
    d = loss_cases.inputs(name)
    f64 = lambda t: t.double()                                                # noqa: E731
    loss, dl, ll, rl = losses.train_objective([f64(e) for e in d["ests"]], f64(d["logits"]), f64(d["logits_r"]), f64(d["gt"]),
                                              f64(d["gt4"]), d["labels"], d["maxdisp"], d["attn"])
    _close(dl.numpy(), fx[f"{name}/train/loss64"], 1e-9, "train_objective/disp")
    _close(ll.numpy(), fx[f"{name}/label/loss64"], 1e-7, "train_objective/label")
    _close(rl.numpy(), fx[f"{name}/lrsc/loss64"], 1e-9, "train_objective/lrsc")
    assert float(loss) == float(dl + ll + rl) and loss.dim() == 0


def test_label_dtypes_agree(losses):
    d = loss_cases.inputs("b1_23x41")
    ref = losses.model_label_loss(d["logits"], d["labels"], 6, False)
    for dt in (torch.uint8, torch.float32, torch.int32):
        assert torch.equal(losses.model_label_loss(d["logits"], d["labels"].to(dt), 6, False), ref)


def test_the_script_regenerates_the_committed_file(tmp_path):
    from golden import make_golden_loss as mg
    if not os.path.isdir(mg.REF):
        pytest.skip("the reference is not on this machine")
    path = str(tmp_path / "loss.npz")
    mg.generate(path)
    new, old = np.load(path), np.load(NPZ)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and new[k].tobytes() == old[k].tobytes(), k
    assert open(path, "rb").read() == open(NPZ, "rb").read()
