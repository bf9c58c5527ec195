"""CPU: the PyTorch composition of semstereo_amd.data against the reference's record (tests/golden/data.npz, written by
tests/golden/make_golden_data.py from the reference's own Us3dDataset / WhuDataset), the key sets of prepare_sample, RawStereoDataset on
files and DeviceLoader on the CPU device (no GPU needed).

Criteria: views, pyramid levels, `disparity` and `label` are torch.equal -- table lookups, copies and exact widenings.  gx / gy are within
1 float32 ulp with NaN in the same places: the module's standard deviation is the exact-integer form, numpy's np.std the centred one, an
ulp of double apart at the most, which can move a float32 rounding by one step.  The count of unequal pixels is in the assertion
message."""
import os

import numpy as np
import pytest
import torch

from golden import data_cases as dc

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "data.npz"))


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    return semstereo_amd


def check_case(sample, fx, name):
    """`sample`: prepare_sample's dictionary for the case, any device."""
    c = dc.CASES[name]
    for k in dc.VIEW_KEYS + dc.level_keys(name):
        want = torch.from_numpy(fx[f"closed/{name}/{k}"])
        got = sample[k].cpu()
        assert got.dtype == torch.float32 and torch.equal(got, want), f"{name} {k}: {(got != want).sum().item()} values differ"
    for k in ("disparity",) + (("label",) if c["kind"] == "us3d" else ()):
        want = torch.from_numpy(fx[f"ref/{name}/{k}"])
        got = sample[k].cpu()
        assert got.dtype == torch.float32 and torch.equal(got, want), f"{name} {k}"
    for k in dc.GRAD_KEYS:
        want = torch.from_numpy(fx[f"ref/{name}/{k}"])
        dc.assert_gradients(sample[k], want, f"{name} {k}")
        assert bool(torch.isnan(want).all()) == (name == dc.NAN_CASE)


@pytest.mark.parametrize("name", list(dc.CASES))
def test_composition_equals_the_reference(sa, fx, name):
    raw = dc.raw_inputs(name)
    before = dict(sa.modules.PATH_COUNTS)
    training = dc.has_training_branch(name)
    sample = sa.prepare_sample(raw, training)
    names = sa.data.KEYS[(dc.CASES[name]["kind"], training)]
    assert tuple(sample) == tuple(k for k in names if k != "left_filename")          # (the raw arrays carry no file name)
    check_case(sample, fx, name)
    pc = sa.modules.PATH_COUNTS
    assert pc.get("data_torch", 0) == before.get("data_torch", 0) + 3 and pc.get("data_hip", 0) == before.get("data_hip", 0)
    assert pc["torch"] == before["torch"] and pc["hip"] == before["hip"]
    # the three calls on their own give the same tensors
    left, right = sa.normalize_views(raw["left_u8"], raw["right_u8"])
    gx, gy = sa.image_gradients(raw["left_u8"])
    assert torch.equal(left, sample["left"]) and torch.equal(right, sample["right"]) and torch.equal(sa.normalize_views(raw["right_u8"]), right)
    assert torch.equal(gx.view(torch.int32), sample["gx"].view(torch.int32)) and torch.equal(gy.view(torch.int32), sample["gy"].view(torch.int32))
    one = sa.normalize_views(raw["left_u8"][0])                         # an item without the batch dimension
    assert one.shape == left.shape[1:] and torch.equal(one, left[0])


def test_table_is_the_stated_arithmetic(sa):
    t = sa.data.view_table()
    assert t.shape == (3, 256) and t.dtype == torch.float32
    u = torch.arange(256, dtype=torch.float32)
    for c in range(3):
        want = (u / 255 - torch.tensor(sa.data.MEAN[c], dtype=torch.float32)) / torch.tensor(sa.data.STD[c], dtype=torch.float32)
        assert torch.equal(t[c], want)


def test_key_sets_per_branch_and_kind(sa):
    us, wh = dc.raw_inputs("random_32x48"), dc.raw_inputs("whu_16x48")
    assert set(sa.prepare_sample(us, True)) == {"left", "right", "disparity", "disparity_4", "disparity_8", "disparity_16", "label",
                                                "label_2", "label_4", "gx", "gy"}
    assert set(sa.prepare_sample(wh, True)) == {"left", "right", "disparity", "disparity_4", "disparity_8", "disparity_16", "gx", "gy"}
    # the test branch: no pyramids; the pads default to 0, the file name is there where the raw item has one
    assert set(sa.prepare_sample(us, False)) == {"left", "right", "disparity", "label", "top_pad", "right_pad", "gx", "gy"}
    t = sa.prepare_sample(dict(wh, left_filename=["a.tif"], top_pad=torch.tensor([3]), right_pad=torch.tensor([0])), False)
    assert set(t) == {"left", "right", "disparity", "top_pad", "right_pad", "left_filename", "gx", "gy"}
    assert t["left_filename"] == ["a.tif"] and int(t["top_pad"][0]) == 3
    assert sa.prepare_sample(us, False)["top_pad"] == 0


def test_keys_select_a_subset_and_nothing_else_is_computed(sa, fx):
    raw = dc.raw_inputs("random_32x48")
    full = sa.prepare_sample(raw, True)
    before = sa.modules.PATH_COUNTS.get("data_torch", 0)
    keys = ("left", "right", "disparity", "disparity_4", "label")       # what a training script reads
    sub = sa.prepare_sample(raw, True, keys=keys)
    assert tuple(sub) == keys and sa.modules.PATH_COUNTS["data_torch"] == before + 2         # views and pyramid: no gradients
    for k in keys:
        assert torch.equal(sub[k], full[k]), k
    assert sub["disparity"] is raw["disparity"]                         # a float32 disparity passes through
    only = sa.prepare_sample(raw, True, keys=("gx",))
    assert tuple(only) == ("gx",) and sa.modules.PATH_COUNTS["data_torch"] == before + 3
    assert tuple(sa.prepare_sample(raw, False, keys=keys + ("top_pad",))) == ("left", "right", "disparity", "label", "top_pad")
    with pytest.raises(AssertionError):
        sa.prepare_sample(raw, True, keys=("left", "lable"))


def test_pyramid_forms(sa):
    raw = dc.raw_inputs("whu_16x48")
    p = sa.nearest_pyramid(raw["disparity"], disp_scale=1 / 256)
    assert p["disparity"].dtype == torch.float32 and torch.equal(p["disparity"], raw["disparity"].float() / 256)
    for k in (4, 8, 16):
        assert torch.equal(p[f"disparity_{k}"], p["disparity"][:, ::k, ::k])
    us = dc.raw_inputs("odd_37x53")                                     # sizes the factor does not divide: the stated formula
    q = sa.nearest_pyramid(us["disparity"], us["label"])
    assert q["disparity_4"].shape == (1, 9, 13) and q["label_2"].shape == (1, 18, 26) and q["disparity_16"].shape == (1, 2, 3)
    ys = sa.data.nearest_index(9, 37, "cpu")
    assert ys.tolist() == [min(int(np.floor(d * (1.0 / (9.0 / 37.0)))), 36) for d in range(9)]
    assert torch.equal(q["disparity_4"], us["disparity"][:, ys][:, :, sa.data.nearest_index(13, 53, "cpu")])
    one = sa.nearest_pyramid(us["disparity"][0], us["label"][0], disp_levels=(4,), label_levels=())
    assert set(one) == {"disparity", "disparity_4", "label"} and one["disparity_4"].shape == (9, 13)


@pytest.mark.parametrize("name", ["random_32x48", "batch_2x16x32", "whu_16x48"])
def test_raw_dataset_returns_the_arrays_the_files_were_written_from(sa, tmp_path, name):
    pytest.importorskip("PIL")
    c, raw = dc.CASES[name], dc.raw_inputs(name)
    lst = dc.write_case(name, str(tmp_path))
    for training in (True, False):
        ds = sa.RawStereoDataset(str(tmp_path), lst, training, kind=c["kind"])
        assert len(ds) == c["B"] and ds.training == training
        for i in range(c["B"]):
            item = ds[i]
            want = {"left_u8", "right_u8", "disparity"} | ({"label"} if c["kind"] == "us3d" else set())
            assert set(item) == want | (set() if training else {"top_pad", "right_pad", "left_filename"})
            for k in want:
                assert item[k].dtype == raw[k].dtype and torch.equal(item[k], raw[k][i]), (name, k)
            if not training:
                assert item["top_pad"] == 0 and item["right_pad"] == 0 and item["left_filename"] == f"{name}_{i}_left.tif"


@pytest.mark.parametrize("training", [True, False])
def test_device_loader_on_the_cpu_equals_prepare_sample(sa, fx, tmp_path, training):
    pytest.importorskip("PIL")
    name = "batch_2x16x32"
    lst = dc.write_case(name, str(tmp_path))
    ds = sa.RawStereoDataset(str(tmp_path), lst, training)
    loader = torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False, num_workers=0)
    dl = sa.DeviceLoader(loader, device="cpu")
    assert len(dl) == 2 and dl.training == training
    raws, got = list(loader), list(dl)
    assert len(got) == 2
    for raw, sample in zip(raws, got):
        want = sa.prepare_sample(raw, training)
        assert list(sample) == list(want)
        for k, v in want.items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(sample[k].view(torch.int32) if v.dtype == torch.float32 else sample[k],
                                   v.view(torch.int32) if v.dtype == torch.float32 else v), k
            else:
                assert sample[k] == v, k
    both = sa.DeviceLoader(torch.utils.data.DataLoader(ds, batch_size=2), device="cpu", keys=("left", "gx", "disparity"))
    (sample,) = list(both)
    assert tuple(sample) == ("left", "disparity", "gx")
    check = dict(sa.prepare_sample(next(iter(torch.utils.data.DataLoader(ds, batch_size=2))), training))
    if training:
        check_case(check, fx, name)
    assert torch.equal(sample["left"], check["left"])
