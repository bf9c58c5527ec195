"""CPU: the PyTorch composition of semstereo_amd.metrics (what CPU, float64 and unsupported inputs run) against tests/golden/metrics.npz,
the record of the reference's own utils/metrics.py and utils/experiment.py on the same closed-form inputs
(tests/golden/make_golden_metrics.py).

float64 inputs: every value within 1e-12 relative of the reference's float64 value (the same operations in another order over at most
a few thousand terms).  float32 inputs: the integer counts of the record equal round(per-image float32 value * n_sel) for D1 and every
threshold (exact while n_sel < 2^22); batch values within (B + 2) * 2^-24 relative of the reference's float32 value for D1 and the
thresholds (one rounding per image value, at most B in the reference's float32 mean, one at the end), EPE within 5e-7 relative (there
the reference's own float32 summation enters); NaN and 0 exactly where the reference has them.  The confusion matrix is equal after one
and after two addBatch calls, the scores are within 1e-12 with NaN in the same places, and EvalAverager returns the stored means bit
for bit."""
import os

import numpy as np
import pytest
import torch

from golden import metrics_cases as mc

HERE = os.path.dirname(os.path.abspath(__file__))
NPZ = os.path.join(HERE, "golden", "metrics.npz")


@pytest.fixture(scope="module")
def fx():
    return np.load(NPZ)


@pytest.fixture(scope="module")
def metrics():
    import semstereo_amd
    return semstereo_amd.metrics


def rel_close(a, ref, tol, what):
    """NaN in the same places, 0 exactly where the reference is 0, else |a - ref| <= tol * |ref|."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    assert np.array_equal(np.isnan(a), np.isnan(ref)), (what, "NaN pattern", a, ref)
    ok = ~np.isnan(ref)
    if not ok.any():
        return
    err = np.abs(a[ok] - ref[ok])
    print(f"{what}: largest relative error {float(np.max(err / np.maximum(np.abs(ref[ok]), 1e-300))):.3e}, bound {tol:.3e}")
    assert np.all(np.where(ref[ok] == 0, a[ok] == 0, err <= tol * np.abs(ref[ok]))), (what, a, ref)


def check_float32_values(name, d, out, rec, fx):
    """What the CPU and the GPU test ask of a float32 run: out [n_est, 5] and the record against the fixture."""
    B = d["gt"].shape[0]
    n_sel, kept = fx[f"{name}/n_sel"], mc.kept(d)
    counts = rec["counts"].cpu().numpy()
    for e in range(len(d["ests"])):
        assert np.array_equal(counts[e, :, 0], n_sel) and np.array_equal(counts[e, :, 1], fx[f"{name}/n_mask"]) \
            and np.array_equal(counts[e, :, 2], fx[f"{name}/n_pos"]), (name, e)
        for key, col in mc.COLUMN.items():
            img32 = fx[f"{name}/{key}/image32"][e]
            if key != "EPE":
                for b in range(B):
                    if kept[b] and n_sel[b] > 0 and not np.isnan(img32[b]):
                        assert n_sel[b] < 2 ** 22
                        want = int(round(float(img32[b]) * int(n_sel[b])))
                        assert int(counts[e, b, 2 + col]) == want, (name, key, e, b, int(counts[e, b, 2 + col]), want)
            tol = 5e-7 if key == "EPE" else (B + 2) * 2.0 ** -24
            rel_close(out[e, col].cpu().numpy(), fx[f"{name}/{key}/batch32"][e], tol, f"{name}/{key}/est{e}/batch32")
        sums = rec["sums"].cpu().numpy()[e]
        for b in range(B):                                           # per-image EPE from the record, where the image has one
            if kept[b] and n_sel[b] > 0:
                rel_close(sums[b] / n_sel[b], fx[f"{name}/EPE/image32"][e, b], 5e-7, f"{name}/EPE/est{e}/image{b}")


def test_the_fixture_holds_every_case_and_stays_small(fx):
    assert os.path.getsize(NPZ) < 2 ** 20
    for name in mc.CASES:
        for key in mc.COLUMN:
            for k in ("batch32", "batch64", "image32", "image64"):
                assert f"{name}/{key}/{k}" in fx.files
        assert fx[f"{name}/confusion1"].shape == (5, 5) and fx[f"{name}/scores"].shape == (13,)
    assert all(v.dtype.kind in "fiub" for v in fx.values())
    # the cases are what they are meant to be
    assert np.array_equal(mc.kept(mc.inputs("skips")), [False, True, True, True]) and fx["skips/n_pos"][1] == 0 and fx["skips/n_mask"][1] > 0
    assert np.all(fx["all_skipped/EPE/batch32"] == 0) and not mc.kept(mc.inputs("all_skipped")).any()
    assert fx["nan_image/n_pos"][1] == 0 and fx["nan_image/n_mask"][1] == 0 and np.isnan(fx["nan_image/D1/batch32"]).all()
    assert np.isnan(fx["nan_image/scores"][[3 + 3, 8 + 3]]).all() and not np.isnan(fx["nan_image/scores"][:3]).any()
    assert np.isnan(fx["edges/EPE/batch32"]).all() and fx["edges/D1/batch32"][0] != fx["edges/Thres3/batch32"][0]
    d = mc.inputs("four_ests_mask_img")
    assert d["labels"].shape[1] > d["logits"].shape[2] and d["labels"].dtype == torch.float32 and not torch.equal(d["mask"], d["mask_img"])


@pytest.mark.parametrize("name", list(mc.CASES))
def test_float64_against_the_reference(fx, metrics, name):
    import semstereo_amd as sa
    before = dict(sa.modules.PATH_COUNTS)
    d = mc.inputs(name)
    res = mc.run_disparity(metrics, d, torch.float64)
    assert sa.modules.PATH_COUNTS.get("metrics_torch", 0) > before.get("metrics_torch", 0)
    assert sa.modules.PATH_COUNTS.get("metrics_hip", 0) == before.get("metrics_hip", 0)
    for key, (batch, images) in res.items():
        rel_close(batch, fx[f"{name}/{key}/batch64"], 1e-12, f"{name}/{key}/batch64")
        rel_close(images, fx[f"{name}/{key}/image64"], 1e-12, f"{name}/{key}/image64")
    one = metrics.EPE_metric(d["ests"][0].double(), d["gt"].double(), d["mask"])
    assert one.dim() == 0 and one.dtype == torch.float64 and not one.requires_grad


@pytest.mark.parametrize("name", list(mc.CASES))
def test_float32_against_the_reference(fx, metrics, name):
    d = mc.inputs(name)
    out, rec = metrics.disparity_metrics(d["ests"], d["gt"], mask=d["mask"], thresholds=mc.THRESHOLDS, mask_img=d["mask_img"],
                                         return_record=True)
    assert out.dtype == torch.float32 and tuple(out.shape) == (len(d["ests"]), 5)
    check_float32_values(name, d, out, rec, fx)
    res = mc.run_disparity(metrics, d, torch.float32)                # the six names give the same values, one at a time
    for key, col in mc.COLUMN.items():
        assert np.array_equal(np.asarray(res[key][0], dtype=np.float32), out[:, col].numpy(), equal_nan=True), (name, key)
    if d["range_form"]:                                              # the range evaluated inside is the mask tensor
        out2, rec2 = metrics.disparity_metrics(d["ests"], d["gt"], maxdisp=d["maxdisp"], thresholds=mc.THRESHOLDS, mask_img=d["mask_img"],
                                               return_record=True)
        assert torch.equal(out2, out) and torch.equal(rec2["counts"], rec["counts"]) and torch.equal(rec2["sums"], rec["sums"])


def check_scores(name, m, fx):
    want = fx[f"{name}/scores"]
    got = np.concatenate([[m.pixelAccuracy(), m.meanPixelAccuracy(), m.meanIntersectionOverUnion()], m.classPixelAccuracy(), m.IoU()])
    rel_close(got, want, 1e-12, f"{name}/scores (host)")
    s = m.scores()
    assert all(v.dtype == torch.float64 and v.device == m._joint.device for v in s.values())
    dev = np.concatenate([[float(s["PA"]), float(s["MPA"]), float(s["mIoU"])], s["CPA"].cpu().numpy(), s["IoU"].cpu().numpy()])
    rel_close(dev, want, 1e-12, f"{name}/scores (device tensors)")


@pytest.mark.parametrize("name", list(mc.CASES))
def test_confusion_matrix_equals_the_reference(fx, metrics, name):
    d = mc.inputs(name)
    m = metrics.SegmentationMetric(5)
    assert m.confusionMatrix.shape == (5, 5) and not m.confusionMatrix.any()
    m.addBatch(d["logits"], d["labels"])
    first = m.confusionMatrix
    assert first.dtype == np.float64 and np.array_equal(first, fx[f"{name}/confusion1"]) and m.confusionMatrix is first
    assert np.array_equal(m.get_confusion_matrix(d["labels"], d["logits"], num_class=5), fx[f"{name}/confusion1"])
    m.addBatch(d["logits2"], d["labels2"])
    assert np.array_equal(m.confusionMatrix, fx[f"{name}/confusion2"])
    check_scores(name, m, fx)
    joint = m.jointMatrix
    assert joint.shape == (7, 6) and joint.dtype == np.int64 and joint.sum() == 2 * d["logits"][:, 0].numel()
    honest = metrics.SegmentationMetric(5, fold=False)
    honest.addBatch(d["logits"], d["labels"])
    honest.addBatch(d["logits2"], d["labels2"])
    assert np.array_equal(honest.confusionMatrix, joint[:5, :5].astype(np.float64))
    assert np.array_equal(honest.device_matrix().numpy(), honest.confusionMatrix)
    if joint[:, 5].any():
        assert not np.array_equal(honest.confusionMatrix, m.confusionMatrix)          # the fold is not the honest block
    m.reset()
    assert not m.confusionMatrix.any() and not m.jointMatrix.any()
    m.addBatch(d["logits"], d["labels"])
    assert np.array_equal(m.confusionMatrix, fx[f"{name}/confusion1"])


def test_label_dtypes_and_stray_labels(metrics):
    d = mc.inputs("plain_b4")
    ref = metrics._joint_torch(d["logits"], d["labels"])
    for dt in (torch.uint8, torch.float32, torch.int32):
        assert torch.equal(metrics._joint_torch(d["logits"], d["labels"].to(dt)), ref), dt
    stray = d["labels"].clone()
    stray[0, 0, :7] = torch.tensor([-1, 6, 255, -2 ** 40, 2 ** 40, 7, -100])
    j = metrics._joint_torch(d["logits"], stray)
    assert int(j[6].sum()) == 7 and int(j.sum()) == stray.numel()


@pytest.mark.parametrize("mode", ["all", "valid"])
def test_eval_averager_bit_for_bit(fx, metrics, mode):
    seq = mc.avg_sequence()
    avg = metrics.EvalAverager(mode)
    for row in seq:
        avg.update({k: [torch.tensor(v, dtype=torch.float32)] for k, v in zip(mc.AVG_KEYS, row)})
    mean = avg.mean()
    if mode == "all":
        got = np.asarray([mean[k][0] for k in mc.AVG_KEYS], dtype=np.float64)
        assert got.tobytes() == fx["avg/all"].tobytes(), (got, fx["avg/all"])
    else:
        present = fx["avg/valid_present"]
        assert [k in mean for k in mc.AVG_KEYS] == list(present)
        got = np.asarray([mean.get(k, np.nan) for k in mc.AVG_KEYS], dtype=np.float64)
        assert got.tobytes() == fx["avg/valid"].tobytes(), (got, fx["avg/valid"])


def test_eval_metrics_keys_and_values(fx, metrics):
    d = mc.inputs("odd_23x41")
    out, out2 = metrics.eval_metrics(d["ests"], d["logits"], d["gt"], d["labels"], d["maxdisp"])
    assert list(out) == ["D1", "EPE", "Thres1", "Thres2", "PA", "MPA", "mIoU"]
    assert list(out2) == [f"{k}{i}" for i in range(5) for k in ("CPA", "IoU")]
    assert all(isinstance(v, list) and all(t.dim() == 0 for t in v) for v in list(out.values()) + list(out2.values()))
    for key in ("D1", "EPE", "Thres1", "Thres2"):
        assert len(out[key]) == 2
        tol = 5e-7 if key == "EPE" else 4 * 2.0 ** -24
        rel_close([float(t) for t in out[key]], fx[f"odd_23x41/{key}/batch32"], tol, key)
    m = metrics.SegmentationMetric(5)
    m.addBatch(d["logits"], d["labels"])
    assert float(out["mIoU"][0]) == pytest.approx(m.meanIntersectionOverUnion(), rel=1e-12)
    assert float(out2["IoU3"][0]) == pytest.approx(m.IoU()[3], rel=1e-12)


def test_the_script_regenerates_the_committed_file(tmp_path):
    from golden import make_golden_metrics as mg
    if not os.path.isdir(mg.REF):
        pytest.skip("the reference is not on this machine")
    path = str(tmp_path / "metrics.npz")
    mg.generate(path)
    new, old = np.load(path), np.load(NPZ)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and new[k].tobytes() == old[k].tobytes(), k
    assert open(path, "rb").read() == open(NPZ, "rb").read()
