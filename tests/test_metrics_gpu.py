"""The evaluation metrics on the HIP kernels (csrc/metrics.hip; reference utils/metrics.py, main_us3d.py:225-263): every fixture case
against the reference's record (tests/golden/metrics.npz), full-size inputs against the PyTorch composition run on the CPU, label
dtypes, routing, repeatability, accumulation, no host wait, and install_metrics on a stand-in evaluation script.
Run on the MI355X box: pytest -m gpu.

Bounds (see tests/test_metrics_golden.py for the CPU side of the same): the integer counts of the record equal
round(per-image float32 value of the fixture * n_sel); D1 and the thresholds within (B + 2) * 2^-24 relative of the float32 fixture; EPE
within 5e-7 relative of the float32 AND of the float64 fixture (each E carries one fp32 rounding, the sums are in double, one rounding
at the end); the confusion matrix equal.  At full size the record counts and the joint matrix are EQUAL to those of the composition on
the CPU in float32 (the CPU's division is IEEE), EPE within 5e-7 relative of the composition in float64."""
import os
import types

import numpy as np
import pytest
import torch

from golden import metrics_cases as mc
from test_metrics_golden import check_float32_values, check_scores, rel_close

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return semstereo_amd


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "metrics.npz"))


def cu(t):
    return None if t is None else t.cuda()


class counted:
    """The calls inside take the kernels (`hip` of them) and the composition (`torch` of them)."""

    def __init__(self, sa, hip, torch_=0):
        self.sa, self.hip, self.torch = sa, hip, torch_

    def __enter__(self):
        self.before = dict(self.sa.modules.PATH_COUNTS)

    def __exit__(self, *exc):
        if exc[0] is None:
            torch.cuda.synchronize()
            pc = self.sa.modules.PATH_COUNTS
            assert pc.get("metrics_hip", 0) == self.before.get("metrics_hip", 0) + self.hip, "metrics_hip"
            assert pc.get("metrics_torch", 0) == self.before.get("metrics_torch", 0) + self.torch, "metrics_torch"


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(mc.CASES))
def test_fixture_cases_disparity(sa, fx, name):
    d = mc.inputs(name)
    ests = [cu(e) for e in d["ests"]]
    with counted(sa, 1):
        out, rec = sa.metrics.disparity_metrics(ests, cu(d["gt"]), mask=cu(d["mask"]), thresholds=mc.THRESHOLDS, mask_img=cu(d["mask_img"]),
                                                return_record=True)
    assert out.is_cuda and out.dtype == torch.float32 and rec["counts"].dtype == torch.int64 and rec["sums"].dtype == torch.float64
    check_float32_values(name, d, out, rec, fx)
    for e in range(len(ests)):                                       # EPE also against the float64 record
        rel_close(out[e, 0].cpu().numpy(), fx[f"{name}/EPE/batch64"][e], 5e-7, f"{name}/EPE/est{e}/batch64")
    if d["range_form"]:
        with counted(sa, 1):
            out2, rec2 = sa.metrics.disparity_metrics(ests, cu(d["gt"]), maxdisp=d["maxdisp"], thresholds=mc.THRESHOLDS,
                                                      mask_img=cu(d["mask_img"]), return_record=True)
        assert torch.equal(out2, out) and torch.equal(rec2["counts"], rec["counts"]) and torch.equal(rec2["sums"], rec["sums"])
    with counted(sa, 5 * len(ests) * (1 + d["gt"].shape[0])):        # the six names, batch and image by image
        res = mc.run_disparity(sa.metrics, d, torch.float32, "cuda")
    for key, col in mc.COLUMN.items():
        assert np.array_equal(np.asarray(res[key][0], dtype=np.float32), out[:, col].cpu().numpy(), equal_nan=True), (name, key)
        tol = 5e-7 if key == "EPE" else 3 * 2.0 ** -24
        rel_close(res[key][1], fx[f"{name}/{key}/image32"], tol, f"{name}/{key}/image32")


@pytest.mark.parametrize("name", list(mc.CASES))
def test_fixture_cases_confusion(sa, fx, name):
    d = mc.inputs(name)
    m = sa.SegmentationMetric(5)
    with counted(sa, 2):
        m.addBatch(cu(d["logits"]), cu(d["labels"]))
        assert np.array_equal(m.confusionMatrix, fx[f"{name}/confusion1"])
        m.addBatch(cu(d["logits2"]), cu(d["labels2"]))
    assert np.array_equal(m.confusionMatrix, fx[f"{name}/confusion2"])
    check_scores(name, m, fx)
    cpu = sa.SegmentationMetric(5)
    cpu.addBatch(d["logits"], d["labels"])
    cpu.addBatch(d["logits2"], d["labels2"])
    assert np.array_equal(m.jointMatrix, cpu.jointMatrix)
    with counted(sa, 1):
        assert np.array_equal(m.get_confusion_matrix(cu(d["labels"]), cu(d["logits"]), num_class=5), fx[f"{name}/confusion1"])


# 2 ------------------------------------------------------------------------------------------------------------------------------
def _full_inputs(B, H, W, nest, seed, label_dtype=torch.int64, pad=(0, 0)):
    from oracle import detdata as dd
    gt = dd.t_uniform((B, H, W), seed, -80.0, 80.0)                  # |gt| up to 80: E / |gt| > 0.05 decides for part of the pixels
    ests = [gt + 2.5 * dd.t_normalish((B, H, W), seed + 10 + i) for i in range(nest)]
    gt[:, ::9, ::5] = 0.0                                            # E / 0
    ests[0][:, 1::9, ::7] = gt[:, 1::9, ::7]                         # E = 0
    ests[0][:, 2::9, ::7] = gt[:, 2::9, ::7] + 3.0                   # E on (or next to) a threshold
    logits = 2.0 * dd.t_normalish((B, 6, H, W), seed + 3)
    logits[:, 2, ::5] = logits[:, 4, ::5]                            # ties
    labels = torch.from_numpy(np.minimum(np.floor(dd.uniform((B, H + pad[0], W + pad[1]), seed + 2, 0.0, 7.0)), 6).astype(np.int64))
    return dict(ests=ests, gt=gt, logits=logits, labels=labels.to(label_dtype))


FULL = [(4, 1024, 1024, 1, "range"), (4, 1024, 1024, 4, "range"), (4, 1024, 1024, 1, "tensor"), (4, 1024, 1024, 4, "tensor"),
        (1, 2048, 2048, 1, "range"), (2, 150, 137, 2, "tensor"), (3, 75, 201, 3, "range")]


@pytest.mark.parametrize("shape", FULL, ids=lambda s: "x".join(str(v) for v in s))
def test_full_size_disparity_against_the_cpu_composition(sa, shape):
    B, H, W, nest, form = shape
    d = _full_inputs(B, H, W, nest, 9800 + H + nest)
    mask = mc.range_mask(d["gt"], 64)
    mask_img = None
    if form == "tensor":
        mask = mask & (d["gt"] != 0.0) | (d["gt"] > 78.0)
        mask_img = mask & (d["ests"][0] > -60.0) if nest == 4 else None
    ratio = mc.skip_ratio(mask, d["gt"])
    assert all(r > 0.2 for r in ratio), ratio
    kw = dict(thresholds=mc.THRESHOLDS, return_record=True, mask_img=mask_img)
    kw.update(dict(maxdisp=64) if form == "range" else dict(mask=mask))
    with counted(sa, 0, 2):
        o32, r32 = sa.metrics.disparity_metrics(d["ests"], d["gt"], **kw)
        o64, r64 = sa.metrics.disparity_metrics([e.double() for e in d["ests"]], d["gt"].double(), **kw)
    kw_gpu = dict(kw, mask_img=cu(mask_img))
    if form == "tensor":
        kw_gpu["mask"] = cu(mask)
    with counted(sa, 1):
        out, rec = sa.metrics.disparity_metrics([cu(e) for e in d["ests"]], cu(d["gt"]), **kw_gpu)
    diff = (rec["counts"].cpu() != r32["counts"])
    print(f"{shape}: record counts that differ from the CPU composition: {int(diff.sum())} of {diff.numel()}")
    assert torch.equal(rec["counts"].cpu(), r32["counts"]), (rec["counts"].cpu() - r32["counts"]).abs().max()
    rel_close(out[:, 0].cpu().numpy(), o64[:, 0].numpy(), 5e-7, f"{shape} EPE against float64")
    rel_close(rec["sums"].cpu().numpy(), r64["sums"].numpy(), 5e-7, f"{shape} sums against float64")
    rel_close(out[:, 1:].cpu().numpy(), o32[:, 1:].numpy(), (B + 2) * 2.0 ** -24, f"{shape} D1 / Thres against the composition")


@pytest.mark.parametrize("shape", [(4, 1024, 1024, torch.int64, (0, 0)), (1, 2048, 2048, torch.uint8, (0, 0)),
                                   (2, 512, 640, torch.float32, (7, 12)), (2, 150, 137, torch.int64, (0, 0)),
                                   (3, 75, 201, torch.uint8, (2, 3))], ids=lambda s: "x".join(str(v) for v in s[:3]))
def test_full_size_joint_matrix_against_the_cpu_composition(sa, shape):
    B, H, W, dt, pad = shape
    d = _full_inputs(B, H, W, 1, 9900 + H, dt, pad)
    want = sa.metrics._joint_torch(d["logits"], d["labels"])
    m = sa.SegmentationMetric(5)
    with counted(sa, 1):
        m.addBatch(cu(d["logits"]), cu(d["labels"]))
    assert np.array_equal(m.jointMatrix, want.numpy())
    assert m.jointMatrix[6].sum() > 0 and m.jointMatrix.sum() == B * H * W
    assert np.array_equal(m.confusionMatrix, sa.metrics.fold_joint(want.numpy(), 5))


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_label_dtypes_and_stray_labels(sa):
    d = mc.inputs("plain_b4")
    z = cu(d["logits"])

    def joint(labels):
        m = sa.SegmentationMetric(5)
        m.addBatch(z, cu(labels))
        return m.jointMatrix
    with counted(sa, 4):
        ref = joint(d["labels"])
        for dt in (torch.uint8, torch.float32, torch.int32):
            assert np.array_equal(joint(d["labels"].to(dt)), ref), dt
    stray = d["labels"].clone()
    stray[0, 0, :7] = torch.tensor([-1, 6, 255, -2 ** 40, 2 ** 40, 7, -100])
    base = d["labels"].clone()
    base[0, 0, :7] = 0
    a, b = joint(stray), joint(base)
    assert a[6].sum() == 7 and b[6].sum() == 0 and np.array_equal(a[:6].sum(0) + a[6], b.sum(0))
    assert np.array_equal(a, sa.metrics._joint_torch(d["logits"], stray).numpy())
    f = d["labels"].float()
    f[0, 1, :6] = torch.tensor([float("nan"), -0.5, 5.99, 6.0, -1.0, float("inf")])
    assert np.array_equal(joint(f), sa.metrics._joint_torch(d["logits"], f).numpy())


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_routing(sa, monkeypatch):
    d = mc.inputs("odd_23x41")
    ests, gt, mask, z, y = [cu(e) for e in d["ests"]], cu(d["gt"]), cu(d["mask"]), cu(d["logits"]), cu(d["labels"])
    with counted(sa, 2):
        on = sa.eval_metrics(ests, z, gt, y, d["maxdisp"])
    monkeypatch.setattr(sa.engine, "METRICS_HIP", False)
    with counted(sa, 0, 2):
        off = sa.eval_metrics(ests, z, gt, y, d["maxdisp"])
    monkeypatch.setattr(sa.engine, "METRICS_HIP", True)
    for a, b in zip(on, off):
        for k in a:
            assert all(t.is_cuda for t in a[k] + b[k])
            tol = 5e-7 if k == "EPE" else (4 * 2.0 ** -24 if k in ("D1", "Thres1", "Thres2") else 1e-12)
            rel_close([float(t) for t in a[k]], [float(t) for t in b[k]], tol, f"switched off/{k}")
    with counted(sa, 0, 3):                                          # float64 and five channels keep the composition
        sa.metrics.EPE_metric(ests[0].double(), gt.double(), mask)
        sa.SegmentationMetric(4).addBatch(z[:, :5].contiguous(), y.clamp(max=4))
        sa.metrics.disparity_metrics(ests, gt, mask=mask, thresholds=(0.5, 1.0, 2.0, 3.0, 4.0))       # more thresholds than the kernel takes
    before = dict(sa.modules.PATH_COUNTS)
    sa.metrics.D1_metric(ests[0], gt, mask)
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"] and sa.modules.PATH_COUNTS["hip"] == before["hip"]


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_accumulate_adds(sa):
    d = [_full_inputs(2, 512, 640, 2, 10000 + i) for i in range(3)]
    ests, gt = [cu(e) for e in d[0]["ests"]], cu(d[0]["gt"])
    a = sa.metrics.disparity_metrics(ests, gt, maxdisp=64, thresholds=mc.THRESHOLDS, return_record=True)
    b = sa.metrics.disparity_metrics(ests, gt, maxdisp=64, thresholds=mc.THRESHOLDS, return_record=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1]["counts"], b[1]["counts"]) and torch.equal(a[1]["sums"], b[1]["sums"])
    total, singles = sa.SegmentationMetric(5), []
    for x in d:
        total.addBatch(cu(x["logits"]), cu(x["labels"]))
        one = sa.SegmentationMetric(5)
        one.addBatch(cu(x["logits"]), cu(x["labels"]))
        singles.append(one.jointMatrix)
        again = sa.SegmentationMetric(5)
        again.addBatch(cu(x["logits"]), cu(x["labels"]))
        assert np.array_equal(again.jointMatrix, singles[-1])
    assert np.array_equal(total.jointMatrix, sum(singles)) and total.jointMatrix.sum() == 3 * 2 * 512 * 640


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_no_host_wait(sa):
    d = _full_inputs(2, 256, 320, 2, 10100)
    ests, gt, z, y = [cu(e) for e in d["ests"]], cu(d["gt"]), cu(d["logits"]), cu(d["labels"])
    metric, avg, avg2 = sa.SegmentationMetric(5), sa.EvalAverager("all"), sa.EvalAverager("valid")

    def step():
        out, out2 = sa.eval_metrics(ests, z, gt, y, 64)
        metric.addBatch(z, y)
        s = metric.scores()
        avg.update(out)
        avg2.update(out2)
        return out, out2, s
    step()                                                           # (library load, workspace query)
    torch.cuda.synchronize()
    before = dict(sa.modules.PATH_COUNTS)
    torch.cuda.set_sync_debug_mode("error")
    try:
        raised = False
        try:
            gt.sum().item()
        except RuntimeError:
            raised = True
        if not raised:
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this build")
        out, out2, s = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert sa.modules.PATH_COUNTS.get("metrics_hip", 0) == before.get("metrics_hip", 0) + 3
    assert sa.modules.PATH_COUNTS.get("metrics_torch", 0) == before.get("metrics_torch", 0)
    assert bool(torch.isfinite(out["EPE"][0])) and bool(torch.isfinite(s["mIoU"]))
    mean, mean2 = avg.mean(), avg2.mean()
    assert mean["EPE"][1] == float(out["EPE"][1]) and avg.count == 2 and mean2["IoU0"] == float(out2["IoU0"][0])


# 7 ------------------------------------------------------------------------------------------------------------------------------
_SCRIPT = '''
def test_sample(disp_ests, label_est, disp_gt, label_true, maxdisp, nums=6):
    metric = SegmentationMetric(nums - 1)
    mask = (disp_gt < maxdisp) & (disp_gt >= -maxdisp)
    metric.addBatch(label_est, label_true)
    disp_gt[disp_gt < -871.0] = 0
    scalar_outputs, scalar_outputs2 = {}, {}
    scalar_outputs["D1"] = [D1_metric(disp_est, disp_gt, mask) for disp_est in disp_ests]
    scalar_outputs["EPE"] = [EPE_metric(disp_est, disp_gt, mask) for disp_est in disp_ests]
    scalar_outputs["Thres1"] = [Thres_metric(disp_est, disp_gt, mask, 1.0) for disp_est in disp_ests]
    scalar_outputs["Thres2"] = [Thres_metric(disp_est, disp_gt, mask, 2.0) for disp_est in disp_ests]
    scalar_outputs["PA"] = [metric.pixelAccuracy()]
    scalar_outputs["MPA"] = [metric.meanPixelAccuracy()]
    scalar_outputs["mIoU"] = [metric.meanIntersectionOverUnion()]
    for i in range(nums - 1):
        scalar_outputs2["CPA" + str(i)] = [metric.classPixelAccuracy()[i]]
        scalar_outputs2["IoU" + str(i)] = [metric.IoU()[i]]
    return scalar_outputs, scalar_outputs2
'''


def test_install_metrics_on_a_stand_in_script(sa, fx):
    script = types.ModuleType("standin_eval_script")
    exec(_SCRIPT, script.__dict__)
    previous = sa.install_metrics(script)
    try:
        for name in ("odd_23x41", "plain_b4"):
            d = mc.inputs(name)
            n = len(d["ests"])
            with counted(sa, 1 + 4 * n):
                out, out2 = script.test_sample([cu(e) for e in d["ests"]], cu(d["logits"]), cu(d["gt"]).clone(), cu(d["labels"]), d["maxdisp"])
            cpu, cpu2 = script.test_sample(d["ests"], d["logits"], d["gt"].clone(), d["labels"], d["maxdisp"])       # the composition
            B = d["gt"].shape[0]
            for key in ("D1", "EPE", "Thres1", "Thres2"):
                tol = 5e-7 if key == "EPE" else (B + 2) * 2.0 ** -24
                rel_close([float(t) for t in out[key]], fx[f"{name}/{key}/batch32"], tol, f"{name}/{key} against the fixture")
                rel_close([float(t) for t in out[key]], [float(t) for t in cpu[key]], tol, f"{name}/{key} against the composition")
            for a, b in ((out, cpu), (out2, cpu2)):
                for key in b:
                    if key not in ("D1", "EPE", "Thres1", "Thres2"):
                        assert a[key] == b[key], key                 # the same integers, the same float64 arithmetic
            both, both2 = sa.eval_metrics([cu(e) for e in d["ests"]], cu(d["logits"]), cu(d["gt"]), cu(d["labels"]), d["maxdisp"])
            for key in out:
                rel_close([float(t) for t in both[key]], [float(t) for t in out[key]], 1e-12, f"{name}/{key} eval_metrics")
            for key in out2:
                rel_close([float(t) for t in both2[key]], [float(t) for t in out2[key]], 1e-12, f"{name}/{key} eval_metrics")
    finally:
        sa.uninstall(script, previous)
    assert not hasattr(script, "EPE_metric")
