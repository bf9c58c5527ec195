"""The joint stereo-semantic record on the HIP kernel (csrc/joint_metrics.hip): every fixture case against the reference's record
(tests/golden/joint_metrics.npz) with the bounds of tests/test_joint_metrics_golden.py, the kernel against the PyTorch composition run on
the CPU at shapes chosen by the paths they take, routing, repeatability, accumulation, no host wait, and eval_metrics_joint on a
stand-in evaluation script.  Run on the MI355X box: pytest -m gpu.

Kernel against composition: every integer table EQUAL (the CPU's division is IEEE, like the kernel's); the error sums within
n * 2^-52 relative, n the pixels of the class in the mask (two float64 sums of the same n fp32 values in different orders, each within
(n - 1) * 2^-53 of exact).

The launch gives image b at most min(1024 / B, 512) workgroups of 256 threads (GJ and GI in joint_metrics.hip); a thread takes four
pixels per trip on the 16-byte path (W % 4 == 0) and one on the scalar path.  So with B = 1 one pass of the capped grid covers
512 * 256 * 4 = 524,288 pixels on the 16-byte path and 131,072 on the scalar one: 1028 x 1024 (1,052,672 pixels, W % 4 == 0) and
1025 x 1027 (1,052,675 pixels, W odd) both ask for more than 512 workgroups, reach the cap and send every thread round the grid-stride
loop more than once -- the last trip with part of the threads only."""
import os
import types

import numpy as np
import pytest
import torch

from golden import joint_metrics_cases as jc
from test_joint_metrics_golden import check_record_against_fixture, np_rec, sums_close

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
INT_KEYS = ("image", "cls_sel", "cls_counts", "joint_all", "joint_out", "joint_good")


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return semstereo_amd


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "joint_metrics.npz"))


def cu(t):
    return None if t is None else t.cuda()


class counted:
    """The calls inside take the kernel (`hip` of them) and the composition (`torch` of them), and move no other counter."""

    def __init__(self, sa, hip, torch_=0):
        self.sa, self.hip, self.torch = sa, hip, torch_

    def __enter__(self):
        self.before = dict(self.sa.modules.PATH_COUNTS)

    def __exit__(self, *exc):
        if exc[0] is None:
            torch.cuda.synchronize()
            pc = self.sa.modules.PATH_COUNTS
            assert pc.get("joint_metrics_hip", 0) == self.before.get("joint_metrics_hip", 0) + self.hip, "joint_metrics_hip"
            assert pc.get("joint_metrics_torch", 0) == self.before.get("joint_metrics_torch", 0) + self.torch, "joint_metrics_torch"
            for k in pc:
                if not k.startswith("joint_metrics"):
                    assert pc[k] == self.before.get(k, 0), k


def same_record(got, want, what):
    """Integer tables equal, sums within n * 2^-52."""
    g, w = np_rec(got), np_rec(want)
    for k in INT_KEYS:
        assert g[k].dtype == np.int64 and np.array_equal(g[k], w[k]), (what, k, int(np.abs(g[k] - w[k]).max()))
    assert g["cls_sums"].dtype == np.float64
    sums_close(g["cls_sums"], w["cls_sums"], w["cls_sel"][None], f"{what}: cls_sums")


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(jc.CASES))
def test_fixture_cases(sa, fx, name):
    d = jc.inputs(name)
    J = sa.joint_metrics.joint_metrics
    ests, z, gt, y, mask = [cu(e) for e in d["ests"]], cu(d["logits"]), cu(d["gt"]), cu(d["labels"]), cu(d["mask"])
    with counted(sa, 1):
        rec = J(ests, z, gt, y, mask=mask, thresholds=jc.THRESHOLDS)
    assert all(v.is_cuda for v in rec.values())
    check_record_against_fixture(name, d, rec, fx)
    with counted(sa, 0, 1):
        cpu = J(d["ests"], d["logits"], d["gt"], d["labels"], mask=d["mask"], thresholds=jc.THRESHOLDS)
    same_record(rec, cpu, name)
    if d["range_form"]:
        with counted(sa, 1):
            rec2 = J(ests, z, gt, y, maxdisp=d["maxdisp"], thresholds=jc.THRESHOLDS)
        assert all(torch.equal(rec[k], rec2[k]) for k in INT_KEYS) and rec["cls_sums"].cpu().numpy().tobytes() == rec2["cls_sums"].cpu().numpy().tobytes()
    with counted(sa, 1):                                             # without logits: the same per-class record, no tables
        bare = J(ests, None, gt, y, mask=mask, thresholds=jc.THRESHOLDS)
    assert bare["joint_all"] is None and bare["joint_out"] is None and bare["joint_good"] is None
    assert all(torch.equal(bare[k], rec[k]) for k in ("image", "cls_sel", "cls_counts"))
    assert bare["cls_sums"].cpu().numpy().tobytes() == rec["cls_sums"].cpu().numpy().tobytes()


# 2 ------------------------------------------------------------------------------------------------------------------------------
def _inputs(B, H, W, nest, seed, label_dtype=torch.int64, pad=(0, 0)):
    from oracle import detdata as dd
    gt = dd.t_uniform((B, H, W), seed, -80.0, 80.0)                  # |gt| up to 80: E / |gt| > 0.05 decides for part of the pixels
    ests = [gt + 2.5 * dd.t_normalish((B, H, W), seed + 10 + i) for i in range(nest)]
    gt[:, ::9, ::5] = 0.0                                            # E / 0
    ests[0][:, 1::9, ::7] = gt[:, 1::9, ::7]                         # E = 0
    ests[0][:, 2::9, ::7] = gt[:, 2::9, ::7] + 3.0                   # E on (or next to) tau and a threshold
    ests[-1][:, 3::9, ::11] = float("nan")                           # a NaN E is neither good nor above a threshold
    logits = 2.0 * dd.t_normalish((B, 6, H, W), seed + 3)
    logits[:, 2, ::5] = logits[:, 4, ::5]                            # ties
    logits[:, 3, 4::7, ::3] = float("nan")                           # a NaN is the maximum
    labels = torch.from_numpy(np.minimum(np.floor(dd.uniform((B, H + pad[0], W + pad[1]), seed + 2, 0.0, 7.0)), 6).astype(np.int64))
    return dict(ests=ests, gt=gt, logits=logits, labels=labels.to(label_dtype))


# B, H, W, estimates, label dtype, label pad, mask form
SHAPES = [(3, 96, 200, 3, torch.float32, (0, 4), "tensor"),          # 19 workgroups per image: the finish adds several partials; labels cropped on the 16-byte path
          (3, 97, 203, 1, torch.int64, (2, 3), "range"),             # the same on the scalar path
          (1, 1028, 1024, 4, torch.int64, (0, 0), "range"),          # past one pass of the capped grid, 16-byte path (see the module's docstring)
          (1, 1025, 1027, 2, torch.uint8, (0, 0), "tensor")]         # ... and on the scalar path


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s[:4]))
def test_kernel_against_the_cpu_composition(sa, shape):
    B, H, W, nest, dt, pad, form = shape
    d = _inputs(B, H, W, nest, 11000 + H + nest, dt, pad)
    kw = dict(thresholds=jc.THRESHOLDS)
    if form == "tensor":
        mask = ((d["gt"] < 64) & (d["gt"] >= -64) & (d["gt"] != 0.0)) | (d["gt"] > 78.0)
        kw_gpu = dict(kw, mask=cu(mask))
        kw["mask"] = mask
    else:
        kw["maxdisp"] = 64
        kw_gpu = kw
    J = sa.joint_metrics.joint_metrics
    with counted(sa, 0, 1):
        want = J(d["ests"], d["logits"], d["gt"], d["labels"], **kw)
    with counted(sa, 1):
        got = J([cu(e) for e in d["ests"]], cu(d["logits"]), cu(d["gt"]), cu(d["labels"]), **kw_gpu)
    same_record(got, want, str(shape[:4]))
    w = np_rec(want)
    assert w["joint_all"].sum() == B * H * W and w["joint_out"].sum() > 0 and w["cls_sel"][:, 6].sum() > 0 and w["joint_good"].sum() > 0
    assert (w["joint_all"][None] - w["joint_out"][None] - w["joint_good"] > 0).any()         # some pixels in the mask are bad


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_routing_and_the_same_bits(sa, monkeypatch):
    d = jc.inputs("odd_23x41")
    ests, z, gt, y = [cu(e) for e in d["ests"]], cu(d["logits"]), cu(d["gt"]), cu(d["labels"])
    J = sa.joint_metrics.joint_metrics
    with counted(sa, 2):
        a = J(ests, z, gt, y, maxdisp=d["maxdisp"], thresholds=jc.THRESHOLDS)
        b = J(ests, z, gt, y, maxdisp=d["maxdisp"], thresholds=jc.THRESHOLDS)
    for k in a:                                                      # two calls: the same bits
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    monkeypatch.setattr(sa.engine, "JOINT_METRICS_HIP", False)
    with counted(sa, 0, 1):
        off = J(ests, z, gt, y, maxdisp=d["maxdisp"], thresholds=jc.THRESHOLDS)
    monkeypatch.setattr(sa.engine, "JOINT_METRICS_HIP", True)
    assert all(v.is_cuda for v in off.values())
    same_record(a, off, "switched off")
    with counted(sa, 0, 2):                                          # float64 and five channels keep the composition
        J([e.double() for e in ests], z.double(), gt.double(), y, maxdisp=d["maxdisp"])
        five = J(ests, z[:, :5].contiguous(), gt, y, maxdisp=d["maxdisp"])
    assert tuple(five["joint_all"].shape) == (2, 6, 5)
    big = _inputs(2, 64, 96, 2, 11500)
    ests, z, gt, y = [cu(e) for e in big["ests"]], cu(big["logits"]), cu(big["gt"]), cu(big["labels"])
    m, one = sa.JointMetric(5, thresholds=jc.THRESHOLDS), sa.JointMetric(5, thresholds=jc.THRESHOLDS)
    with counted(sa, 3):
        one.addBatch(ests, z, gt, y, maxdisp=64)
        m.addBatch(ests, z, gt, y, maxdisp=64)
        m.addBatch(ests, z, gt, y, maxdisp=64)
    s1, s2 = one.state(), m.state()
    for k in s1:                                                     # addBatch twice: twice the sums (doubling is exact)
        assert (2 * s1[k]).cpu().numpy().tobytes() == s2[k].cpu().numpy().tobytes(), k
    assert s1["images"].tolist() == [2, 2]


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_no_host_wait(sa):
    d = _inputs(2, 128, 160, 2, 11600)
    ests, z, gt, y = [cu(e) for e in d["ests"]], cu(d["logits"]), cu(d["gt"]), cu(d["labels"])
    metric, avg = sa.JointMetric(5), sa.EvalAverager("all")

    def step():
        rec = sa.joint_metrics.joint_metrics(ests, z, gt, y, maxdisp=64)
        metric.addBatch(ests, z, gt, y, maxdisp=64)
        s, s_img = metric.scores(), metric.scores("image")
        out = sa.eval_metrics_joint(ests, z, gt, y, 64)
        avg.update(out)
        return rec, s, s_img, out
    step()                                                           # (library load, scratch query)
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
        rec, s, s_img, out = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert sa.modules.PATH_COUNTS.get("joint_metrics_hip", 0) == before.get("joint_metrics_hip", 0) + 3
    assert sa.modules.PATH_COUNTS.get("joint_metrics_torch", 0) == before.get("joint_metrics_torch", 0)
    assert bool(torch.isfinite(s["mIoU3"]).all()) and bool(torch.isfinite(s["EPE_c"][0]).all()) and bool(torch.isfinite(out["mIoU3"][0]))
    assert int(rec["joint_all"].sum()) == 2 * 128 * 160 and avg.count == 2


# 5 ------------------------------------------------------------------------------------------------------------------------------
_SCRIPT = '''
def test_sample(disp_ests, label_est, disp_gt, label_true, maxdisp, nums=6):
    scalar_outputs3 = eval_metrics_joint(disp_ests, label_est, disp_gt, label_true, maxdisp, nums)
    disp_gt[disp_gt < -871.0] = 0
    return scalar_outputs3
'''


def test_eval_metrics_joint_on_a_stand_in_script(sa):
    script = types.ModuleType("standin_eval_script")
    script.eval_metrics_joint = sa.eval_metrics_joint
    exec(_SCRIPT, script.__dict__)
    d = jc.inputs("class_gap")
    with counted(sa, 1):
        out = script.test_sample([cu(e) for e in d["ests"]], cu(d["logits"]), cu(d["gt"]).clone(), cu(d["labels"]), d["maxdisp"])
    assert list(out) == ["mIoU3"] + [f"{k}{i}" for i in range(5) for k in ("EPE_c", "D1_c", "IoU3_")]
    assert all(isinstance(v, list) and len(v) == 2 and all(t.dim() == 0 and t.is_cuda and t.dtype == torch.float64 for t in v)
               for v in out.values())
    cpu = script.test_sample(d["ests"], d["logits"], d["gt"].clone(), d["labels"], d["maxdisp"])               # the composition
    for k in out:
        a, b = np.asarray([float(t) for t in out[k]]), np.asarray([float(t) for t in cpu[k]])
        assert np.array_equal(np.isnan(a), np.isnan(b)), k
        if k.startswith("EPE"):
            assert np.allclose(a, b, rtol=400 * 2.0 ** -52, atol=0, equal_nan=True), k         # (n * 2^-52 with the batch's 400 pixels for n)
        elif k == "mIoU3":
            assert np.allclose(a, b, rtol=1e-12, atol=0), k                                    # (the float64 mean of five equal values, in the device's order)
        else:
            assert np.array_equal(a, b, equal_nan=True), k                                     # the same integers, the same float64 division
