"""Every kernel call of the training step against float64 on its own inputs (tests/train_calls.py), at the size and batch the training
rate is measured at: 1024 x 1024, maxdisp 64 (main_us3d.py:54), batch 1 and batch 4 (main_us3d.py:74).  The small-shape tests of
tests/test_parity_gpu.py hold each function to its bound at toy sizes; here the same bounds hold for the grid decompositions that only
the full-size shapes reach (the cooperative weight gradient's row segments, the shared-gout stride-2 chunks, BatchNorm's multi-block
reduction, the scatter kernels' batch axis).  Report: train_calls.report_path() (SS_TEST_REPORT_DIR)."""
import pytest
import torch
import torch.nn.functional as F

import train_calls as TC
from golden import cases
from oracle import detdata as dd
from oracle import hot_segment as oseg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    return semstereo_amd


@pytest.fixture(autouse=True)
def _fp32_accurate_engines(sa):
    if sa.modules.CONV_ENGINE == "bf16x3":
        pytest.skip("SS_CONV_ENGINE=bf16x3: these bounds are for the fp32-accurate engines")


def _segment(sa, maxdisp):
    seg = sa.HotSegment(maxdisp)
    res = seg.load_state_dict(oseg.deterministic_params(), strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    return seg.cuda().train()


def _full_size_inputs(B, H=1024, W=1024):
    """The inputs and target of test_hot_segment_training_step_full_size_smoke, at batch B."""
    fl8, fr8 = dd.stereo_features(B, 256, H // 8, W // 8, 870, max_shift=3)
    fl4, fr4 = dd.stereo_features(B, 128, H // 4, W // 4, 871, max_shift=6)
    gt = dd.t_uniform((B, H // 4, W // 4), 872, -15.0, 15.0)
    return [t.cuda().requires_grad_(True) for t in (fl4, fr4, fl8, fr8)], gt.cuda()


def _step(sa, rec, feats, gt, maxdisp):
    """One train() step with every seam checked; -> increase of PATH_COUNTS["hip_train"] over the forward."""
    seg = _segment(sa, maxdisp)
    before = sa.modules.PATH_COUNTS.get("hip_train", 0)
    torch_before = sa.modules.PATH_COUNTS["torch"]
    r = seg(*feats)
    grew = sa.modules.PATH_COUNTS.get("hip_train", 0) - before
    assert sa.modules.PATH_COUNTS["torch"] == torch_before, "a PyTorch layer ran in the training pass"
    (F.smooth_l1_loss(r["pred"].squeeze(1), gt) + F.smooth_l1_loss(r["pred_att"], gt)).backward()
    torch.cuda.synchronize()
    return grew


def _assert_clean_step(rec, grew, tag):
    rep = rec.report()
    TC.write_report(tag, rep)
    missing = TC.STEP_SEAMS - rec.seams_checked()
    assert not missing, f"seams the step did not reach (renamed?): {sorted(missing)}"
    fn_fwd = sum(n for (s, p), n in rec.calls.items() if p == "fwd")
    assert fn_fwd >= grew, (fn_fwd, grew)
    assert not rec.failures(), ([e for e in rec.findings][:8], dict(rec.unexplained))
    return rep


@pytest.mark.parametrize("B", [1, 4])
def test_every_call_of_the_full_size_training_step_vs_float64(sa, monkeypatch, B):
    """The 1024^2 / maxdisp 64 step of the smoke test (stereo_features seeds 870 / 871, target 872, smooth L1): every call of the
    forward and backward at batch 1; at batch 4 the first call per distinct (seam, part, input shapes) -- the kernels' grids change with
    the shape and B, not with the call, and checking all ~300 calls in float64 would take several minutes."""
    rec = TC.Recorder(sa, first_per_shape=(B > 1)).install(monkeypatch)
    feats, gt = _full_size_inputs(B)
    grew = _step(sa, rec, feats, gt, 64)
    _assert_clean_step(rec, grew, f"step_1024_md64_b{B}")


def test_batchnorm_multi_block_reduction_at_production_sizes(sa, monkeypatch):
    """BatchNorm with batch statistics where one channel spans many reduction blocks (N = 16 * 256 * 256 per (b, c), B = 4: float partials
    and float64 atomics across blocks), each channel 30 sigma off zero; and N = 20 435 (N % 4 != 0, > 16 384: the scalar path) -- forward,
    running statistics, backward with and without the residual."""
    rec = TC.Recorder(sa).install(monkeypatch)
    T = sa.train
    gen = torch.Generator(device="cuda").manual_seed(913)
    for shape in ((4, 4, 16, 256, 256), (2, 3, 5, 61, 67)):
        C = shape[1]
        sigma = torch.linspace(0.5, 2.0, C, device="cuda").reshape(1, C, 1, 1, 1)
        x = torch.randn(shape, generator=gen, device="cuda") * sigma + 30.0 * sigma
        w = torch.linspace(0.6, 1.4, C, device="cuda").requires_grad_(True)
        b = torch.linspace(-0.3, 0.2, C, device="cuda").requires_grad_(True)
        res = torch.randn(shape, generator=gen, device="cuda")
        go = torch.randn(shape, generator=gen, device="cuda")
        for residual in (None, res):
            xg = x.clone().requires_grad_(True)
            rg = None if residual is None else residual.clone().requires_grad_(True)
            stats = (torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), torch.zeros((), dtype=torch.int64, device="cuda"), 0.1)
            y = T._BatchNormTrain.apply(xg, w, b, 1e-5, True, rg, stats)[0]
            y.backward(go)
            assert int(stats[2]) == 1
    torch.cuda.synchronize()
    assert rec.checked[("train._BatchNormTrain", "fwd")] == 4 and rec.checked[("train._BatchNormTrain", "bwd")] == 4
    TC.write_report("batchnorm_production", rec.report())
    assert not rec.failures(), (rec.findings[:8], dict(rec.unexplained))


@pytest.mark.parametrize("form", ["default", "per_wave", "f32", "stride2"])
def test_weight_gradient_forms_on_a_batch4_layer(sa, form, tuning_env, monkeypatch):
    """The weight gradient of one 32 -> 32 layer of the batch-4 step (16 x 256 x 256: one 256-row segment per column in the cooperative
    form) in each form -- the default, the per-wave form (SS_WGRAD_COOP=0), the exact-fp32 kernel (WGRAD_ENGINE = "f32") -- and the
    stride-2 shared-gout form on hourglass.conv1's 32 -> 64 layer at batch 4."""
    if form == "per_wave":
        tuning_env("SS_WGRAD_COOP", "0")
    elif form == "f32":
        monkeypatch.setattr(sa.train_layers, "WGRAD_ENGINE", "f32")
    rec = TC.Recorder(sa).install(monkeypatch)
    gen = torch.Generator(device="cuda").manual_seed(917)
    Cin, Cout, stride = (32, 64, 2) if form == "stride2" else (32, 32, 1)
    x = torch.randn((4, Cin, 16, 256, 256), generator=gen, device="cuda")
    go = torch.randn((4, Cout) + tuple(n // stride for n in (16, 256, 256)), generator=gen, device="cuda")
    sa.train_layers.conv3d_wgrad_hip(go, x, Cout, Cin, stride)
    torch.cuda.synchronize()
    assert rec.checked[("train_layers.conv3d_wgrad_hip", "fwd")] == 1
    TC.write_report(f"wgrad_b4_{form}", rec.report())
    assert not rec.failures(), rec.findings


def _scale_one_slice(state):
    def perturb(part, gw):
        if state["done"]:
            return gw
        state["done"] = True
        co, ci = divmod(int(gw.abs().amax(dim=(2, 3, 4)).argmax()), gw.shape[1])
        gw = gw.clone()
        gw[co, ci] *= 1.0 + 1e-4
        return gw
    return perturb


def _flip_one_mask_element(state):
    def perturb(part, outs):
        if state["done"] or part != "fwd" or float(outs[0].min()) < 0:          # (a BatchNorm with its ReLU)
            return outs
        state["done"] = True
        y = outs[0].clone()
        y.view(-1)[int(y.argmax())] = 0.0
        return (y,) + tuple(outs[1:])
    return perturb


@pytest.mark.parametrize("seam", ["train_layers.conv3d_wgrad_hip", "train._BatchNormTrain"])
def test_checker_flags_a_perturbed_seam_and_no_other(sa, monkeypatch, seam):
    """The checker's self-test on a small step (s128): one (co, ci) slice of one weight gradient scaled by (1 + 1e-4), or one element of
    one BatchNorm's ReLU mask flipped, in Python after the kernel -- the checker flags that seam and no other."""
    state = {"done": False}
    fn = _scale_one_slice(state) if seam.endswith("wgrad_hip") else _flip_one_mask_element(state)
    rec = TC.Recorder(sa, perturb={seam: fn}).install(monkeypatch)
    fl4, fr4, fl8, fr8, maxdisp = cases.segment_inputs("s128")
    feats = [t.cuda().requires_grad_(True) for t in (fl4, fr4, fl8, fr8)]
    gt = dd.t_uniform(tuple(fl4.shape[:1]) + tuple(fl4.shape[2:]), 872, -15.0, 15.0).cuda()
    _step(sa, rec, feats, gt, maxdisp)
    assert state["done"]
    TC.write_report(f"self_test/{seam}", rec.report())
    assert rec.failures() == {seam}, (rec.failures(), rec.findings[:4])
