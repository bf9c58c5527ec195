"""`accelerate(model, fuse_forward=True, fuse_training=True)`: a train() call of a model shaped like the reference (tests/standin_model.py)
runs `install.fused_training_forward` -- the reference's sub-module calls around `segment.run_segment`, i.e. `train.attention_tail` and
`train.concat_volume_sampled` instead of the statements of models/SemStereo.py:279-310, :316-318 -- and must agree with the model's own
forward() on the same HIP ops and twins, both measured against a float64 CPU run of the same model on the oracle op library:
outputs, gradients, BatchNorm buffers.  Three runs per case, computed once and shared.  Run on the MI355X box: pytest -m gpu."""
import copy
import json
import math
import os

import pytest
import torch

from test_dropin_gpu import _build, _images

pytestmark = pytest.mark.gpu

#: name -> (H, W, att_weights_only).  128 x 160: W/4 = 40, no multiple of 64 -> the three-statement concat volume (counted);
#: 256 x 256: W/4 = 64 -> the one-launch train.concat_volume_sampled (the `t256_md64` size of the segment training test)
CASES = {"h128w160": (128, 160, False), "h128w160_att": (128, 160, True), "h256w256": (256, 256, False), "h256w256_att": (256, 256, True)}
PX = 4e-3                   # 1e-3 px at 1/4 scale, on the x4 outputs (tests/test_dropin_gpu.py)
REPORT = {}
_RUNS = {}
# the gradient of a bias that feeds a BatchNorm on batch statistics is zero up to rounding (1e-20 in float64), so its error is read
# against the scale of the weight gradient of the same layer, as in tests/test_ssr_train_gpu.py
_BIAS_SCALE = {f"ssr_upsample.{k}.bias": f"ssr_upsample.{k}.weight" for k in ("conv.1", "conv1.0", "conv2.0")}


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    return semstereo_amd


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    # (where the reports go: $SS_TEST_REPORT_DIR, by default test_reports/ at the repository root, git-ignored -- as tests/train_calls.py)
    out = os.environ.get("SS_TEST_REPORT_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test_reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "train_route_report.json"), "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)
    with open(os.path.join(out, "train_route_err.txt"), "w") as f:
        f.write("# tests/test_train_route_gpu.py: routed (fused_training_forward) and untouched (the model's own forward() on the HIP ops and\n"
                "# twins) train() calls of the stand-in model against a float64 CPU run on the oracle op library\n")
        for k in sorted(REPORT):
            f.write(f"{k} = {REPORT[k]}\n")
    _RUNS.clear()


def _scalar(out):
    outs, lab, lab_r = out
    return sum(o.mean() for o in outs) + lab.mean() + lab_r.mean()


def _snapshot(net, out):
    outs, lab, lab_r = out
    return dict(outs=[o.detach().cpu() for o in outs], labels=[lab.detach().cpu(), lab_r.detach().cpu()],
                structure=(type(out).__name__, type(outs).__name__, [(tuple(o.shape), o.dtype) for o in list(outs) + [lab, lab_r]]),
                grads={k: p.grad.detach().cpu() for k, p in net.named_parameters() if p.grad is not None},
                buffers={k: b.detach().cpu().clone() for k, b in net.named_buffers()})


def _segment_hip_train(sa, H, W, att_only):
    """PATH_COUNTS["hip_train"] of one HotSegment.train() pass at this size"""
    from semstereo_amd import segment
    seg = sa.HotSegment(64).cuda().train()
    g = torch.Generator().manual_seed(1)
    feats = [torch.randn(1, c, H // s, W // s, generator=g).cuda() for c, s in ((128, 4), (128, 4), (256, 8), (256, 8))]
    before = sa.modules.PATH_COUNTS.get("hip_train", 0)
    segment.run_segment(seg, *feats, matching=not att_only)
    return sa.modules.PATH_COUNTS.get("hip_train", 0) - before


def _runs(sa, case):
    """The three runs of a case: float64 on the CPU, the untouched forward on the HIP ops + twins, the routed forward."""
    if case in _RUNS:
        return _RUNS[case]
    H, W, att_only = CASES[case]
    net, module = _build(sa, att_weights_only=att_only)
    net.train()
    left, right = _images(1, H, W)
    R = dict(H=H, W=W, att_only=att_only, left=left, right=right)
    counts = lambda: {k: sa.modules.PATH_COUNTS.get(k, 0) for k in ("torch", "hip_train", "train_route", "train_tail_statements",   # noqa: E731
                                                                     "train_concat_statements")}
    # float64, CPU, oracle op library (standin_model's own globals), PyTorch layers
    ref = copy.deepcopy(net).cpu().double().train()
    out = ref(left.cpu().double(), right.cpu().double())
    _scalar(out).backward()
    R["f64"] = _snapshot(ref, out)
    sa.modules.drop_parked_gates()
    del ref, out
    # the model's own forward(), untouched, after install() + accelerate(): what a training script gets without the route
    plain = copy.deepcopy(net)
    previous = sa.install(module)
    try:
        sa.accelerate(plain)
        calls = plain.calls
        out = plain(left, right)
        _scalar(out).backward()
        assert plain.calls == calls + 1
        R["untouched"] = _snapshot(plain, out)
    finally:
        sa.uninstall(module, previous)
    del plain, out
    # the routed forward (the op library in the model module's globals is NOT needed: nothing of forward()'s text runs)
    R["segment_hip_train"] = _segment_hip_train(sa, H, W, att_only)
    routed = copy.deepcopy(net)
    sa.accelerate(routed, fuse_forward=True, fuse_training=True)
    calls, before = routed.calls, counts()
    out = routed(left, right)
    after = counts()
    _scalar(out).backward()
    torch.cuda.synchronize()
    R["routed"] = _snapshot(routed, out)
    R["routed_calls"] = routed.calls - calls
    R["routed_counts"] = {k: after[k] - before[k] for k in after}
    R["routed_net"] = routed
    _RUNS[case] = R
    return R


@pytest.mark.parametrize("case", list(CASES))
def test_train_call_takes_the_route(sa, case):
    R = _runs(sa, case)
    c = R["routed_counts"]
    REPORT[f"{case}/counts"] = dict(c, segment_hip_train=R["segment_hip_train"])
    print(case, c, R["segment_hip_train"])
    assert R["routed_calls"] == 0, "the model's own forward() ran"
    assert c["train_route"] == 1 and c["torch"] == 0, c
    assert c["hip_train"] >= R["segment_hip_train"] > 0, (c, R["segment_hip_train"])
    # the fused tail applies at both sizes; the one-launch concat volume only where W/4 is a multiple of 64 -- its fallback is counted
    assert c["train_tail_statements"] == 0
    assert c["train_concat_statements"] == (1 if (R["W"] // 4) % 64 and not R["att_only"] else 0), c


@pytest.mark.parametrize("case", list(CASES))
def test_structure_equals_the_untouched_forwards(sa, case):
    R = _runs(sa, case)
    assert R["routed"]["structure"] == R["untouched"]["structure"]
    n = 2 if R["att_only"] else 4
    assert R["routed"]["structure"][:2] == ("tuple", "list") and len(R["routed"]["outs"]) == n
    assert all(dt == torch.float32 for _, dt in R["routed"]["structure"][2])


@pytest.mark.parametrize("case", list(CASES))
def test_outputs_are_as_close_to_float64_as_the_untouched_forwards(sa, case):
    """Per estimate: the routed result's distance from the float64 run is at most twice the untouched forward's (median, and share of
    pixels beyond 4e-3 px: the fused selection kernel rounds the propagated logits in another order than the statements and may move
    an isolated top-24 / top-2 pick), and in either arm at most 0.5 % of the pixels lie beyond 4e-3 px."""
    R = _runs(sa, case)
    names = ["pred_att_up", "pred_att"] if R["att_only"] else ["pred_up", "pred", "pred_att_up", "pred_att"]
    figures = {}
    for i, name in enumerate(names):
        for arm in ("routed", "untouched"):
            e = (R[arm]["outs"][i].double() - R["f64"]["outs"][i]).abs()
            figures[name, arm] = (float(e.median()), float((e > PX).double().mean()), float(e.max()))
            REPORT[f"{case}/out/{name}/{arm}"] = dict(zip(("median", "share_beyond_4e-3", "max"), figures[name, arm]))
    for i, arm in enumerate(("routed", "untouched")):
        for j, lab in enumerate(("pred_label", "pred_label_r")):
            REPORT[f"{case}/out/{lab}/{arm}"] = float((R[arm]["labels"][j].double() - R["f64"]["labels"][j]).abs().max())
    print(case, figures)
    for name in names:
        (med_r, far_r, _), (med_u, far_u, _) = figures[name, "routed"], figures[name, "untouched"]
        assert far_r <= 0.005 and far_u <= 0.005, (name, far_r, far_u)
        assert med_r <= 2 * med_u and far_r <= 2 * far_u, (name, figures[name, "routed"], figures[name, "untouched"])
    # the label maps come from the same calls on the same inputs in both arms
    for j in range(2):
        assert torch.equal(R["routed"]["labels"][j], R["untouched"]["labels"][j])


@pytest.mark.parametrize("case", list(CASES))
def test_gradients_against_float64(sa, case):
    """The parameters that receive a gradient are the untouched run's; per parameter max |g - g64| / max |g64|: median <= 5e-3, worst
    <= 5e-2 (the segment training test's bound where a pick or a ReLU may land on the other side); gamma / beta -- sums of nearly
    cancelling per-pixel terms -- within 1e-4 of the overall gradient scale."""
    R = _runs(sa, case)
    g64 = R["f64"]["grads"]
    assert set(R["routed"]["grads"]) == set(R["untouched"]["grads"]) == set(g64)
    gscale = max(float(g.abs().max()) for g in g64.values())
    summary = {}
    for arm in ("routed", "untouched"):
        grads = R[arm]["grads"]
        assert all(bool(torch.isfinite(g).all()) for g in grads.values()), arm
        errs = {k: float((g.double() - g64[k]).abs().max()) / (float(g64[_BIAS_SCALE.get(k, k)].abs().max()) + 1e-12) for k, g in grads.items()}
        scalars = {k: float((grads[k].double() - g64[k]).abs().max()) / gscale for k in ("gamma", "beta")}
        for k in scalars:
            errs.pop(k)
        vals = sorted(errs.values())
        summary[arm] = dict(median=vals[len(vals) // 2], worst=vals[-1], worst_parameter=max(errs, key=errs.get), gamma=scalars["gamma"],
                            beta=scalars["beta"], parameters=len(grads),
                            worst_five={k: errs[k] for k in sorted(errs, key=errs.get, reverse=True)[:5]})
        REPORT[f"{case}/grad/{arm}"] = summary[arm]
    print(case, summary)
    s = summary["routed"]
    assert s["median"] <= 5e-3 and s["worst"] <= 5e-2, s
    assert s["gamma"] <= 1e-4 and s["beta"] <= 1e-4, s


@pytest.mark.parametrize("case", list(CASES))
def test_batchnorm_buffers_after_the_call(sa, case):
    """num_batches_tracked equal in all three runs (a skipped, merged or doubled call shows here); running_mean / running_var no
    farther from the float64 run than twice the untouched arm's distance plus one fp32 ulp at the buffer's largest magnitude."""
    R = _runs(sa, case)
    b64, bu, br = R["f64"]["buffers"], R["untouched"]["buffers"], R["routed"]["buffers"]
    assert list(b64) == list(bu) == list(br)
    tracked, worst = 0, (0.0, None)
    for k in b64:
        if k.endswith("num_batches_tracked"):
            assert int(b64[k]) == int(bu[k]) == int(br[k]), (k, int(b64[k]), int(bu[k]), int(br[k]))
            tracked += int(br[k])
        elif k.endswith(("running_mean", "running_var")):
            d_r, d_u = float((br[k].double() - b64[k]).abs().max()), float((bu[k].double() - b64[k]).abs().max())
            mag = float(b64[k].abs().max())
            ulp = 2.0 ** (math.floor(math.log2(mag)) - 23) if mag > 0 else 0.0
            if d_r - (2 * d_u + ulp) > worst[0]:
                worst = (d_r - (2 * d_u + ulp), k)
            assert d_r <= 2 * d_u + ulp, (k, d_r, d_u, ulp)
    REPORT[f"{case}/bn/calls_tracked"] = tracked
    assert tracked > 0


@pytest.mark.parametrize("case", list(CASES))
def test_second_call_reproduces_the_first(sa, case):
    """No weight update in between: train() outputs depend on the batch alone, so they are reproduced to rounding (the statistics and
    scatter kernels sum through atomics) -- the form two fp32 evaluation orders are held to in tests/test_dropin_gpu.py; and no class
    gate parked by SSR_upsample outlives a call, also where the head keeps its PyTorch composition and is called an odd number of
    times (att_weights_only)."""
    from semstereo_amd import engine
    R = _runs(sa, case)
    net = R["routed_net"]
    for p in net.parameters():
        p.grad = None
    outs, lab, lab_r = net(R["left"], R["right"])
    assert net.ssr_upsample not in sa.modules._GATE_PARKED
    for i, (o, w) in enumerate(zip(outs, R["routed"]["outs"])):
        e = (o.detach().cpu() - w).abs()
        REPORT[f"{case}/second_call/{i}"] = dict(median=float(e.median()), max=float(e.max()))
        assert float(e.median()) <= 1e-4 and float((e <= PX).float().mean()) >= 0.995, (i, float(e.median()), float(e.max()))
    assert torch.equal(lab.cpu(), R["routed"]["labels"][0]) and torch.equal(lab_r.cpu(), R["routed"]["labels"][1])
    if R["att_only"] and R["H"] == 128:
        prev, engine.SSR_TRAIN_HIP = engine.SSR_TRAIN_HIP, False        # the head's PyTorch composition parks its gate for a second call
        try:
            before = sa.modules.PATH_COUNTS["torch"]
            net(R["left"], R["right"])
            assert sa.modules.PATH_COUNTS["torch"] == before + 1        # (that composition ran ...)
            assert net.ssr_upsample not in sa.modules._GATE_PARKED      # ... and what it parked is gone
        finally:
            engine.SSR_TRAIN_HIP = prev


def test_environment_switch_turns_the_route_off(sa, monkeypatch):
    R = _runs(sa, "h128w160_att")
    net = R["routed_net"]
    module = __import__("standin_model")
    previous = sa.install(module)
    try:
        monkeypatch.setenv("SS_FUSE_TRAINING", "0")
        calls, routed = net.calls, sa.modules.PATH_COUNTS.get("train_route", 0)
        out = net(R["left"], R["right"])
        assert net.calls == calls + 1 and sa.modules.PATH_COUNTS.get("train_route", 0) == routed and len(out) == 3
    finally:
        sa.uninstall(module, previous)


def test_eval_under_autograd_takes_the_route(sa):
    """eval() with parameters that require grad (frozen statistics, which the twins support): routed, the eval-mode structure, every
    buffer untouched, finite gradients."""
    net, module = _build(sa)
    left, right = _images(1, 128, 160)
    sa.accelerate(net, fuse_forward=True, fuse_training=True)
    assert not net.training and all(p.requires_grad for p in net.parameters())
    buffers = {k: b.detach().clone() for k, b in net.named_buffers()}
    calls, before = net.calls, dict(sa.modules.PATH_COUNTS)
    out = net(left, right)
    assert net.calls == calls and sa.modules.PATH_COUNTS.get("train_route", 0) == before.get("train_route", 0) + 1
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"]
    assert isinstance(out, tuple) and len(out) == 2 and isinstance(out[0], list) and len(out[0]) == 1
    (disp,), lab = out
    assert disp.shape == (1, 128, 160) and lab.shape == (1, 6, 128, 160) and disp.requires_grad
    (disp.mean() + lab.mean()).backward()
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert len(grads) > 60 and all(bool(torch.isfinite(g).all()) for g in grads)
    for k, b in net.named_buffers():
        assert torch.equal(b, buffers[k]), k
    # ... and without autograd the same model's eval() call is the inference route's
    with torch.no_grad():
        (d0,), lab0 = net(left, right)
    assert net.calls == calls and sa.modules.PATH_COUNTS.get("train_route", 0) == before.get("train_route", 0) + 1
    err = (d0 - disp.detach()).abs()
    assert float(err.median()) <= 1e-4 and float((err <= PX).float().mean()) >= 0.995, (float(err.median()), float(err.max()))
    sa.restore_forward(net)
