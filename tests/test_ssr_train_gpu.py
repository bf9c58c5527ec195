"""SSR_upsample trained on the HIP kernels (csrc/ssr_upsample_train.hip; reference models/submodule.py:412-431, called at
models/SemStereo.py:311 and :324 in training): routing, one call and the reference's two-call pattern against the twin's own PyTorch
path in float64 (pinned to the reference's fixture by test_ssr.py), eval() under autograd, needs_input_grad, determinism, the eval
kernel after a training step, and the stand-in model's training step.  Run on the MI355X box: pytest -m gpu."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# the gradient of a bias that feeds a BatchNorm on batch statistics is zero up to rounding, so its error is read against the scale of
# the weight gradient of the same layer (the bias is that layer's weight on a constant input)
_BIAS_SCALE = {"conv.0.bias": "conv.0.weight", "conv.1.bias": "conv.1.weight", "conv1.0.bias": "conv1.0.weight",
               "conv2.0.bias": "conv2.0.weight"}


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    return semstereo_amd


def _twin(sa, training=True):
    from oracle import ssr as ossr
    mod = sa.modules.SSR_upsample(6)
    P = ossr.deterministic_ssr_params()
    res = mod.load_state_dict({k[len("ssr_upsample."):]: v for k, v in P.items()}, strict=False)
    assert not res.unexpected_keys
    return mod.train(training)


def _inputs(B, h, w, seed):
    from oracle import detdata as dd
    d = dd.t_uniform((B, 1, h, w), seed, -16.0, 16.0)
    wt = dd.t_normalish((B, 6, 4 * h, 4 * w), seed + 1)
    lab = dd.t_normalish((B, 6, 4 * h, 4 * w), seed + 2) * 2.0
    gt = dd.t_uniform((B, 4 * h, 4 * w), seed + 3, -64.0, 64.0)
    return d, wt, lab, gt


def _run(mod, calls, dev, dtype, wt_grad=True):
    """calls = [(depth_low, loss weight, target)] with ONE (weights, pred_label) pair: loss = sum_i w_i smooth-L1(4 out_i, gt_i) as
    model_loss_train weighs the head's outputs.  Returns the outputs, the input / parameter gradients and the module's buffers."""
    ws, lab = calls[0][3], calls[0][4]
    leaf = lambda t, rg: t.detach().to(dev, dtype).clone().requires_grad_(rg)      # noqa: E731
    wt, lb = leaf(ws, wt_grad), leaf(lab, wt_grad)
    ds = [leaf(c[0], True) for c in calls]
    mod.zero_grad(set_to_none=True)
    outs, loss = [], 0.0
    for d, (_, lw, gt, _, _) in zip(ds, calls):
        y = mod(d, wt, lb)
        outs.append(y)
        loss = loss + lw * F.smooth_l1_loss(4 * y, gt.to(dev, dtype))
    loss.backward()
    res = {f"out{i}": y.detach() for i, y in enumerate(outs)}
    res.update({f"grad_depth_low{i}": d.grad for i, d in enumerate(ds)})
    res["grad_weights"], res["grad_pred_label"] = wt.grad, lb.grad
    res.update({"grad:" + k: p.grad for k, p in mod.named_parameters()})
    res.update({"buf:" + k: b.detach().clone() for k, b in mod.named_buffers()})
    return res


def _check(hip, f64, f32, skip=()):
    for k, ref in f64.items():
        if k in skip:
            continue
        a = hip[k]
        if k.startswith("buf:"):
            if k.endswith("num_batches_tracked"):
                assert int(a) == int(ref), (k, int(a), int(ref))
                continue
            err = float((a.double().cpu() - ref).abs().max())
            assert err <= 1e-6 * float(ref.abs().max()) + 1e-12, (k, err)
            continue
        assert a is not None, k
        a, r, c = a.double().cpu(), ref.double(), f32[k].double()
        err, e32, scale = float((a - r).abs().max()), float((c - r).abs().max()), float(r.abs().max())
        ok = err <= 5e-6 * scale or err <= 1.5 * e32
        name = k[len("grad:"):] if k.startswith("grad:") else None
        if not ok and name in _BIAS_SCALE:
            ok = err <= 5e-6 * float(f64["grad:" + _BIAS_SCALE[name]].abs().max())
        assert ok, (k, err, scale, e32)


def _three(sa, calls, training=True):
    base = _twin(sa, training)
    m64, m32, mg = copy.deepcopy(base).double(), copy.deepcopy(base), copy.deepcopy(base).cuda()
    torch.set_num_threads(min(16, __import__("os").cpu_count() or 1))
    r64 = _run(m64, calls, "cpu", torch.float64)
    r32 = _run(m32, calls, "cpu", torch.float32)
    sa.modules.drop_parked_gates()
    before = dict(sa.modules.PATH_COUNTS)
    rg = _run(mg, calls, "cuda", torch.float32)
    torch.cuda.synchronize()
    return r64, r32, rg, before, mg


def test_routing(sa, monkeypatch):
    """This fails without the training kernels: a train() call with autograd used to run the PyTorch composition."""
    mod = _twin(sa).cuda()
    d, wt, lab, gt = _inputs(1, 8, 32, 4100)
    sa.modules.drop_parked_gates()
    before = dict(sa.modules.PATH_COUNTS)
    wg, lg = wt.cuda().requires_grad_(True), lab.cuda().requires_grad_(True)
    for _ in range(2):
        y = mod(d.cuda().requires_grad_(True), wg, lg)
        y.sum().backward()
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"]
    assert sa.modules.PATH_COUNTS.get("ssr_train", 0) == before.get("ssr_train", 0) + 2
    assert sa.modules.PATH_COUNTS.get("hip_train", 0) == before.get("hip_train", 0) + 2
    assert mod not in sa.modules._GATE_PARKED
    with torch.no_grad():                              # train() without autograd: the same kernels, forward only
        mod(d.cuda(), wt.cuda(), lab.cuda())
    assert sa.modules.PATH_COUNTS.get("ssr_train", 0) == before.get("ssr_train", 0) + 3
    monkeypatch.setattr(sa.engine, "SSR_TRAIN_HIP", False)
    t0 = sa.modules.PATH_COUNTS["torch"]
    mod(d.cuda().requires_grad_(True), wg, lg).sum().backward()
    assert sa.modules.PATH_COUNTS["torch"] == t0 + 1
    assert sa.modules.PATH_COUNTS.get("ssr_train", 0) == before.get("ssr_train", 0) + 3
    sa.modules.drop_parked_gates()


@pytest.mark.parametrize("shape", [(2, 37, 70), (1, 1, 9), (1, 8, 32), (4, 256, 256)])
def test_one_training_call_vs_float64(sa, shape):
    B, h, w = shape
    d, wt, lab, gt = _inputs(B, h, w, 4200 + h)
    r64, r32, rg, before, _ = _three(sa, [(d, 1.0, gt, wt, lab)])
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"]
    _check(rg, r64, r32)


def test_two_calls_as_the_reference_trains(sa):
    """models/SemStereo.py:311, 324: the same (spx_pred, pred_label) twice, different disparities; loss weights 1.0 (pred_up, the second
    call) and 0.5 (pred_att_up, the first).  The gate's BatchNorms move their running statistics twice."""
    d1, wt, lab, gt1 = _inputs(2, 37, 70, 4300)
    d2, _, _, gt2 = _inputs(2, 37, 70, 4310)
    r64, r32, rg, before, _ = _three(sa, [(d1, 0.5, gt1, wt, lab), (d2, 1.0, gt2, wt, lab)])
    assert sa.modules.PATH_COUNTS.get("ssr_train", 0) == before.get("ssr_train", 0) + 2
    assert int(rg["buf:conv1.1.num_batches_tracked"]) == 2 and int(rg["buf:conv2.1.num_batches_tracked"]) == 2
    _check(rg, r64, r32)


def test_eval_with_autograd_freezes_the_statistics(sa):
    d, wt, lab, gt = _inputs(2, 37, 70, 4400)
    r64, r32, rg, before, _ = _three(sa, [(d, 1.0, gt, wt, lab)], training=False)
    assert sa.modules.PATH_COUNTS.get("ssr_train", 0) == before.get("ssr_train", 0) + 1
    for k, v in _twin(sa, False).named_buffers():
        assert torch.equal(rg["buf:" + k].cpu(), v), k              # untouched
    _check(rg, r64, r32)


def test_needs_input_grad(sa):
    d, wt, lab, gt = _inputs(2, 37, 70, 4500)
    base = _twin(sa).cuda()
    full = _run(copy.deepcopy(base), [(d, 1.0, gt, wt, lab)], "cuda", torch.float32)
    part = _run(copy.deepcopy(base), [(d, 1.0, gt, wt, lab)], "cuda", torch.float32, wt_grad=False)
    assert part["grad_weights"] is None and part["grad_pred_label"] is None
    for k, v in full.items():
        if k not in ("grad_weights", "grad_pred_label"):
            assert torch.equal(part[k], v), k


def test_determinism(sa):
    d, wt, lab, gt = _inputs(4, 64, 96, 4600)
    base = _twin(sa).cuda()
    a = _run(copy.deepcopy(base), [(d, 1.0, gt, wt, lab)], "cuda", torch.float32)
    b = _run(copy.deepcopy(base), [(d, 1.0, gt, wt, lab)], "cuda", torch.float32)
    for k, v in a.items():
        assert torch.equal(b[k], v), k


@pytest.mark.parametrize("optimizer_step", [True, False])
def test_eval_after_a_training_step(sa, optimizer_step):
    """A train() step (and an SGD step), then the eval / no-grad inference kernel: it must fold the UPDATED running statistics and
    parameters (the in-kernel update bumps the buffers' versions, which the eval path's parameter cache is keyed on)."""
    d, wt, lab, gt = _inputs(2, 37, 70, 4700)
    base = _twin(sa)
    m64, mg = copy.deepcopy(base).double(), copy.deepcopy(base).cuda()
    # the eval kernel first, so that its folded parameters are cached with the old statistics
    mg.eval()
    with torch.no_grad():
        sa.deferred.real(mg(d.cuda(), wt.cuda(), lab.cuda()))
    for m, dev, dt in ((m64, "cpu", torch.float64), (mg, "cuda", torch.float32)):
        m.train()
        _run(m, [(d, 1.0, gt, wt, lab)], dev, dt)
        if optimizer_step:
            with torch.no_grad():
                for p in m.parameters():
                    p.add_(p.grad, alpha=-0.5)
        m.eval()
    sa.modules.drop_parked_gates()
    ref = m64(d.double().requires_grad_(True), wt.double(), lab.double()).detach()     # (autograd on: the PyTorch composition on the CPU)
    sa.modules.drop_parked_gates()
    with torch.no_grad():
        before = dict(sa.modules.PATH_COUNTS)
        y = sa.deferred.real(mg(d.cuda(), wt.cuda(), lab.cuda()))
    assert sa.modules.PATH_COUNTS["hip"] > before["hip"]
    err = float((y.double().cpu() - ref).abs().max())
    assert err <= 2e-5, err


def test_model_level_training_step(sa):
    """The stand-in model (tests/standin_model.py) with install() + accelerate() in train(): one step with the four-term loss of
    model_loss_train runs the head on the HIP training path twice, and every gradient of the head's parameters is finite."""
    import standin_model
    from oracle import detdata as dd
    net = standin_model.StandInSemStereo(64, sa.modules).cuda().train()
    left = dd.t_normalish((1, 3, 128, 160), 4801).cuda()
    right = torch.roll(left, shifts=-3, dims=3) + 0.05 * dd.t_normalish((1, 3, 128, 160), 4802).cuda()
    previous = sa.install(standin_model)
    try:
        sa.accelerate(net)
        before = dict(sa.modules.PATH_COUNTS)
        outs, _, _ = net(left, right)
        gt = dd.t_uniform((1, 128, 160), 4803, -60.0, 60.0).cuda()
        gt4 = dd.t_uniform((1, 32, 40), 4804, -15.0, 15.0).cuda()
        loss = sum(wl * F.smooth_l1_loss(o, g) for o, g, wl in zip(outs, (gt, gt4, gt, gt4), (1.0, 0.6, 0.5, 0.3)))
        loss.backward()
        assert sa.modules.PATH_COUNTS.get("ssr_train", 0) == before.get("ssr_train", 0) + 2
        for k, p in net.ssr_upsample.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    finally:
        sa.uninstall(standin_model, previous)
        sa.modules.drop_parked_gates()
