"""The training objective on the HIP kernels (csrc/loss.hip; reference main_us3d.py:199-208, models/loss.py): every function on every
fixture case against the reference's float64 record (tests/golden/loss.npz), the full training shape and a ragged one against the
PyTorch composition in float64, the warped label map bit for bit, routing, needs_input_grad, repeatability, no host wait, the NaN
cases, and one training step of the stand-in model with install_losses.  Run on the MI355X box: pytest -m gpu.

The criterion is the one the project's training kernels are held to (tests/test_ssr_train_gpu.py:_check): the error against the
float64 values is at most 5e-6 of the tensor's largest magnitude, or at most 1.5 x the error of the fp32 CPU composition against the
same float64 values."""
import os
import types

import numpy as np
import pytest
import torch

from golden import loss_cases

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(4, 1024, 1024), (2, 150, 138)]


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return semstereo_amd


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "loss.npz"))


def _check_one(what, hip, f64, f32):
    a, r, c = (torch.as_tensor(np.asarray(t)).double().reshape(-1) for t in (hip, f64, f32))
    assert a.shape == r.shape, (what, a.shape, r.shape)
    assert torch.equal(torch.isnan(a), torch.isnan(r)), (what, "NaN pattern")
    keep = ~torch.isnan(r)
    if not bool(keep.any()):
        return
    a, r, c = a[keep], r[keep], c[keep]
    err, e32, scale = float((a - r).abs().max()), float((c - r).abs().max()), float(r.abs().max())
    print(f"{what}: error {err:.3e}  fp32 CPU composition {e32:.3e}  scale {scale:.3e}")
    assert err <= 5e-6 * scale or err <= 1.5 * e32, (what, err, scale, e32)


def _check(tag, hip, f64, f32):
    """{function: (loss, [grads])} of the HIP run, the float64 values and the fp32 CPU composition."""
    for fn, (loss, grads) in f64.items():
        _check_one(f"{tag}/{fn}/loss", hip[fn][0], loss, f32[fn][0])
        assert len(hip[fn][1]) == len(grads), (tag, fn)
        for i, g in enumerate(grads):
            _check_one(f"{tag}/{fn}/grad{i}", hip[fn][1][i], g, f32[fn][1][i])


def _fixture_values(fx, name):
    out = {}
    for fn in loss_cases.FUNCTIONS:
        grads, i = [], 0
        while f"{name}/{fn}/grad64/{i}" in fx.files:
            grads.append(fx[f"{name}/{fn}/grad64/{i}"])
            i += 1
        out[fn] = (fx[f"{name}/{fn}/loss64"], grads)
    return out


def _hip_run(sa, d, calls=4):
    before = dict(sa.modules.PATH_COUNTS)
    res = loss_cases.run_data(sa.losses, d, torch.float32, "cuda")
    torch.cuda.synchronize()
    assert sa.modules.PATH_COUNTS.get("loss_hip", 0) == before.get("loss_hip", 0) + calls
    assert sa.modules.PATH_COUNTS.get("loss_torch", 0) == before.get("loss_torch", 0)
    return res


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(loss_cases.CASES))
def test_fixture_cases(sa, fx, name):
    d = loss_cases.inputs(name)
    hip = _hip_run(sa, d)
    f32 = loss_cases.run_data(sa.losses, d, torch.float32, "cpu")
    _check(name, hip, _fixture_values(fx, name), f32)


# 2 ------------------------------------------------------------------------------------------------------------------------------
def _shape_inputs(B, H, W, seed, label_dtype=torch.int64):
    from oracle import detdata as dd
    h4, w4 = H // 4, W // 4
    gt, gt4 = dd.t_uniform((B, H, W), seed, -40.0, 40.0), dd.t_uniform((B, h4, w4), seed + 1, -40.0, 40.0)
    labels = torch.from_numpy(np.minimum(np.floor(dd.uniform((B, H, W), seed + 2, 0.0, 6.0)), 5).astype(np.int64)).to(label_dtype)
    ests = [(gt if i % 2 == 0 else gt4) + 1.5 * dd.t_normalish((B, H, W) if i % 2 == 0 else (B, h4, w4), seed + 10 + i) for i in range(4)]
    return dict(ests=ests, gt=gt, gt4=gt4, labels=labels, logits=2.0 * dd.t_normalish((B, 6, H, W), seed + 3),
                logits_r=2.0 * dd.t_normalish((B, 6, H, W), seed + 4), maxdisp=32, attn=False)


def _objective(lib, d, dtype, device):
    """train_objective and the gradients of everything the model produced: {"objective": (loss, grads), "parts": ...}."""
    cast = lambda t: t.to(device=device, dtype=dtype)                       # noqa: E731
    ests = [cast(t).requires_grad_(True) for t in d["ests"]]
    z, zr = cast(d["logits"]).requires_grad_(True), cast(d["logits_r"]).requires_grad_(True)
    loss, dl, ll, rl = lib.train_objective(ests, z, zr, cast(d["gt"]), cast(d["gt4"]), d["labels"].to(device), d["maxdisp"], d["attn"])
    loss.backward()
    cpu = lambda t: t.detach().cpu()                                         # noqa: E731
    return {"objective": (cpu(loss), [cpu(t.grad) for t in ests + [z, zr]]), "disp": (cpu(dl), []), "label": (cpu(ll), []), "lrsc": (cpu(rl), [])}


def _assert_mask_is_not_degenerate(d):
    for gt in (d["gt"], d["gt4"]):
        kept = float(loss_cases.range_mask(gt, d["maxdisp"]).float().mean())
        assert 0.5 <= kept <= 0.95, kept


@pytest.mark.parametrize("shape", SHAPES)
def test_four_functions_against_float64(sa, shape):
    B, H, W = shape
    d = _shape_inputs(B, H, W, 8100 + H, torch.int64 if H == 1024 else torch.uint8)
    _assert_mask_is_not_degenerate(d)
    hip = _hip_run(sa, d)
    f64 = loss_cases.run_data(sa.losses, d, torch.float64, "cpu")
    f32 = loss_cases.run_data(sa.losses, d, torch.float32, "cpu")
    _check(f"{B}x{H}x{W}", hip, f64, f32)


@pytest.mark.parametrize("shape", SHAPES)
def test_train_objective_against_float64(sa, shape):
    B, H, W = shape
    d = _shape_inputs(B, H, W, 8300 + H, torch.float32 if H == 1024 else torch.int64)
    _assert_mask_is_not_degenerate(d)
    before = dict(sa.modules.PATH_COUNTS)
    hip = _objective(sa.losses, d, torch.float32, "cuda")
    torch.cuda.synchronize()
    assert sa.modules.PATH_COUNTS.get("loss_hip", 0) == before.get("loss_hip", 0) + 3
    assert sa.modules.PATH_COUNTS.get("loss_torch", 0) == before.get("loss_torch", 0)
    _check(f"objective {B}x{H}x{W}", hip, _objective(sa.losses, d, torch.float64, "cpu"), _objective(sa.losses, d, torch.float32, "cpu"))


# 3 ------------------------------------------------------------------------------------------------------------------------------
def _warped_on_hip(sa, logits_r, disp, labels):
    out = torch.full(labels.shape, -7, dtype=torch.int64, device="cuda")
    before = sa.modules.PATH_COUNTS.get("loss_hip", 0)
    sa.losses.LRSC_loss(logits_r.cuda(), [disp.cuda()], labels.cuda(), warped=out)
    torch.cuda.synchronize()
    assert sa.modules.PATH_COUNTS.get("loss_hip", 0) == before + 1
    return out.cpu()


def test_warped_labels_bit_for_bit_on_the_edge_case(sa, fx):
    d = loss_cases.inputs("lrsc_edges")
    got = _warped_on_hip(sa, d["logits_r"], d["ests"][0], d["labels"])
    assert torch.equal(got, sa.losses.warp_labels(d["ests"][0], d["labels"]))                  # PyTorch's fp32 expression
    assert np.array_equal(got.numpy(), fx["lrsc_edges/lrsc/warped32"].astype(np.int64))        # ... which is the reference's
    assert not np.array_equal(got.numpy(), fx["lrsc_edges/lrsc/warped64"].astype(np.int64))    # and not a float64 evaluation


@pytest.mark.parametrize("label_dtype", [torch.int64, torch.uint8, torch.float32])
def test_warped_labels_bit_for_bit_at_full_size(sa, label_dtype):
    B, H, W = 4, 1024, 1024
    d = _shape_inputs(B, H, W, 8500, label_dtype)
    disp = d["ests"][0].clone()
    disp[:, ::7] = torch.round(disp[:, ::7])                    # rows of exact integers
    disp[:, 1::7] = disp[:, 1::7] * 30.0                        # rows that leave the image on both sides
    disp[:, 2::7] = 1e-9 * torch.sign(disp[:, 2::7])            # rows where fp32 and float64 truncate differently
    got = _warped_on_hip(sa, d["logits_r"], disp, d["labels"])
    assert torch.equal(got, sa.losses.warp_labels(disp, d["labels"]))


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_routing_and_needs_input_grad(sa, monkeypatch):
    d = loss_cases.inputs("b2_48x80")
    _hip_run(sa, d)                                              # CUDA fp32: "loss_hip" moves, "loss_torch" does not
    before = dict(sa.modules.PATH_COUNTS)
    monkeypatch.setattr(sa.engine, "LOSS_HIP", False)
    off = loss_cases.run_data(sa.losses, d, torch.float32, "cuda")
    torch.cuda.synchronize()
    assert sa.modules.PATH_COUNTS.get("loss_torch", 0) == before.get("loss_torch", 0) + 4
    assert sa.modules.PATH_COUNTS.get("loss_hip", 0) == before.get("loss_hip", 0)
    monkeypatch.setattr(sa.engine, "LOSS_HIP", True)
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"]
    f64 = loss_cases.run_data(sa.losses, d, torch.float64, "cpu")
    _check("switched off", off, f64, loss_cases.run_data(sa.losses, d, torch.float32, "cpu"))
    # a detached estimate gets no gradient, the others the same bits as before
    cu = lambda t: t.cuda()                                                                     # noqa: E731
    gts, masks = [cu(d["gt"]), cu(d["gt4"])] * 2, [cu(loss_cases.range_mask(d["gt"], 32)), cu(loss_cases.range_mask(d["gt4"], 32))] * 2
    full = [cu(t).requires_grad_(True) for t in d["ests"]]
    part = [cu(t).requires_grad_(i != 1) for i, t in enumerate(d["ests"])]
    sa.losses.model_loss_train(full, gts, masks).backward()
    sa.losses.model_loss_train(part, gts, masks).backward()
    assert part[1].grad is None
    for i in (0, 2, 3):
        assert torch.equal(part[i].grad, full[i].grad), i
    z = cu(d["logits"])                                          # no gradient asked at all: the forward alone
    assert not sa.losses.model_label_loss(z, cu(d["labels"]), 6, False).requires_grad
    # unsupported inputs keep the composition: float64 on the GPU, five classes
    before = dict(sa.modules.PATH_COUNTS)
    sa.losses.model_label_loss(z.double(), cu(d["labels"]), 6, False)
    sa.losses.model_label_loss(z[:, :5].contiguous(), cu(d["labels"]).clamp(max=4), 5, False)
    assert sa.modules.PATH_COUNTS.get("loss_torch", 0) == before.get("loss_torch", 0) + 2
    assert sa.modules.PATH_COUNTS.get("loss_hip", 0) == before.get("loss_hip", 0)


def test_label_dtypes_and_stray_labels(sa):
    """int64, uint8 and float32 labels give the same bits; a label outside [0, 6) counts as ignored and indexes nothing."""
    d = loss_cases.inputs("b1_23x41")
    z, zr, disp = d["logits"].cuda(), d["logits_r"].cuda(), d["ests"][0].cuda()
    ref = sa.losses.model_label_loss(z, d["labels"].cuda(), 6, False)
    ref_r = sa.losses.LRSC_loss(zr, [disp], d["labels"].cuda())
    for dt in (torch.uint8, torch.float32, torch.int32):
        y = d["labels"].to(dt).cuda()
        assert torch.equal(sa.losses.model_label_loss(z, y, 6, False), ref), dt
        assert torch.equal(sa.losses.LRSC_loss(zr, [disp], y), ref_r), dt
    stray = d["labels"].clone()
    stray[0, 0, :7] = torch.tensor([-1, 6, 255, -2 ** 40, 2 ** 40, 7, -100])
    as5 = d["labels"].clone()
    as5[0, 0, :7] = 5
    zg = z.clone().requires_grad_(True)
    a = sa.losses.model_label_loss(zg, stray.cuda(), 6, False)
    a.backward()
    zh = z.clone().requires_grad_(True)
    b = sa.losses.model_label_loss(zh, as5.cuda(), 6, False)
    b.backward()
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(zg.grad, zh.grad)


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits(sa):
    d = _shape_inputs(2, 512, 640, 8700)
    a, b = _objective(sa.losses, d, torch.float32, "cuda"), _objective(sa.losses, d, torch.float32, "cuda")
    for k in a:
        assert torch.equal(a[k][0], b[k][0]), k
        for u, v in zip(a[k][1], b[k][1]):
            assert torch.equal(u, v), k
    x, y = _hip_run(sa, d), _hip_run(sa, d)
    for fn in loss_cases.FUNCTIONS:
        assert torch.equal(x[fn][0], y[fn][0]) and all(torch.equal(u, v) for u, v in zip(x[fn][1], y[fn][1])), fn


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_no_host_wait(sa):
    d = _shape_inputs(2, 256, 320, 8800)
    cu = lambda t: t.cuda()                                                                     # noqa: E731
    ests = [cu(t).requires_grad_(True) for t in d["ests"]]
    z, zr = cu(d["logits"]).requires_grad_(True), cu(d["logits_r"]).requires_grad_(True)
    gt, gt4, y = cu(d["gt"]), cu(d["gt4"]), cu(d["labels"])
    sa.losses.train_objective(ests, z, zr, gt, gt4, y, 32, False)[0].backward()              # (library load, workspace query)
    torch.cuda.synchronize()
    before = sa.modules.PATH_COUNTS.get("loss_hip", 0)
    torch.cuda.set_sync_debug_mode("error")
    try:
        raised = False
        try:
            gt.sum().item()
        except RuntimeError:
            raised = True
        if not raised:
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not raise on .item() in this build")
        loss = sa.losses.train_objective(ests, z, zr, gt, gt4, y, 32, False)[0]
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert sa.modules.PATH_COUNTS.get("loss_hip", 0) == before + 3
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(z.grad).all())


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_empty_mask_and_all_ignored_labels_give_nan(sa, fx):
    d = loss_cases.inputs("empty_nan")
    hip = _hip_run(sa, d)
    for fn in ("train", "test", "label"):
        assert np.isnan(fx[f"empty_nan/{fn}/loss64"]) and bool(torch.isnan(hip[fn][0])), fn
        for i, g in enumerate(hip[fn][1]):                       # the reference's gradients there are finite (zeros, and the Dice term's)
            ref = fx[f"empty_nan/{fn}/grad64/{i}"]
            assert bool(torch.isfinite(g).all()) and float((g.double() - torch.from_numpy(ref)).abs().max()) <= 5e-6 * max(float(np.abs(ref).max()), 1e-30)
    assert bool(torch.isfinite(hip["lrsc"][0]))
    loss = sa.losses.train_objective([t.cuda() for t in d["ests"]], d["logits"].cuda(), d["logits_r"].cuda(), d["gt"].cuda(),
                                     d["gt4"].cuda(), d["labels"].cuda(), 32, False)[0]
    assert bool(torch.isnan(loss))


# 8 ------------------------------------------------------------------------------------------------------------------------------
_SCRIPT = '''
def objective(disp_ests, label_est, label_est_r, disp_gt, disp_gt_4, label_true, maxdisp):
    inside = lambda g: (g < maxdisp) & (g >= -maxdisp)
    gts = [disp_gt, disp_gt_4, disp_gt, disp_gt_4]
    consistency = LRSC_loss(label_est_r, disp_ests, label_true)
    disparity = model_loss_train(disp_ests, gts, [inside(g) for g in gts])
    labels = model_label_loss(label_est, label_true, 6, False)
    return disparity + labels + consistency
'''


def test_model_level_training_step(sa, monkeypatch):
    """The stand-in model in train() returns the four disparity maps and both label logits, as the reference does; a script module that
    calls the four loss names from its own globals gets them rebound by install_losses."""
    import standin_model
    from oracle import detdata as dd
    script = types.ModuleType("standin_train_script")
    exec(_SCRIPT, script.__dict__)
    net = standin_model.StandInSemStereo(64, sa.modules).cuda().train()
    left = dd.t_normalish((1, 3, 128, 160), 8901).cuda()
    right = torch.roll(left, shifts=-3, dims=3) + 0.05 * dd.t_normalish((1, 3, 128, 160), 8902).cuda()
    gt, gt4 = dd.t_uniform((1, 128, 160), 8903, -80.0, 80.0).cuda(), dd.t_uniform((1, 32, 40), 8904, -80.0, 80.0).cuda()
    y = torch.from_numpy(np.minimum(np.floor(dd.uniform((1, 128, 160), 8905, 0.0, 6.0)), 5).astype(np.int64)).cuda()
    assert 0.5 <= float(loss_cases.range_mask(gt, 64).float().mean()) <= 0.95
    previous = sa.install(standin_model)
    previous_losses = sa.install_losses(script)
    try:
        sa.accelerate(net)
        before = dict(sa.modules.PATH_COUNTS)
        outs, lab, lab_r = net(left, right)
        loss = script.objective(outs, lab, lab_r, gt, gt4, y, 64)
        loss.backward()
        torch.cuda.synchronize()
        assert sa.modules.PATH_COUNTS.get("loss_hip", 0) == before.get("loss_hip", 0) + 3
        assert sa.modules.PATH_COUNTS.get("loss_torch", 0) == before.get("loss_torch", 0)
        grads = {k: p.grad for k, p in net.named_parameters() if p.grad is not None}
        for k, g in grads.items():
            assert bool(torch.isfinite(g).all()), k
        for prefix in ("head_l.", "head_r.", "ssr_upsample.", "hourglass.", "hourglass_att.", "feature."):
            assert any(k.startswith(prefix) for k in grads), prefix
        missing = [k for k, p in net.named_parameters() if p.requires_grad and p.grad is None]
        assert not missing, missing
        # the same outputs through the composition: float64 on the CPU is the yardstick, fp32 on the CPU the allowance
        det = lambda t, dt: t.detach().cpu().to(dt)                                            # noqa: E731
        vals = {}
        monkeypatch.setattr(sa.engine, "LOSS_HIP", False)
        for dt in (torch.float64, torch.float32):
            vals[dt] = script.objective([det(o, dt) for o in outs], det(lab, dt), det(lab_r, dt), det(gt, dt), det(gt4, dt), y.cpu(), 64)
        _check_one("stand-in step/loss", loss.detach().cpu(), vals[torch.float64], vals[torch.float32])
    finally:
        sa.uninstall(script, previous_losses)
        sa.uninstall(standin_model, previous)
        sa.modules.drop_parked_gates()
