"""CPU: the 2-D decoder twins (modules.Conv2x, FeatUp, Spx2) against tests/golden/decoder.npz -- the outputs of the REFERENCE's own
Conv2x, FeatUp and SemStereo.spx* on the closed-form weights and inputs of golden/decoder_cases.py.  On CPU the twins run the
reference's statements on the stock layers, so the only difference is thread-order rounding: 1e-6."""
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from golden import decoder_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
TOL = 1e-6
EXTRA = ["feature_up", "spx32_16", "spx16_8", "spx8_4", "spx4_2", "spx2"]


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "decoder.npz"))


def _check(t, rec, salt, what):
    err, rms, dsum, dsq = dc.compare(t, rec, salt)
    tol = TOL * max(1.0, rms)
    assert err <= tol, (what, err, rms)
    assert dsum <= tol and dsq <= 2 * tol, (what, dsum, dsq)  # what the per-element bound implies for the two sums


def test_conv2x_cases(fixture):
    import semstereo_amd as sa
    before = dict(sa.modules.PATH_COUNTS)
    with torch.no_grad():
        for n, (B, Cin, Cout, H, W, Hr, Wr) in dc.CONV2X.items():
            mod = dc.fill(sa.modules.Conv2x(Cin, Cout, deconv=True).eval(), dc.conv2x_salt(n))
            x, rem = dc.conv2x_inputs(n)
            _check(mod(x, rem), fixture[f"conv2x/{n}"], 0, n)
    assert sa.modules.PATH_COUNTS["hip"] == before["hip"] and sa.modules.PATH_COUNTS["torch"] == before["torch"] + 4


def test_featup(fixture):
    import semstereo_amd as sa
    fu = dc.fill(sa.modules.FeatUp().eval(), dc.FEATUP_SALT)
    featL, featR = dc.featup_inputs()
    with torch.no_grad():
        L, R = fu(featL, featR)
    assert isinstance(L, list) and isinstance(R, list) and len(L) == len(R) == 5
    assert L[4] is featL[4] and R[4] is featR[4]                 # x32 / y32 pass through (models/SemStereo.py:86)
    for side, maps in (("L", L), ("R", R)):
        for k, t in enumerate(maps):
            _check(t, fixture[f"featup/{side}{k}"], 10 + k, f"{side}{k}")


def test_spx_chain_and_spx2(fixture):
    import semstereo_amd as sa
    M = sa.modules
    mods = {"spx32_16": M.Conv2x(256, 384, True), "spx16_8": M.Conv2x(768, 256, True), "spx8_4": M.Conv2x(512, 128, True),
            "spx4_2": M.Conv2x(256, 64, True), "spx2": M.Spx2(128, 6)}
    for name, salt in dc.SPX_SALTS.items():
        dc.fill(mods[name].eval(), salt)
    with torch.no_grad():
        outs = dc.run_spx(mods, dc.spx_inputs())
    assert tuple(outs[4].shape) == (1, 6, 64, 96)
    for k, t in enumerate(outs):
        _check(t, fixture[f"spx/{k}"], 20 + k, f"spx/{k}")


def test_twins_under_autograd_and_in_train_mode_use_the_stock_layers():
    import semstereo_amd as sa
    mod = dc.fill(sa.modules.Conv2x(16, 8, deconv=True), 3).train()
    x, rem = torch.randn(2, 16, 4, 4, requires_grad=True), torch.randn(2, 8, 8, 8)
    before = dict(sa.modules.PATH_COUNTS)
    mod(x, rem).sum().backward()
    assert x.grad is not None and mod.conv1.conv.weight.grad is not None
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"] + 2 and sa.modules.PATH_COUNTS["hip"] == before["hip"]
    # the other forms of the reference's Conv2x keep working: no concat, the strided conv, the 3-D form
    y = sa.modules.Conv2x(8, 8, deconv=False, concat=False)(torch.randn(1, 8, 8, 8), torch.randn(1, 8, 4, 4))
    assert tuple(y.shape) == (1, 8, 4, 4)
    y = sa.modules.Conv2x(4, 4, deconv=True, is_3d=True)(torch.randn(1, 4, 2, 4, 4), torch.randn(1, 4, 4, 8, 8))
    assert tuple(y.shape) == (1, 8, 4, 8, 8)
    y = sa.modules.Conv2x(4, 4, deconv=True, is_3d=True, keep_dispc=True)(torch.randn(1, 4, 3, 4, 4), torch.randn(1, 4, 3, 8, 8))
    assert tuple(y.shape) == (1, 8, 3, 8, 8)


def test_accelerate_decoder_on_the_stand_in():
    import semstereo_amd as sa
    import decoder_model
    net = decoder_model.DecoderStandIn(64, sa.modules, twins=False).eval()
    keys = list(net.state_dict().keys())
    w = net.feature_up.deconv16_8.conv1.conv.weight
    b = net.spx2[0].bias
    done = sa.accelerate(net, decoder=True)
    assert done[-6:] == EXTRA and not set(EXTRA) & set(done[:-6]), done
    assert isinstance(net.feature_up, sa.modules.FeatUp) and isinstance(net.spx8_4, sa.modules.Conv2x) and isinstance(net.spx2, sa.modules.Spx2)
    assert net.feature_up.deconv16_8.conv1.conv.weight is w and net.spx2[0].bias is b
    assert list(net.state_dict().keys()) == keys
    assert sa.accelerate(net, decoder=True) == []                # idempotent
    # without decoder=True the list is what it always was, and the decoder is left alone
    net2 = decoder_model.DecoderStandIn(64, sa.modules, twins=False).eval()
    done2 = sa.accelerate(net2)
    assert not set(EXTRA) & set(done2) and done2 == done[:-6]
    assert isinstance(net2.feature_up, decoder_model.PlainFeatUp) and not isinstance(net2.spx2, sa.modules.Spx2)
    # ... and the adopted model computes what the plain one does (CPU: the reference's statements on the shared stock layers)
    net3 = decoder_model.DecoderStandIn(64, sa.modules, twins=False).eval()
    feats = [torch.randn(1, c, 64 >> (k + 1), 96 >> (k + 1)) for k, c in enumerate(dc.CHANS)]
    with torch.no_grad():
        want = net3.feature_up(feats, feats)[0][0]
        sa.accelerate(net3, decoder=True)
        got = net3.feature_up(feats, feats)[0][0]
    assert torch.allclose(got, want, atol=1e-5, rtol=1e-5)


# ---- against the reference's own classes (build container only) ----

@pytest.fixture(scope="module")
def ref_module():
    if not os.path.isdir(os.path.join(REF, "models")):
        pytest.skip("reference not mounted")

    class _Backbone(nn.Module):            # attribute surface Feature() reads (models/SemStereo.py:37-45)
        def __init__(self):
            super().__init__()
            mk = lambda i, o, s: nn.Sequential(nn.Conv2d(i, o, 3, s, 1, bias=False), nn.BatchNorm2d(o), nn.SiLU())
            self.stem = mk(3, 32, 2)
            self.stages_0 = nn.Sequential(mk(32, 64, 1)); self.stages_1 = nn.Sequential(mk(64, 128, 2))
            self.stages_2 = nn.Sequential(mk(128, 256, 2)); self.stages_3 = nn.Sequential(mk(256, 384, 2))
            self.stages_4 = nn.Sequential(mk(384, 512, 2))
    saved = {k: sys.modules.get(k) for k in ("timm", "models")}
    timm = types.ModuleType("timm")
    timm.create_model = lambda *a, **k: _Backbone()
    sys.modules["timm"] = timm
    pkg = types.ModuleType("models")
    pkg.__path__ = [os.path.join(REF, "models")]
    sys.modules["models"] = pkg
    sys.path.insert(0, REF)
    import importlib
    ms = importlib.import_module("models.SemStereo")
    yield ms
    sys.path.remove(REF)
    for k in [k for k in sys.modules if k.startswith("models.")]:
        sys.modules.pop(k)
    for k, v in saved.items():
        if v is None:
            sys.modules.pop(k, None)
        else:
            sys.modules[k] = v


def test_state_dict_keys_equal_the_reference_classes(ref_module):
    import importlib
    import semstereo_amd as sa
    sub = importlib.import_module("models.submodule")
    for args, kw in (((20, 12), dict(deconv=True)), ((8, 8), dict(deconv=False, concat=False)), ((16, 8), dict(deconv=True, keep_concat=False)),
                     ((4, 4), dict(deconv=True, is_3d=True)), ((4, 4), dict(deconv=True, is_3d=True, keep_dispc=True))):
        ref, twin = sub.Conv2x(*args, **kw), sa.modules.Conv2x(*args, **kw)
        assert [(k, tuple(v.shape)) for k, v in ref.state_dict().items()] == [(k, tuple(v.shape)) for k, v in twin.state_dict().items()], kw
        assert list(sa.modules.Conv2x.adopt(ref).state_dict().keys()) == list(ref.state_dict().keys())
    ref, twin = ref_module.FeatUp(), sa.modules.FeatUp()
    assert [(k, tuple(v.shape)) for k, v in ref.state_dict().items()] == [(k, tuple(v.shape)) for k, v in twin.state_dict().items()]
    net = ref_module.SemStereo(64, False, True, True, 6)
    assert [(k, tuple(v.shape)) for k, v in net.spx2.state_dict().items()] == [(k, tuple(v.shape)) for k, v in sa.modules.Spx2(128, 6).state_dict().items()]


def test_accelerate_decoder_on_the_real_reference_model(ref_module):
    import semstereo_amd as sa
    torch.manual_seed(0)
    net = ref_module.SemStereo(64, False, True, True, 6).eval()
    keys = list(net.state_dict().keys())
    plain = sa.accelerate(ref_module.SemStereo(64, False, True, True, 6).eval())
    imgL, imgR = torch.randn(1, 3, 128, 128), torch.randn(1, 3, 128, 128)
    with torch.no_grad():
        (want,), _ = net(imgL, imgR)
    w = net.feature_up.deconv4_2.conv2.conv.weight
    done = sa.accelerate(net, decoder=True)
    assert done == plain + EXTRA
    assert net.feature_up.deconv4_2.conv2.conv.weight is w and list(net.state_dict().keys()) == keys
    (got,), _ = net(imgL, imgR)            # (autograd on: every twin takes its PyTorch path, which is what a CPU can run)
    assert torch.allclose(got.detach(), want, atol=1e-4, rtol=1e-4)
