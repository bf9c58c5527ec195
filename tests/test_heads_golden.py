"""CPU: the head twins (modules.segmenthead, ChalProjection) against tests/golden/heads.npz -- the outputs of the REFERENCE's own
segmenthead and of the `head_l`, `chal_0 .. chal_4` of its SemStereo on the closed-form weights and inputs of golden/heads_cases.py.
On CPU the twins run the reference's statements on the stock layers."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from golden import decoder_cases as dc
from golden import heads_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5
NAMES = ["head_l", "head_r", "chal_0", "chal_1", "chal_2", "chal_3", "chal_4"]


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "heads.npz"))


def _twins(M):
    head = dc.fill(M.segmenthead(128, 32, 6, 2).eval(), hc.HEAD_SALT)
    ragged = dc.fill(M.segmenthead(*hc.RAGGED[0]).eval(), hc.RAGGED_SALT)
    chals = {name: dc.fill(M.ChalProjection(ci, co).eval(), hc.CHAL_SALTS[name])
             for name, ci, co in zip(sorted(hc.CHAL_SALTS), hc.CHAL_IN, hc.CHAL_OUT)}
    return head, ragged, chals


def test_twins_reproduce_the_fixture_on_the_stock_path(fixture):
    import semstereo_amd as sa
    before = dict(sa.modules.PATH_COUNTS)
    with torch.no_grad():
        outs = hc.run_all(*_twins(sa.modules))
    assert sorted(outs) == sorted(fixture.files)
    for key, (t, salt) in outs.items():
        err, rms, dsum, dsq = dc.compare(t, fixture[key], salt)
        tol = TOL * max(1.0, rms)
        assert err <= tol, (key, err, rms)
        assert dsum <= tol and dsq <= 2 * tol, (key, dsum, dsq)  # what the per-element bound implies for the two sums
    assert tuple(outs["head/full"][0].shape) == (1, 6, 64, 96) and tuple(outs["head/ragged"][0].shape) == (1, 5, 12, 18)
    assert sa.modules.PATH_COUNTS["hip"] == before["hip"] and sa.modules.PATH_COUNTS["torch"] == before["torch"] + 3 + 7


def test_fixture_is_small():
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "heads.npz")) <= 512 * 1024


def test_adopt_keeps_the_keys_and_shares_storage():
    import semstereo_amd as sa
    import heads_model
    M = sa.modules
    ref = heads_model.PlainHead(M)
    twin = M.segmenthead.adopt(ref)
    assert list(twin.state_dict().keys()) == list(ref.state_dict().keys()) == list(M.segmenthead(128, 32, 6, 2).state_dict().keys())
    assert "conv1.conv.weight" in twin.state_dict() and "conv1.bn.running_var" in twin.state_dict() and "conv2.bias" in twin.state_dict()
    assert twin.conv1.conv.weight is ref.conv1.conv.weight and twin.conv2.bias is ref.conv2.bias and twin.scale_factor == 2
    seq = nn.Sequential(nn.Conv2d(16, 8, 1), nn.BatchNorm2d(8))
    proj = M.ChalProjection.adopt(seq)
    assert list(proj.state_dict().keys()) == list(seq.state_dict().keys()) == list(M.ChalProjection(16, 8).state_dict().keys())
    assert proj[0].weight is seq[0].weight and proj[1].running_mean is seq[1].running_mean
    x = torch.randn(2, 16, 3, 5)
    seq.eval(), proj.eval()
    with torch.no_grad():
        assert torch.equal(proj(x), seq(x))
        a, b = proj.forward_pair(x, x + 1)
        assert torch.equal(a, seq(x)) and torch.equal(b, seq(x + 1))
    # layouts the twins are not built for are declined
    assert M.segmenthead.adopt(heads_model.PreActHead()) is None
    assert M.ChalProjection.adopt(nn.Conv2d(16, 8, 1)) is None and M.ChalProjection.adopt(nn.Sequential(nn.Conv2d(16, 8, 1))) is None


def test_accelerate_heads_on_the_stand_in():
    import semstereo_amd as sa
    import heads_model
    M = sa.modules
    net = heads_model.HeadsStandIn(64, M, twins=False).eval()
    keys = list(net.state_dict().keys())
    w, b = net.head_l.conv1.conv.weight, net.chal_3[1].running_var
    plain = sa.accelerate(heads_model.HeadsStandIn(64, M, twins=False).eval())
    done = sa.accelerate(net, heads=True)
    assert done == plain + NAMES, done
    assert isinstance(net.head_l, M.segmenthead) and isinstance(net.head_r, M.segmenthead)
    assert all(isinstance(getattr(net, f"chal_{i}"), M.ChalProjection) for i in range(5))
    assert net.head_l.conv1.conv.weight is w and net.chal_3[1].running_var is b
    assert list(net.state_dict().keys()) == keys
    assert sa.accelerate(net, heads=True) == []                  # idempotent
    # without heads=True none of the seven is swapped, with or without the decoder
    for kw in ({}, {"decoder": True}):
        net2 = heads_model.HeadsStandIn(64, M, twins=False).eval()
        done2 = sa.accelerate(net2, **kw)
        assert not set(NAMES) & set(done2)
        assert isinstance(net2.head_l, heads_model.PlainHead) and type(net2.chal_0) is nn.Sequential
    # ... and the adopted modules compute what the plain ones do (CPU: the reference's statements on the shared stock layers)
    net3 = heads_model.HeadsStandIn(64, M, twins=False).eval()
    x = torch.randn(1, 128, 6, 9)
    with torch.no_grad():
        want_h, want_c = net3.head_l(x), net3.chal_0(x)
        sa.accelerate(net3, heads=True)
        assert torch.equal(net3.head_l(x), want_h) and torch.equal(net3.chal_0(x), want_c)


def test_a_pre_activation_head_is_left_alone():
    import semstereo_amd as sa
    import heads_model
    net = heads_model.HeadsStandIn(64, sa.modules, twins=False).eval()
    net.head_l, net.head_r = heads_model.PreActHead(), heads_model.PreActHead()
    pre = net.head_l
    done = sa.accelerate(net, heads=True)
    assert "head_l" not in done and "head_r" not in done and done[-5:] == NAMES[2:]
    assert net.head_l is pre and isinstance(net.head_r, heads_model.PreActHead)


def test_twins_under_autograd_and_in_train_mode_use_the_stock_layers():
    import semstereo_amd as sa
    M = sa.modules
    head, proj = M.segmenthead(16, 32, 6, 2).train(), M.ChalProjection(16, 8).train()
    x = torch.randn(2, 16, 4, 5, requires_grad=True)
    before = dict(M.PATH_COUNTS)
    y = head(x)
    assert isinstance(y, torch.Tensor) and tuple(y.shape) == (2, 6, 8, 10)
    (y.sum() + proj(x).sum()).backward()
    assert x.grad is not None and head.conv1.conv.weight.grad is not None and proj[0].bias.grad is not None
    assert M.PATH_COUNTS["torch"] == before["torch"] + 2 and M.PATH_COUNTS["hip"] == before["hip"]
    assert tuple(M.segmenthead(16, 32, 6)(x).shape) == (2, 6, 4, 5)       # scale_factor None: no up-sampling
