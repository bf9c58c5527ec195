"""`accelerate(model, fuse_forward=True, fuse_training=True)` off the GPU: the switch's bookkeeping (class routing, restore, pickling,
nn.DataParallel replicas, the environment switch) and the hand-off of CPU calls to the model's own forward() with the reference's
return structure -- on the stand-in model (tests/standin_model.py) and, where the reference is mounted, on its real `SemStereo` class
with the stand-in `timm` of tests/test_reference_dropin.py.  The routed forward itself needs the MI355X: tests/test_train_route_gpu.py."""
import copy
import io
import os
import sys

import pytest
import torch
import torch.nn as nn

import semstereo_amd as sa

inst = sys.modules["semstereo_amd.install"]               # (the package attribute `install` is the function of that module)

COMBOS = [(False, True), (True, True), (False, False), (True, False)]          # (att_weights_only, seg_if)


def _standin(att_only=False, seg_if=True):
    import standin_model
    torch.manual_seed(3)
    net = standin_model.StandInSemStereo(64, sa.modules, att_weights_only=att_only, seg_if=seg_if)
    with torch.no_grad():
        net.gamma.fill_(0.25)
    return net.train()


def _images(H=64, W=64):
    g = torch.Generator().manual_seed(5)
    left = torch.randn(2, 3, H, W, generator=g)
    return left, torch.roll(left, shifts=-2, dims=3) + 0.05 * torch.randn(2, 3, H, W, generator=g)


def _flat(out):
    """-> (structure, tensors): the nesting of a forward's return value as nested tuples of shapes / dtypes, and its tensors in order"""
    if isinstance(out, torch.Tensor):
        return (tuple(out.shape), out.dtype), [out]
    assert isinstance(out, (list, tuple)), type(out)
    parts = [_flat(o) for o in out]
    return (type(out).__name__, tuple(p[0] for p in parts)), [t for p in parts for t in p[1]]


def test_default_is_the_hand_off_to_the_models_own_forward():
    net = _standin()
    sa.accelerate(net, fuse_forward=True)
    assert type(net)._ss_fused_forward and not type(net)._ss_fused_training
    calls = net.calls
    out = net(*_images())
    assert net.calls == calls + 1 and len(out) == 3 and len(out[0]) == 4
    sa.restore_forward(net)


@pytest.mark.parametrize("att_only,seg_if", COMBOS)
def test_cpu_calls_are_handed_to_the_reference_forward(att_only, seg_if):
    net = _standin(att_only, seg_if)
    plain = copy.deepcopy(net)
    left, right = _images()
    want_s, want_t = _flat(plain(left, right))
    sa.accelerate(net, fuse_forward=True, fuse_training=True)
    assert type(net)._ss_fused_forward and type(net)._ss_fused_training
    calls, routed = net.calls, sa.modules.PATH_COUNTS.get("train_route", 0)
    out = net(left, right)
    assert net.calls == calls + 1 and sa.modules.PATH_COUNTS.get("train_route", 0) == routed
    got_s, got_t = _flat(out)
    assert got_s == want_s
    if seg_if:
        assert len(out) == 3 and isinstance(out[0], list) and len(out[0]) == (2 if att_only else 4)
    else:
        assert isinstance(out, list) and len(out) == (2 if att_only else 4)
    for g_, w_ in zip(got_t, want_t):
        assert torch.allclose(g_, w_, atol=1e-5, rtol=1e-5)
    # ... and the eval structure in eval() under autograd
    net.eval(); plain.eval()
    assert _flat(net(left, right))[0] == _flat(plain(left, right))[0]
    sa.restore_forward(net)


def test_upgrading_an_inference_routed_model_and_restoring_it():
    import standin_model
    net = _standin()
    sa.accelerate(net, fuse_forward=True)
    first = type(net)
    sa.accelerate(net, fuse_forward=True, fuse_training=True)
    assert type(net) is not first and type(net)._ss_fused_training and type(net)._ss_reference_class is standin_model.StandInSemStereo
    assert "forward" not in net.__dict__ and isinstance(net, standin_model.StandInSemStereo)
    assert type(net) is inst._fused_class(standin_model.StandInSemStereo, training=True)      # one class per reference class
    sa.accelerate(net, fuse_forward=True)                                                     # (no downgrade by a later plain call)
    assert type(net)._ss_fused_training
    sa.restore_forward(net)
    assert type(net) is standin_model.StandInSemStereo
    # fuse_training alone includes the inference routing
    sa.accelerate(net, fuse_training=True)
    assert type(net)._ss_fused_forward and type(net)._ss_fused_training
    sa.restore_forward(net)
    assert type(net) is standin_model.StandInSemStereo


def test_routed_model_pickles_as_the_reference_class():
    import standin_model
    net = _standin()
    sa.accelerate(net, fuse_forward=True, fuse_training=True)
    buf = io.BytesIO()
    torch.save(net, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)
    assert type(back) is standin_model.StandInSemStereo
    assert list(back.state_dict().keys()) == list(net.state_dict().keys())
    assert all(torch.equal(a, b) for a, b in zip(back.state_dict().values(), net.state_dict().values()))
    sa.restore_forward(net)


def test_data_parallel_replicas_share_the_routed_class():
    net = _standin()
    sa.accelerate(net, fuse_forward=True, fuse_training=True)
    replica = net._replicate_for_data_parallel()
    assert type(replica) is type(net) and type(replica)._ss_fused_training and "forward" not in replica.__dict__
    assert replica.forward.__self__ is replica
    dp = nn.DataParallel(net)
    sa.restore_forward(dp)                              # (through the wrapper, as accelerate() accepts it)
    assert not getattr(type(net), "_ss_fused_forward", False)


def test_environment_switch_is_read_at_call_time(monkeypatch):
    from semstereo_amd import engine
    monkeypatch.delenv("SS_FUSE_TRAINING", raising=False)
    assert engine._fuse_training_on()
    monkeypatch.setenv("SS_FUSE_TRAINING", "0")
    assert not engine._fuse_training_on()
    monkeypatch.setenv("SS_FUSE_TRAINING", "1")
    assert engine._fuse_training_on()


def test_route_declines_what_it_is_not_built_for():
    """Half tensors and segmentation-only models reach the reference forward before anything of the route runs (no GPU needed: the
    checks come first)."""
    seen = []
    net = _standin()
    left, right = _images()
    inst.fused_training_forward(net, left.half(), right.half(), reference_forward=lambda l, r: seen.append("half") or "ref")
    net.stereo_if = False
    inst.fused_training_forward(net, left, right, reference_forward=lambda l, r: seen.append("seg-only") or "ref")
    assert seen == ["half", "seg-only"]


# ---- the reference's own class, where it is mounted ---------------------------------------------------------------------------------

from test_reference_dropin import REF, ref_module          # noqa: E402,F401  (the stand-in `timm` and the reference's module, as that file builds them)

needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "models")), reason="reference not mounted")


@needs_reference
@pytest.mark.parametrize("att_only", [False, True])
def test_real_reference_class_cpu_hand_off_and_bookkeeping(ref_module, att_only):
    """(seg_if=False with stereo_if is not a combination the reference can run: `pred_label` is undefined at models/SemStereo.py:311)"""
    torch.manual_seed(0)
    net = ref_module.SemStereo(64, att_only, True, True, 6).train()
    plain = copy.deepcopy(net)
    g = torch.Generator().manual_seed(7)
    left, right = torch.randn(2, 3, 128, 128, generator=g), torch.randn(2, 3, 128, 128, generator=g)
    want_s, want_t = _flat(plain(left, right))
    keys = list(net.state_dict().keys())
    sa.accelerate(net, fuse_forward=True, fuse_training=True, decoder=True, heads=True)
    assert list(net.state_dict().keys()) == keys
    assert type(net)._ss_fused_training and isinstance(net, ref_module.SemStereo) and type(net).__name__ == "SemStereo"
    for name in ("feature", "feature_up", "head_l", "head_r", "chal_0", "chal_1", "chal_2", "chal_3", "chal_4", "spx32_16", "spx16_8",
                 "spx8_4", "spx4_2", "spx2", "ssr_upsample", "stereo_if", "seg_if", "att_weights_only", "maxdisp", "gamma", "beta"):
        assert hasattr(net, name), name            # what fused_training_forward reads
    routed = sa.modules.PATH_COUNTS.get("train_route", 0)
    out = net(left, right)
    assert sa.modules.PATH_COUNTS.get("train_route", 0) == routed
    got_s, got_t = _flat(out)
    assert got_s == want_s and len(out) == 3 and len(out[0]) == (2 if att_only else 4)
    for g_, w_ in zip(got_t, want_t):
        assert torch.allclose(g_, w_, atol=1e-4, rtol=1e-4)
    for (k, a), b in zip(net.state_dict().items(), plain.state_dict().values()):
        if k.endswith("num_batches_tracked"):
            assert torch.equal(a, b), k
    replica = net._replicate_for_data_parallel()
    assert type(replica) is type(net) and replica.forward.__self__ is replica
    buf = io.BytesIO()
    torch.save(net, buf)
    buf.seek(0)
    assert type(torch.load(buf, weights_only=False)) is ref_module.SemStereo
    sa.restore_forward(net)
    assert type(net) is ref_module.SemStereo and "forward" not in net.__dict__
