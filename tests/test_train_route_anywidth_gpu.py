"""The routed train() call (`accelerate(model, fuse_forward=True, fuse_training=True)`) at 128 x 160 -- W/4 = 40, no multiple of 64 --
with `train.CONCAT_VOLUME_ANY_WIDTH` on: models/SemStereo.py:316-318 runs as the one-launch `train.concat_volume_sampled` instead of
the three statements that tests/test_train_route_gpu.py counts at this size by default, and the call is held to that file's bounds
against a float64 CPU run of the same model on the oracle op library.  Two runs, computed once.  Run on the MI355X box: pytest -m gpu."""
import copy

import pytest
import torch

from test_train_route_gpu import PX, _build, _images, _scalar, _snapshot

pytestmark = pytest.mark.gpu

H, W = 128, 160
_RUN = {}


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    return semstereo_amd


@pytest.fixture(scope="module")
def runs(sa):
    """float64 on the CPU, and the routed forward with the switch on"""
    net, _ = _build(sa, att_weights_only=False)
    net.train()
    left, right = _images(1, H, W)
    ref = copy.deepcopy(net).cpu().double().train()
    out = ref(left.cpu().double(), right.cpu().double())
    _scalar(out).backward()
    _RUN["f64"] = _snapshot(ref, out)
    sa.modules.drop_parked_gates()
    del ref, out
    keys = ("torch", "hip_train", "train_route", "train_tail_statements", "train_concat_statements")
    counts = lambda: {k: sa.modules.PATH_COUNTS.get(k, 0) for k in keys}          # noqa: E731
    routed = copy.deepcopy(net)
    sa.accelerate(routed, fuse_forward=True, fuse_training=True)
    previous, sa.train.CONCAT_VOLUME_ANY_WIDTH = sa.train.CONCAT_VOLUME_ANY_WIDTH, True
    try:
        calls, before = routed.calls, counts()
        out = routed(left, right)
        after = counts()
        _scalar(out).backward()
        torch.cuda.synchronize()
    finally:
        sa.train.CONCAT_VOLUME_ANY_WIDTH = previous
    _RUN["routed"] = _snapshot(routed, out)
    _RUN["routed_calls"] = routed.calls - calls
    _RUN["routed_counts"] = {k: after[k] - before[k] for k in after}
    yield _RUN
    _RUN.clear()


def test_no_statement_of_the_concat_volume_runs(runs):
    c = runs["routed_counts"]
    print(c)
    assert runs["routed_calls"] == 0, "the model's own forward() ran"
    assert c["train_route"] == 1 and c["torch"] == 0, c
    assert c["train_tail_statements"] == 0 and c["train_concat_statements"] == 0, c
    assert c["hip_train"] > 0, c


def test_outputs_against_float64(runs):
    """per estimate at most 0.5 % of the pixels beyond 4e-3 px of the float64 run"""
    assert len(runs["routed"]["outs"]) == len(runs["f64"]["outs"]) == 4
    for name, o, o64 in zip(("pred_up", "pred", "pred_att_up", "pred_att"), runs["routed"]["outs"], runs["f64"]["outs"]):
        e = (o.double() - o64).abs()
        far = float((e > PX).double().mean())
        print(name, dict(median=float(e.median()), share_beyond_4e_3=far, max=float(e.max())))
        assert bool(torch.isfinite(o).all()) and far <= 0.005, (name, far)


def test_gradients_against_float64(runs):
    """tests/test_train_route_gpu.py's bounds: per parameter max |g - g64| / max |g64|: median <= 5e-3, worst <= 5e-2; gamma / beta
    within 1e-4 of the overall gradient scale"""
    from test_train_route_gpu import _BIAS_SCALE
    g64, grads = runs["f64"]["grads"], runs["routed"]["grads"]
    assert set(grads) == set(g64)
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    gscale = max(float(g.abs().max()) for g in g64.values())
    errs = {k: float((g.double() - g64[k]).abs().max()) / (float(g64[_BIAS_SCALE.get(k, k)].abs().max()) + 1e-12) for k, g in grads.items()}
    scalars = {k: float((grads[k].double() - g64[k]).abs().max()) / gscale for k in ("gamma", "beta")}
    for k in scalars:
        errs.pop(k)
    vals = sorted(errs.values())
    s = dict(median=vals[len(vals) // 2], worst=vals[-1], worst_parameter=max(errs, key=errs.get), **scalars)
    print(s)
    assert s["median"] <= 5e-3 and s["worst"] <= 5e-2, s
    assert s["gamma"] <= 1e-4 and s["beta"] <= 1e-4, s


def test_batchnorm_calls_tracked(runs):
    b64, br = runs["f64"]["buffers"], runs["routed"]["buffers"]
    assert list(b64) == list(br)
    tracked = 0
    for k in b64:
        if k.endswith("num_batches_tracked"):
            assert int(b64[k]) == int(br[k]), (k, int(b64[k]), int(br[k]))
            tracked += int(br[k])
    assert tracked > 0
