"""The segmentation heads and the chal_* projections on HIP (csrc/seghead_f16s.hip, csrc/proj2d_f16s.hip): per-layer error against
float64 with the fp32 CPU layer as the yardstick, element-wise bounds on edge shapes, bit identities, NaN / Inf containment, the twins
against tests/golden/heads.npz, a whole forward, the cache and the switches.  Run on the MI355X box: pytest -m gpu."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from golden import decoder_cases as dc
from golden import heads_cases as hc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (Cin, Cout) of chal_0 .. chal_4 (models/SemStereo.py:196-197, 213-217)
CHALS = [(128, 64), (256, 128), (512, 256), (768, 384), (512, 256)]


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    assert semstereo_amd.engine.CONV_ENGINE == "f16x3"
    return semstereo_amd


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _judge(name, hip, cpu32, truth):
    """HIP rms error <= 2x the fp32 CPU layer's, max-abs <= 4x its max-abs, both against float64."""
    eh, ec = (hip.double() - truth).abs(), (cpu32.double() - truth).abs()
    rh, rc = float(eh.pow(2).mean().sqrt()), float(ec.pow(2).mean().sqrt())
    mh, mc = float(eh.max()), float(ec.max())
    line = f"{name:44s} rms hip {rh:.3e} cpu {rc:.3e} ratio {rh / rc:5.2f} | max hip {mh:.3e} cpu {mc:.3e} ratio {mh / mc:5.2f}"
    print(line)
    return rh <= 2.0 * rc and mh <= 4.0 * mc, line


def _bound(x, w, scale, K, padding=0):
    """|error| the two-term fp16 form may have against the exact layer: per product 2^-21 (two operand representations at 2^-23 and
    the dropped lo*lo at 2^-22), a K-term fp32 accumulation as a random walk with a factor 4, and two roundings of the affine --
    all relative to sum |x| |w| (times |scale|)."""
    S = F.conv2d(x.double().abs(), w.double().abs(), None, 1, padding)
    if scale is not None:
        S = S * scale.double().abs()[None, :, None, None]
    return (2.0 ** -21 + 4.0 * K ** 0.5 * 2.0 ** -24) * S + 1e-30


def _proj_params(Cin, Cout, seed, shift_only=False):
    g = _gen(seed)
    w = (torch.rand(Cout, Cin, 1, 1, generator=g) * 2 - 1) * (3.0 / Cin) ** 0.5
    if shift_only:
        return w, None, torch.rand(Cout, generator=g) * 0.2 - 0.1
    return w, torch.rand(Cout, generator=g) * 0.8 + 0.6, torch.rand(Cout, generator=g) * 0.2 - 0.1


def _affine(y, scale, shift, relu):
    if scale is not None:
        y = y * scale.to(y.dtype)[None, :, None, None]
    if shift is not None:
        y = y + shift.to(y.dtype)[None, :, None, None]
    return F.relu(y) if relu else y


def _proj_ref(x, w, scale, shift, relu, dtype):
    return _affine(F.conv2d(x.to(dtype), w.to(dtype)), scale, shift, relu)


def _hip_proj(sa, x, w, scale, shift, relu, xb=None):
    E = sa.engine
    ws = E.pack_conv2d_k1_weight(w.cuda())
    c = lambda t: None if t is None else t.cuda().contiguous()
    return E.conv2d_k1_f16s_hip(x, ws, w.shape[0], c(scale), c(shift), relu, xb=xb)


# ---- 4. projection error against float64 ----

@pytest.mark.parametrize("layer", CHALS, ids=[f"{a}to{b}" for a, b in CHALS])
def test_projection_error_against_float64(sa, layer):
    Cin, Cout = layer
    w, scale, shift = _proj_params(Cin, Cout, 100 + Cin + Cout)
    x = torch.randn(1, Cin, 16, 24, generator=_gen(7 + Cin))
    hip = _hip_proj(sa, x.cuda(), w, scale, shift, False).cpu()
    assert tuple(hip.shape) == (1, Cout, 16, 24)
    ok, line = _judge(f"chal {Cin}->{Cout} @16x24", hip, _proj_ref(x, w, scale, shift, False, torch.float32),
                      _proj_ref(x, w, scale, shift, False, torch.float64))
    assert ok, line


# ---- 5. projection edge shapes ----

def _check_proj_bound(sa, x, w, scale, shift, relu, what):
    got = _hip_proj(sa, x.cuda(), w, scale, shift, relu).cpu().double()
    want = _proj_ref(x, w, scale, shift, relu, torch.float64)
    assert got.shape == want.shape
    excess = ((got - want).abs() - _bound(x, w, scale, x.shape[1]) - 2.0 ** -22 * want.abs()).max()
    print(what, "max error", float((got - want).abs().max()), "excess over the bound", float(excess))
    assert float(excess) <= 0.0, (what, float(excess))


@pytest.mark.parametrize("Cin", [8, 24, 768])
@pytest.mark.parametrize("Cout", [1, 6, 33, 384])
def test_projection_edge_shapes(sa, Cin, Cout):
    for (H, W) in ((1, 1), (1, 31), (1, 33), (35, 37)):
        x = torch.randn(3, Cin, H, W, generator=_gen(H * W + Cin))
        for mode in ("relu", "plain", "shift_only"):
            w, scale, shift = _proj_params(Cin, Cout, Cin * 7 + Cout + W, shift_only=(mode == "shift_only"))
            _check_proj_bound(sa, x, w, scale, shift, mode == "relu", (Cin, Cout, H * W, mode))


# maps with at least 256 position tiles keep 256 / 384 channels in one workgroup (two / three channel tiles per wave): ragged ends
WIDE = [(8, 200, 129, 127), (24, 384, 127, 130), (8, 257, 128, 128)]


@pytest.mark.parametrize("shape", WIDE, ids=["x".join(map(str, s)) for s in WIDE])
def test_projection_wide_tiles(sa, shape):
    Cin, Cout, H, W = shape
    assert -(-H * W // 64) >= 256 and Cout > 128
    w, scale, shift = _proj_params(Cin, Cout, Cin + Cout)
    _check_proj_bound(sa, torch.randn(2, Cin, H, W, generator=_gen(H)), w, scale, shift, True, shape)


# ---- 6. projection bit identities ----

IDENT = [(768, 384, 16, 24), (256, 128, 5, 7), (24, 33, 9, 70), (24, 384, 127, 130), (8, 200, 129, 127)]


@pytest.mark.parametrize("shape", IDENT, ids=["x".join(map(str, s)) for s in IDENT])
def test_projection_batch_and_pair_bit_identities(sa, shape):
    Cin, Cout, H, W = shape
    w, scale, shift = _proj_params(Cin, Cout, 400 + Cin)
    g = _gen(Cin + W)
    xa, xb = torch.randn(1, Cin, H, W, generator=g).cuda(), (torch.randn(1, Cin, H, W, generator=g) * 37.0).cuda()
    one_a, one_b = _hip_proj(sa, xa, w, scale, shift, True), _hip_proj(sa, xb, w, scale, shift, True)
    pair = _hip_proj(sa, xa, w, scale, shift, True, xb=xb)
    assert tuple(pair.shape) == (2, Cout, H, W)
    assert torch.equal(pair[:1], one_a) and torch.equal(pair[1:], one_b), shape
    x3 = torch.cat((xb, xa, (torch.randn(1, Cin, H, W, generator=g) * 1e3).cuda()), 0)
    b3 = _hip_proj(sa, x3, w, scale, shift, True)
    assert torch.equal(b3[1:2], one_a) and torch.equal(b3[:1], one_b), shape


# ---- 7. projection NaN / Inf ----

def test_projection_nan_and_inf_stay_in_their_position(sa):
    Cin, Cout, H, W = 24, 33, 6, 40
    w, scale, shift = _proj_params(Cin, Cout, 9)
    x = torch.randn(2, Cin, H, W, generator=_gen(9))
    clean = _hip_proj(sa, x.cuda(), w, scale, shift, False).cpu()
    hit = torch.zeros(2, Cout, H, W, dtype=torch.bool)
    hit[1, :, 2, 17] = True
    for bad in (float("nan"), float("inf"), -float("inf")):
        for relu in (False, True):
            xb = x.clone()
            xb[1, 3, 2, 17] = bad
            got = _hip_proj(sa, xb.cuda(), w, scale, shift, relu).cpu()
            if relu and bad != bad:
                assert bool(torch.isnan(got[hit]).all())         # a NaN survives the ReLU, as in F.relu
            if not relu:
                assert bool((~torch.isfinite(got[hit])).all()), bad
            want = F.relu(clean) if relu else clean
            assert torch.equal(got[~hit], want[~hit]), (bad, relu)


# ---- 8. the head against float64 ----

def _head(sa, Cin, seed, K=6, scale_factor=2):
    head = sa.modules.segmenthead(Cin, 32, K, scale_factor)
    g = _gen(seed)
    with torch.no_grad():
        head.conv1.conv.weight.copy_((torch.rand(32, Cin, 3, 3, generator=g) * 2 - 1) * (3.0 / (9 * Cin)) ** 0.5)
        head.conv1.bn.weight.copy_(torch.rand(32, generator=g) * 0.8 + 0.6)
        head.conv1.bn.running_var.copy_(torch.rand(32, generator=g) * 0.8 + 0.6)
        head.conv1.bn.bias.copy_(torch.rand(32, generator=g) * 0.2 - 0.1)
        head.conv1.bn.running_mean.copy_(torch.rand(32, generator=g) * 0.2 - 0.1)
        head.conv2.weight.copy_((torch.rand(K, 32, 1, 1, generator=g) * 2 - 1) * (3.0 / 32) ** 0.5)
        head.conv2.bias.copy_(torch.rand(K, generator=g) * 0.2 - 0.1)
    return head.eval()


def _head_hip(sa, head, x):
    dev = copy.deepcopy(head).cuda().eval()
    with torch.no_grad():
        y = sa.engine.run_seghead(dev, dev, x.cuda())
    assert y is not None
    return y.cpu()


def _head_cpu(head, x, dtype):
    with torch.no_grad():
        return copy.deepcopy(head).to(dtype)._forward_now(x.to(dtype))


def test_head_error_against_float64(sa):
    head = _head(sa, 128, 21)
    x = torch.randn(1, 128, 32, 48, generator=_gen(22))
    hip = _head_hip(sa, head, x)
    assert tuple(hip.shape) == (1, 6, 64, 96)
    ok, line = _judge("segmenthead 128->32->6 @32x48", hip, _head_cpu(head, x, torch.float32), _head_cpu(head, x, torch.float64))
    assert ok, line


HEAD_SHAPES = [(2, 128, 5, 7), (1, 128, 37, 70), (3, 16, 1, 1)]


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=["x".join(map(str, s)) for s in HEAD_SHAPES])
def test_head_bound_against_float64(sa, shape):
    B, Cin, H, W = shape
    head = _head(sa, Cin, 30 + Cin + W)
    x = torch.randn(B, Cin, H, W, generator=_gen(W + Cin))
    got = _head_hip(sa, head, x).double()
    want = _head_cpu(head, x, torch.float64)
    assert got.shape == want.shape == (B, 6, 2 * H, 2 * W)
    h64 = copy.deepcopy(head).double()
    bn = h64.conv1.bn
    scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    with torch.no_grad():
        y1 = F.relu(bn(h64.conv1.conv(x.double())))
        # the first stage's bound (the projection tests' bound with K = 9 Cin; the ReLU does not enlarge an error) ...
        b1 = _bound(x, h64.conv1.conv.weight, scale, 9 * Cin, padding=1) + 2.0 ** -22 * y1.abs()
        # ... through the 32 -> 6 contraction in fp32 and through the up-sampling, a convex combination
        w2 = h64.conv2.weight.abs()
        b2 = F.conv2d(b1, w2) + 32 * 2.0 ** -24 * F.conv2d(y1.abs(), w2)
        bound = F.interpolate(b2, size=(2 * H, 2 * W), mode="bilinear", align_corners=False) + 2.0 ** -22 * want.abs()
    excess = ((got - want).abs() - bound).max()
    print(shape, "max error", float((got - want).abs().max()), "excess over the bound", float(excess))
    assert float(excess) <= 0.0, (shape, float(excess))


# ---- 9. the up-sample kernel alone ----

@pytest.mark.parametrize("shape", [(2, 6, 1, 1), (1, 6, 5, 7), (1, 3, 33, 65), (2, 6, 9, 70)], ids=str)
def test_bilinear_up2(sa, shape):
    B, C, H, W = shape
    x = torch.randn(shape, generator=_gen(H + W))
    got = sa.engine.bilinear_up2_hip(x.cuda()).cpu()
    want = F.interpolate(x.double(), size=(2 * H, 2 * W), mode="bilinear", align_corners=False)
    assert got.shape == want.shape
    assert float((got.double() - want).abs().max()) <= 2.0 ** -22 * float(x.abs().max())
    const = torch.full(shape, 0.7311, dtype=torch.float32)
    assert torch.equal(sa.engine.bilinear_up2_hip(const.cuda()).cpu(), torch.full((B, C, 2 * H, 2 * W), 0.7311, dtype=torch.float32))


# ---- 10. head bit identities ----

def test_head_batch_bit_identity(sa):
    head = _head(sa, 128, 41)
    g = _gen(42)
    xs = [torch.randn(1, 128, 19, 45, generator=g) * s for s in (1.0, 50.0, 1e-3)]
    alone = [_head_hip(sa, head, x) for x in xs]
    batch = _head_hip(sa, head, torch.cat(xs, 0))
    for i in range(3):
        assert torch.equal(batch[i:i + 1], alone[i]), i


# ---- 11. the fixture on HIP ----

def test_twins_against_the_reference_fixture(sa):
    M, fx = sa.modules, np.load(os.path.join(ROOT, "tests", "golden", "heads.npz"))
    head = dc.fill(M.segmenthead(128, 32, 6, 2).eval(), hc.HEAD_SALT).cuda()
    ragged = dc.fill(M.segmenthead(*hc.RAGGED[0]).eval(), hc.RAGGED_SALT).cuda()
    chals = {name: dc.fill(M.ChalProjection(ci, co).eval(), hc.CHAL_SALTS[name]).cuda()
             for name, ci, co in zip(sorted(hc.CHAL_SALTS), hc.CHAL_IN, hc.CHAL_OUT)}
    before = dict(M.PATH_COUNTS)
    with torch.no_grad():
        outs = {key: (sa.deferred.real(t), salt) for key, (t, salt) in hc.run_all(head, ragged, chals).items()}
    assert sorted(outs) == sorted(fx.files)
    assert M.PATH_COUNTS["hip"] == before["hip"] + 2 + 7 and M.PATH_COUNTS["torch"] == before["torch"] + 1     # the ragged head
    for key, (t, salt) in outs.items():
        err, rms, dsum, dsq = dc.compare(t, fx[key], salt)
        tol = 1e-5 * max(1.0, rms)
        print(f"fixture {key}: max err {err:.2e}, rms {rms:.3f}, sum {dsum:.2e}, sum of squares {dsq:.2e} (tolerance {tol:.1e})")
        assert err <= tol, (key, err, rms)
        assert dsum <= tol and dsq <= 2 * tol, (key, dsum, dsq)  # what the per-element bound implies for the two sums


# ---- 12. a whole forward ----

def _model(sa):
    import heads_model
    from oracle import detdata as dd
    net = heads_model.HeadsStandIn(64, sa.modules, twins=True, head_twins=False)
    with torch.no_grad():
        for i, (name, t) in enumerate(sorted(list(net.named_parameters()) + list(net.named_buffers()))):
            if name.endswith("num_batches_tracked") or name in ("gamma", "beta"):
                continue
            if name.endswith("running_var") or (name.endswith(".weight") and t.dim() == 1):
                t.copy_(dd.t_uniform(tuple(t.shape), 900 + i, 0.6, 1.4))
            elif t.dim() == 1:
                t.copy_(dd.t_uniform(tuple(t.shape), 900 + i, -0.1, 0.1))
            else:
                if ".conv5.0." in name or ".conv6.0." in name:
                    fan_in = t.shape[0] * 27 // 8
                elif t.dim() == 4 and t.shape[2] == 4:
                    fan_in = t.shape[0] * 4
                else:
                    fan_in = t[0].numel()
                a = (3.0 / fan_in) ** 0.5
                t.copy_(dd.t_uniform(tuple(t.shape), 900 + i, -a, a))
    return net.cuda().eval()


def test_whole_forward_with_the_heads_on_hip(sa, monkeypatch):
    import standin_model
    previous = sa.install(standin_model)                         # the stand-in looks its op library up by bare name, as the reference does
    try:
        _whole_forward(sa, monkeypatch)
    finally:
        sa.uninstall(standin_model, previous)


def _whole_forward(sa, monkeypatch):
    from oracle import detdata as dd
    M, E = sa.modules, sa.engine
    # (`semstereo_amd.install` is the function; the module of the same name holds the fused forward)
    fused_forward = __import__("importlib").import_module("semstereo_amd.install").fused_inference_forward
    net = _model(sa)
    left = dd.t_normalish((1, 3, 256, 384), 951)
    right = torch.roll(left, shifts=-3, dims=3) + 0.05 * dd.t_normalish((1, 3, 256, 384), 952)
    left, right = left.cuda(), right.cuda()
    done = sa.accelerate(net, decoder=True, heads=True)          # (the reference-order forward of the stand-in, not the fused one)
    assert done == ["head_l", "head_r", "chal_0", "chal_1", "chal_2", "chal_3", "chal_4"]
    symbols = []
    real_call = E.call
    monkeypatch.setattr(E, "call", lambda name, *a: (symbols.append(name), real_call(name, *a))[1])
    with torch.no_grad():
        net(left, right)                                         # (packs the weights)
        torch.cuda.synchronize()
        before = dict(M.PATH_COUNTS)
        del symbols[:]
        (d1,), lab1 = net(left, right)
        assert isinstance(lab1, torch.Tensor) and tuple(lab1.shape) == (1, 6, 256, 384)
        assert M.PATH_COUNTS["torch"] == before["torch"]
        assert M.PATH_COUNTS["hip"] >= before["hip"] + 1 + 7
        # head_r's result is never read in an eval forward: it is never launched
        assert symbols.count("ss_seghead_logits_fwd") == 1 and symbols.count("ss_bilinear_up2_fwd") == 1, symbols
        assert symbols.count("ss_conv2d_k1_f16s_fwd") == 7 and "ss_conv2d_k1_f16s_pair_fwd" not in symbols
        E.HEADS_HIP = False
        try:
            mid = dict(M.PATH_COUNTS)
            (d0,), lab0 = net(left, right)
            assert M.PATH_COUNTS["torch"] >= mid["torch"] + 1 + 7
            (d0f,), _ = fused_forward(net, left, right)
        finally:
            E.HEADS_HIP = "auto"
        # the fused inference forward sends both views of chal_1 / chal_2 through one launch each
        del symbols[:]
        (d2,), lab2 = fused_forward(net, left, right)
        assert symbols.count("ss_conv2d_k1_f16s_pair_fwd") == 2 and symbols.count("ss_conv2d_k1_f16s_fwd") == 3
        assert symbols.count("ss_seghead_logits_fwd") == 1
        assert torch.equal(lab2, lab1)
    assert d1.shape == d0.shape == (1, 256, 384)
    for name, d, dref in (("reference-order", d1, d0), ("fused", d2, d0f)):
        err = (d - dref).abs()
        print(f"whole forward ({name}): median", float(err.median()), "max", float(err.max()), "label max", float((lab1 - lab0).abs().max()))
        # the SSR head's tolerance (test_dropin_gpu): full-resolution disparities (x4), 1e-3 px at 1/4 scale = 4e-3 here
        assert float(err.median()) <= 1e-4 and float((err <= 4e-3).float().mean()) >= 0.995, (name, float(err.median()), float(err.max()))
    assert float((lab1 - lab0).abs().max()) <= 1e-4 * max(1.0, float(lab0.abs().max()))
    # train(): batch statistics -- both heads and the projections run the stock layers, and the forward returns three values
    net.train()
    try:
        mid = dict(M.PATH_COUNTS)
        del symbols[:]
        out = net(left, right)
        assert len(out) == 3 and all(isinstance(t, torch.Tensor) and tuple(t.shape) == (1, 6, 256, 384) for t in out[1:])
        assert M.PATH_COUNTS["torch"] >= mid["torch"] + 2 + 7
        assert "ss_seghead_logits_fwd" not in symbols and "ss_conv2d_k1_f16s_fwd" not in symbols
    finally:
        net.eval()


# ---- 13. the cache ----

def test_cache_follows_the_weights(sa):
    M, dfr = sa.modules, sa.deferred
    head = copy.deepcopy(_head(sa, 16, 61)).cuda().eval()
    proj = dc.fill(M.ChalProjection(24, 33).eval(), 7).cuda()
    x, z = torch.randn(2, 16, 9, 11, generator=_gen(1)).cuda(), torch.randn(2, 24, 9, 11, generator=_gen(2)).cuda()

    def stock(fn):
        old, sa.engine.HEADS_HIP = sa.engine.HEADS_HIP, False
        try:
            return dfr.real(fn())
        finally:
            sa.engine.HEADS_HIP = old
    with torch.no_grad():
        h0, p0 = dfr.real(head(x)), proj(z)
        assert torch.allclose(h0, stock(lambda: head(x)), atol=2e-5, rtol=1e-5) and torch.allclose(p0, stock(lambda: proj(z)), atol=2e-5, rtol=1e-5)
        # load_state_dict with other values
        head.load_state_dict(copy.deepcopy(_head(sa, 16, 62)).state_dict())
        proj.load_state_dict(dc.fill(M.ChalProjection(24, 33), 8).state_dict())
        h1, p1 = dfr.real(head(x)), proj(z)
        assert not torch.allclose(h1, h0, atol=1e-3) and not torch.allclose(p1, p0, atol=1e-3)
        assert torch.allclose(h1, stock(lambda: head(x)), atol=2e-5, rtol=1e-5) and torch.allclose(p1, stock(lambda: proj(z)), atol=2e-5, rtol=1e-5)
        # in-place updates of single tensors: the 1x1's bias, a BatchNorm buffer, a projection's bias
        head.conv2.bias.add_(1.0)
        head.conv1.bn.running_var.mul_(4.0)
        proj[0].bias.add_(0.5)
        proj[1].running_mean.sub_(0.25)
        h2, p2 = dfr.real(head(x)), proj(z)
        assert not torch.allclose(h2, h1, atol=1e-3) and not torch.allclose(p2, p1, atol=1e-3)
        assert torch.allclose(h2, stock(lambda: head(x)), atol=2e-5, rtol=1e-5) and torch.allclose(p2, stock(lambda: proj(z)), atol=2e-5, rtol=1e-5)


# ---- 14. the switches ----

def test_switches_route_to_the_stock_layers_and_count_it(sa):
    M, E, dfr = sa.modules, sa.engine, sa.deferred
    head = copy.deepcopy(_head(sa, 16, 71)).cuda().eval()
    proj = dc.fill(M.ChalProjection(24, 33).eval(), 9).cuda()
    x, z = torch.randn(1, 16, 8, 8, generator=_gen(3)).cuda(), torch.randn(1, 24, 8, 8, generator=_gen(4)).cuda()

    def counts(fn):
        b = dict(M.PATH_COUNTS)
        y = dfr.real(fn())
        return y, M.PATH_COUNTS["hip"] - b["hip"], M.PATH_COUNTS["torch"] - b["torch"]
    with torch.no_grad():
        h_hip, h, t = counts(lambda: head(x))
        assert (h, t) == (1, 0)
        p_hip, h, t = counts(lambda: proj(z))
        assert (h, t) == (1, 0)
        (pa, pb), h, t = counts(lambda: proj.forward_pair(z, z * 2))
        assert (h, t) == (1, 0) and torch.equal(pa, p_hip) and torch.equal(pb, proj(z * 2))
        for name, value in (("HEADS_HIP", False), ("CONV_ENGINE", "f32")):
            old = getattr(E, name)
            setattr(E, name, value)
            try:
                y, h, t = counts(lambda: head(x))
                assert (h, t) == (0, 1), (name, h, t)
                assert torch.allclose(y, h_hip, atol=2e-5, rtol=1e-5)
                y, h, t = counts(lambda: proj(z))
                assert (h, t) == (0, 1), (name, h, t)
                assert torch.allclose(y, p_hip, atol=2e-5, rtol=1e-5)
                (ya, yb), h, t = counts(lambda: proj.forward_pair(z, z * 2))
                assert (h, t) == (0, 2) and torch.allclose(ya, p_hip, atol=2e-5, rtol=1e-5)
            finally:
                setattr(E, name, old)
        # CPU tensors on a CPU copy
        y, h, t = counts(lambda: copy.deepcopy(head).cpu()(x.cpu()))
        assert (h, t) == (0, 1) and torch.allclose(y, h_hip.cpu(), atol=2e-5, rtol=1e-5)
        y, h, t = counts(lambda: copy.deepcopy(proj).cpu()(z.cpu()))
        assert (h, t) == (0, 1) and torch.allclose(y, p_hip.cpu(), atol=2e-5, rtol=1e-5)
        # float64: the stock layers
        y, h, t = counts(lambda: copy.deepcopy(proj).double()(z.double()))
        assert (h, t) == (0, 1) and y.dtype == torch.float64
    # autograd on (the parameters require grad): the stock layers, counted, tensors rather than handles
    y, h, t = counts(lambda: head(x))
    assert (h, t) == (0, 1) and isinstance(y, torch.Tensor) and y.requires_grad
    y, h, t = counts(lambda: proj(z))
    assert (h, t) == (0, 1) and y.requires_grad
