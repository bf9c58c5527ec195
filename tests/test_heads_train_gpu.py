"""The segmentation heads and the chal_* projections under autograd / in train() on HIP (csrc/seghead_train.hip,
semstereo_amd/train_heads.py, SS_HEADS_TRAIN_HIP=1): the tail kernels against float64 on edge shapes, the adjoint identity, bit
identities, NaN / Inf containment; the projection and the head as layers against float64 with the fp32 CPU layer as the yardstick;
the routing; one train() forward + backward of the stand-in model.  Run on the MI355X box: pytest -m gpu."""
import copy
import os

import pytest
import torch
import torch.nn.functional as F

from golden import decoder_cases as dc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    assert semstereo_amd.engine.CONV_ENGINE == "f16x3" and semstereo_amd.engine.HEADS_TRAIN_HIP is False
    return semstereo_amd


@pytest.fixture
def switch_on(sa, monkeypatch):
    """The switch on, and projections of every size on the kernels (by default those of fewer than
    train_heads.PROJ_MIN_POSITIONS positions keep the stock layers, where they were measured slower: test_routing covers that)."""
    monkeypatch.setattr(sa.engine, "HEADS_TRAIN_HIP", True)
    monkeypatch.setattr(_th(), "PROJ_MIN_POSITIONS", 0)
    return sa


def _th():
    return __import__("semstereo_amd.train_heads", fromlist=["x"])


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- the tail kernels, called directly -------------------------------------------------------------------------------------------

# (B, H, W): single positions, single rows / columns, a ragged map, exactly one 8 x 32 tile, a tile plus one in both axes, a ragged map
# of several tiles with an even width (16-byte stores forward, the scalar form backward), and one whose width is a multiple of 4 but
# not of the tile (the 16-byte form backward with a partial tile)
TAIL_SHAPES = [(1, 1, 1), (1, 1, 9), (1, 9, 1), (2, 5, 7), (1, 8, 32), (1, 9, 33), (1, 17, 70), (2, 12, 36)]
CLASSES = (1, 6, 8)
_CASES = {}


def _case(B, H, W, C, up2):
    """Inputs and the float64 CPU results of one case, computed once and shared (never modified)."""
    key = (B, H, W, C, up2)
    if key not in _CASES:
        g = _gen(1000 * H + 10 * W + C + up2)
        a = torch.relu(torch.randn(B, 32, H, W, generator=g) + 0.3)             # what a BatchNorm + ReLU hands over
        w2 = (torch.rand(C, 32, generator=g) * 2 - 1) * (3.0 / 32) ** 0.5
        bias = torch.rand(C, generator=g) * 0.2 - 0.1
        s = 2 if up2 else 1
        G = torch.randn(B, C, s * H, s * W, generator=g)
        ad, wd, bd = (t.double().requires_grad_(True) for t in (a, w2, bias))
        out = _tail_torch(ad, wd, bd, up2)
        ga, gw, gb = torch.autograd.grad(out, (ad, wd, bd), G.double())
        _CASES[key] = (a, w2, bias, G, {"out": out.detach(), "grad_a": ga, "grad_w2": gw, "grad_bias": gb})
    return _CASES[key]


def _tail_torch(a, w2, bias, up2):
    y = F.conv2d(a, w2.reshape(w2.shape[0], 32, 1, 1), bias)
    if up2:
        y = F.interpolate(y, size=(2 * a.shape[2], 2 * a.shape[3]), mode="bilinear", align_corners=False)
    return y


def _tail_hip(sa, a, w2, bias, G, up2, want=(True, True, True)):
    """The two entry points on device copies -> out, grad_a, grad_w2, grad_bias (None where not requested)."""
    L, TH = sa._lib, __import__("semstereo_amd.train_heads", fromlist=["x"])
    a, w2, bias, G = (t.cuda().contiguous() for t in (a, w2, bias, G))
    B, K, H, W = a.shape
    C = w2.shape[0]
    out = torch.full_like(G, float("nan"))
    L.call("ss_seghead_tail_fwd", L.ptr(a), L.ptr(w2), L.ptr(bias), L.ptr(out), B, K, C, H, W, int(up2))
    nan = float("nan")
    ga = torch.full_like(a, nan) if want[0] else None
    gw = torch.full_like(w2, nan) if want[1] else None
    gb = torch.full_like(bias, nan) if want[2] else None
    work = TH.tail_workspace(B, C, H, W, a.device) if (want[1] or want[2]) else None
    L.call("ss_seghead_tail_bwd", L.ptr(G), L.ptr(a), L.ptr(w2), L.ptr(ga), L.ptr(gw), L.ptr(gb), L.ptr(work), B, K, C, H, W, int(up2))
    torch.cuda.synchronize()
    return out, ga, gw, gb


@pytest.mark.parametrize("shape", TAIL_SHAPES, ids=["x".join(map(str, s)) for s in TAIL_SHAPES])
def test_tail_against_float64(sa, shape):
    """Forward and the three gradients: max |err| <= 2e-5 max |ref| per output (the bound tests/train_calls.py::BOUNDS gives every
    comparable fp32 seam; no "fp32 is as bad" clause: these are 32-term fp32 sums of O(1) data).  grad_bias against the plain sum of
    grad_out in float64 to 1e-6 of max |ref| (the convention of the bound above: relative to the largest reference value)."""
    B, H, W = shape
    for C in CLASSES:
        for up2 in (1, 0):
            a, w2, bias, G, ref = _case(B, H, W, C, up2)
            got = dict(zip(("out", "grad_a", "grad_w2", "grad_bias"), _tail_hip(sa, a, w2, bias, G, up2)))
            for k, r in ref.items():
                assert got[k].shape == r.shape, (shape, C, up2, k)
                err, scale = float((got[k].double().cpu() - r).abs().max()), float(r.abs().max())
                print(f"tail {shape} C={C} up2={up2} {k:9s} max err {err:.3e} max |ref| {scale:.3e} ratio {err / max(scale, 1e-30):.2e}")
                assert err <= 2e-5 * scale, (shape, C, up2, k, err, scale)
            plain = G.double().sum((0, 2, 3))
            err = float((got["grad_bias"].double().cpu() - plain).abs().max())
            print(f"tail {shape} C={C} up2={up2} grad_bias against sum(grad_out): {err:.3e} of {float(plain.abs().max()):.3e}")
            assert err <= 1e-6 * float(plain.abs().max()), (shape, C, up2, err)


@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 9, 33), (2, 12, 36)], ids=str)
def test_tail_adjoint_identity(sa, shape):
    """With bias = 0 the tail is bilinear in (a, w2): <tail(a, w2), G> = <a, grad_a> = <w2, grad_w2>, evaluated in float64 from the
    GPU's outputs, each to 1e-5 of the inner product itself."""
    B, H, W = shape
    for C in CLASSES:
        for up2 in (1, 0):
            a, w2, bias, G, _ = _case(B, H, W, C, up2)
            out, ga, gw, _ = _tail_hip(sa, a, w2, torch.zeros_like(bias), G, up2)
            lhs = float((out.double().cpu() * G.double()).sum())
            ra, rw = float((a.double() * ga.double().cpu()).sum()), float((w2.double() * gw.double().cpu()).sum())
            print(f"adjoint {shape} C={C} up2={up2}: <out,G> {lhs:.9e} <a,ga> {ra:.9e} <w2,gw> {rw:.9e} "
                  f"relative {abs(lhs - ra) / abs(lhs):.2e} {abs(lhs - rw) / abs(lhs):.2e}")
            assert abs(lhs - ra) <= 1e-5 * abs(lhs) and abs(lhs - rw) <= 1e-5 * abs(lhs), (shape, C, up2, lhs, ra, rw)


def test_tail_bit_identities(sa):
    """Two calls give the same bits; an element has the same bits alone and in a batch of 3; a NULL gradient leaves the others' bits."""
    for (H, W, up2) in ((17, 70, 1), (12, 36, 1), (9, 33, 0)):
        C = 6
        g = _gen(H * W)
        a = torch.relu(torch.randn(3, 32, H, W, generator=g)) * torch.tensor([1.0, 40.0, 1e-3]).reshape(3, 1, 1, 1)
        w2, bias = torch.randn(C, 32, generator=g) * 0.3, torch.randn(C, generator=g) * 0.1
        s = 2 if up2 else 1
        G = torch.randn(3, C, s * H, s * W, generator=g)
        first, second = _tail_hip(sa, a, w2, bias, G, up2), _tail_hip(sa, a, w2, bias, G, up2)
        for x, y in zip(first, second):
            assert torch.equal(x, y), (H, W, up2)
        for b in range(3):
            out, ga, _, _ = _tail_hip(sa, a[b:b + 1], w2, bias, G[b:b + 1], up2)
            assert torch.equal(out, first[0][b:b + 1]) and torch.equal(ga, first[1][b:b + 1]), (H, W, up2, b)
        for drop in range(3):
            want = tuple(i != drop for i in range(3))
            part = _tail_hip(sa, a, w2, bias, G, up2, want=want)
            assert torch.equal(part[0], first[0])
            for i in range(3):
                if want[i]:
                    assert torch.equal(part[1 + i], first[1 + i]), (H, W, up2, drop, i)
                else:
                    assert part[1 + i] is None


def test_tail_nan_and_inf_stay_in_their_footprint(sa):
    """Rows of grad_out set to inf / nan reach the positions whose 4 x 4 footprint (output rows 2i - 1 .. 2i + 2) they touch, and no
    other position of grad_a."""
    B, H, W, C = 2, 19, 40, 6
    g = _gen(77)
    a = torch.relu(torch.randn(B, 32, H, W, generator=g))
    w2, bias = torch.randn(C, 32, generator=g) * 0.3, torch.zeros(C)
    G = torch.randn(B, C, 2 * H, 2 * W, generator=g)
    clean = _tail_hip(sa, a, w2, bias, G, 1, want=(True, False, False))[1]
    for bad in (float("nan"), float("inf")):
        for rows in ((0,), (15, 16), (2 * H - 1,)):
            Gb = G.clone()
            hit = torch.zeros(B, 32, H, W, dtype=torch.bool)
            for r in rows:
                Gb[1, :, r, :] = bad
                for i in range(H):
                    if max(2 * i - 1, 0) <= r <= min(2 * i + 2, 2 * H - 1):
                        hit[1, :, i, :] = True
            got = _tail_hip(sa, a, w2, bias, Gb, 1, want=(True, False, False))[1].cpu()
            assert bool((~torch.isfinite(got[hit])).all()), (bad, rows)
            assert torch.equal(got[~hit], clean.cpu()[~hit]), (bad, rows)


# ---- the layers through the twins, the switch on ---------------------------------------------------------------------------------

def _bound(x, w, scale, K, padding=0):
    """|error| the two-term fp16 form may have against the exact layer: per product 2^-21 (two operand representations at 2^-23 and
    the dropped lo*lo at 2^-22), a K-term fp32 accumulation as a random walk with a factor 4, and two roundings of the affine --
    all relative to sum |x| |w| (times |scale|)."""
    S = F.conv2d(x.double().abs(), w.double().abs(), None, 1, padding)
    if scale is not None:
        S = S * scale.double().abs()[None, :, None, None]
    return (2.0 ** -21 + 4.0 * K ** 0.5 * 2.0 ** -24) * S + 1e-30


def _run_layer(mod, x, wt, dev, dtype):
    """One forward + backward of loss = <layer(x), wt> (a seeded linear functional) -> outputs, gradients, buffers."""
    xl = x.detach().to(dev, dtype).clone().requires_grad_(True)
    mod.zero_grad(set_to_none=True)
    y = mod(xl)
    (y * wt.to(dev, dtype)).sum().backward()
    res = {"out": y.detach(), "grad_x": xl.grad}
    res.update({"grad:" + k: p.grad for k, p in mod.named_parameters()})
    res.update({"buf:" + k: b.detach().clone() for k, b in mod.named_buffers()})
    return res


def _check(hip, f64, f32, training):
    """The protocol of test_ssr_train_gpu._check at this layer's bound: 2e-5 max |ref| or 1.5 x the fp32 CPU layer's error; the bias
    of a convolution that feeds a BatchNorm on batch statistics (its true gradient is zero: the mean is subtracted) is read against
    the scale of that convolution's weight gradient; buffers to 1e-6 relative, the batch counter equal."""
    for k, ref in f64.items():
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
        if training and k == "grad:0.bias":
            scale = float(f64["grad:0.weight"].abs().max())
        print(f"  {k:28s} max err {err:.3e} fp32 cpu {e32:.3e} max |ref| {scale:.3e}")
        assert err <= 2e-5 * scale or err <= 1.5 * e32, (k, err, scale, e32)


LAYERS = {
    "chal24to32": (lambda M: M.ChalProjection(24, 32), (2, 24, 5, 7)),
    "chal768to384": (lambda M: M.ChalProjection(768, 384), (2, 768, 5, 7)),
    "head16": (lambda M: M.segmenthead(16, 32, 6, 2), (2, 16, 6, 10)),
    "head128": (lambda M: M.segmenthead(128, 32, 6, 2), (2, 128, 6, 10)),
}


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval_autograd"])
@pytest.mark.parametrize("name", sorted(LAYERS))
def test_layers_against_float64(switch_on, name, training):
    sa = switch_on
    M = sa.modules
    make, shape = LAYERS[name]
    base = dc.fill(make(M), 31 + len(name)).train(training)
    x = torch.randn(shape, generator=_gen(sum(shape)))
    m64, m32, mg = copy.deepcopy(base).double(), copy.deepcopy(base), copy.deepcopy(base).cuda()
    with torch.no_grad():
        wt = torch.randn(m32(x).shape, generator=_gen(5 + shape[1]))
    m32 = copy.deepcopy(base)                                    # (the probe above moved the running statistics)
    r64, r32 = _run_layer(m64, x, wt, "cpu", torch.float64), _run_layer(m32, x, wt, "cpu", torch.float32)
    before = dict(M.PATH_COUNTS)
    rg = _run_layer(mg, x, wt, "cuda", torch.float32)
    torch.cuda.synchronize()
    assert M.PATH_COUNTS.get("hip_train", 0) > before.get("hip_train", 0) and M.PATH_COUNTS["torch"] == before["torch"]
    print(name, "train()" if training else "eval() under autograd")
    _check(rg, r64, r32, training)
    if name.startswith("chal"):
        # the projection's convolution alone: forward and data gradient inside the derived two-term fp16 bound
        TH = __import__("semstereo_amd.train_heads", fromlist=["x"])
        conv = base[0]
        Cout, Cin = conv.out_channels, conv.in_channels
        xg = x.cuda().requires_grad_(True)
        w, bias = conv.weight.detach().cuda().requires_grad_(True), conv.bias.detach().cuda().requires_grad_(True)
        y = TH._Proj2dK1.apply(xg, w, bias)
        gy = torch.randn(y.shape, generator=_gen(Cout))
        y.backward(gy.cuda())
        want = F.conv2d(x.double(), conv.weight.detach().double(), conv.bias.detach().double())
        excess = ((y.detach().double().cpu() - want).abs() - _bound(x, conv.weight.detach(), None, Cin) - 2.0 ** -22 * want.abs()).max()
        assert float(excess) <= 0.0, ("forward", name, float(excess))
        wt_t = conv.weight.detach().reshape(Cout, Cin).t().reshape(Cin, Cout, 1, 1)
        want = F.conv2d(gy.double(), wt_t.double())
        excess = ((xg.grad.double().cpu() - want).abs() - _bound(gy, wt_t, None, Cout) - 2.0 ** -22 * want.abs()).max()
        assert float(excess) <= 0.0, ("data gradient", name, float(excess))


def _record(sa, monkeypatch):
    E, symbols = sa.engine, []
    real_call = E.call
    monkeypatch.setattr(E, "call", lambda name, *a: (symbols.append((name, a)), real_call(name, *a))[1])
    return symbols


def _names(symbols):
    return [n for n, _ in symbols]


def test_routing(sa, monkeypatch):
    """This fails without the feature: with the switch on a train() / autograd call of the twins used to run the stock layers."""
    M, E = sa.modules, sa.engine
    head = dc.fill(M.segmenthead(16, 32, 6, 2), 41).cuda().train()
    proj = dc.fill(M.ChalProjection(24, 32), 42).cuda().train()
    x, z = torch.randn(2, 16, 6, 10, generator=_gen(1)).cuda(), torch.randn(2, 24, 5, 7, generator=_gen(2)).cuda()
    symbols = _record(sa, monkeypatch)

    def counts(fn):
        b = dict(M.PATH_COUNTS)
        y = fn()
        return y, M.PATH_COUNTS.get("hip_train", 0) - b.get("hip_train", 0), M.PATH_COUNTS["torch"] - b["torch"]

    monkeypatch.setattr(E, "HEADS_TRAIN_HIP", True)
    # a projection of fewer positions than the threshold keeps the stock layers (measured slower there), from it up the kernels run
    assert _th().PROJ_MIN_POSITIONS == 32768
    big = torch.randn(2, 24, 128, 128, generator=_gen(5)).cuda()
    y, h, t = counts(lambda: proj(z))
    assert (h, t) == (0, 1)
    y, h, t = counts(lambda: proj(big))
    assert h >= 1 and t == 0
    y, h, t = counts(lambda: proj(big[:, :, :127].contiguous()))
    assert (h, t) == (0, 1)
    monkeypatch.setattr(_th(), "PROJ_MIN_POSITIONS", 0)
    for mode in (True, False):                                   # train(), and eval() with parameters that require grad
        head.train(mode), proj.train(mode)
        del symbols[:]
        y, h, t = counts(lambda: head(x.clone().requires_grad_(True)))
        assert h >= 1 and t == 0 and y.requires_grad, (mode, h, t)
        assert _names(symbols).count("ss_seghead_tail_fwd") == 1 and "ss_seghead_tail_bwd" not in _names(symbols)
        y.sum().backward()
        assert _names(symbols).count("ss_seghead_tail_bwd") == 1
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in head.parameters())
        del symbols[:]
        y, h, t = counts(lambda: proj(z))
        assert h >= 1 and t == 0 and y.requires_grad, (mode, h, t)
        assert _names(symbols).count("ss_conv2d_k1_f16s_fwd") == 1
        (ya, yb), h, t = counts(lambda: proj.forward_pair(z, z * 2))        # under autograd: two single calls
        assert h >= 2 and t == 0 and "ss_conv2d_k1_f16s_pair_fwd" not in _names(symbols)
    head.train(), proj.train()
    h_hip, p_hip = head(x).detach(), proj(z).detach()

    # anything else: the stock layers, counted, with the same values
    def stock(what, hd, pj, xx, zz):
        y, h, t = counts(lambda: hd(xx))
        assert (h, t) == (0, 1), (what, h, t)
        assert torch.allclose(y.detach().float().cpu(), h_hip.cpu(), atol=2e-5, rtol=1e-5), what
        y, h, t = counts(lambda: pj(zz))
        assert (h, t) == (0, 1), (what, h, t)
        assert torch.allclose(y.detach().float().cpu(), p_hip.cpu(), atol=2e-5, rtol=1e-5), what

    def fresh():
        # (a train() forward moves the running statistics, not the output: every comparison starts from the same module)
        return dc.fill(M.segmenthead(16, 32, 6, 2), 41).cuda().train(), dc.fill(M.ChalProjection(24, 32), 42).cuda().train()
    for name, value in (("HEADS_TRAIN_HIP", False), ("TRAIN_HIP", False), ("CONV_ENGINE", "f32"), ("HEADS_HIP", False)):
        with monkeypatch.context() as mp:
            mp.setattr(E, name, value)
            stock(name, *fresh(), x, z)
    hd, pj = fresh()
    stock("cpu", hd.cpu(), pj.cpu(), x.cpu(), z.cpu())
    hd, pj = fresh()
    stock("float64", hd.double(), pj.double(), x.double(), z.double())
    hd, pj = fresh()
    y, h, t = counts(lambda: hd(x.transpose(2, 3).contiguous().transpose(2, 3)))                  # a non-contiguous input
    assert (h, t) == (0, 1)


def test_only_the_gradients_autograd_needs_are_computed(switch_on, monkeypatch):
    sa = switch_on
    M = sa.modules
    head = dc.fill(M.segmenthead(16, 32, 6, 2), 43).cuda().train()
    x = torch.randn(2, 16, 6, 10, generator=_gen(3)).cuda()
    symbols = _record(sa, monkeypatch)

    def bwd_args():
        (args,) = [a for n, a in symbols if n == "ss_seghead_tail_bwd"]
        return args[3:6]                                         # grad_a, grad_w2, grad_bias

    # everything requires grad: three pointers, and conv1's data-gradient convolution runs in the backward
    head(x.clone().requires_grad_(True)).sum().backward()
    assert all(p is not None for p in bwd_args())
    assert _names(symbols).count("ss_conv2d_bf16s_fwd") == 2
    # an input that does not require grad: conv1's data gradient is not launched
    del symbols[:]
    head(x).sum().backward()
    assert all(p is not None for p in bwd_args())                # (conv1's weight and the BatchNorm still need grad_a)
    assert _names(symbols).count("ss_conv2d_bf16s_fwd") == 1
    # conv2 frozen: neither grad_w2 nor grad_bias
    del symbols[:]
    head.conv2.requires_grad_(False)
    head(x).sum().backward()
    ga, gw, gb = bwd_args()
    assert ga is not None and gw is None and gb is None
    # only conv2 trains and the input needs nothing: grad_a is not requested
    del symbols[:]
    head.requires_grad_(False)
    head.conv2.requires_grad_(True)
    head(x).sum().backward()
    ga, gw, gb = bwd_args()
    assert ga is None and gw is not None and gb is not None
    assert _names(symbols).count("ss_conv2d_bf16s_fwd") == 1


# ---- a train() forward + backward of the stand-in model ---------------------------------------------------------------------------

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
    return net.cuda()


def test_train_step_of_the_standin_model(sa, monkeypatch):
    import standin_model
    previous = sa.install(standin_model)                         # the stand-in looks its op library up by bare name, as the reference does
    try:
        _train_step(sa, monkeypatch)
    finally:
        sa.uninstall(standin_model, previous)


def _train_step(sa, monkeypatch):
    from oracle import detdata as dd
    M, E = sa.modules, sa.engine
    net = _model(sa)
    left = dd.t_normalish((1, 3, 256, 384), 951)
    right = torch.roll(left, shifts=-3, dims=3) + 0.05 * dd.t_normalish((1, 3, 256, 384), 952)
    left, right = left.cuda(), right.cuda()
    done = sa.accelerate(net, decoder=True, heads=True)
    assert done == ["head_l", "head_r", "chal_0", "chal_1", "chal_2", "chal_3", "chal_4"]
    net.train()
    state = copy.deepcopy(net.state_dict())                      # (a train() forward moves the running statistics)
    with torch.no_grad():
        ref = net(left, right)                                   # the switch off: the stock layers
    net.load_state_dict(state)
    symbols = _record(sa, monkeypatch)
    monkeypatch.setattr(E, "HEADS_TRAIN_HIP", True)
    monkeypatch.setattr(_th(), "PROJ_MIN_POSITIONS", 0)         # (the smaller maps of a 256 x 384 pair are below the threshold: all seven on HIP)
    before = dict(M.PATH_COUNTS)
    out = net(left, right)
    assert len(out) == 3 and all(isinstance(t, torch.Tensor) and tuple(t.shape) == (1, 6, 256, 384) for t in out[1:])
    assert _names(symbols).count("ss_seghead_tail_fwd") == 2 and _names(symbols).count("ss_conv2d_k1_f16s_fwd") == 7, _names(symbols)
    assert M.PATH_COUNTS.get("hip_train", 0) >= before.get("hip_train", 0) + 2 + 7
    for got, want in zip(out[1:], ref[1:]):
        err = float((got.detach() - want).abs().max())
        print("train() label map against the stock layers: max", err, "of", float(want.abs().max()))
        assert err <= 1e-4 * max(1.0, float(want.abs().max()))
    (out[1] + out[2]).sum().backward()
    assert _names(symbols).count("ss_seghead_tail_bwd") == 2
    reached = 0
    for name, p in net.named_parameters():
        if name.split(".")[0] in ("head_l", "head_r", "chal_0", "chal_1", "chal_2", "chal_3", "chal_4") and p.grad is not None:
            reached += 1
            assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, name
    assert reached >= 2 * 5                                      # both heads: conv1.conv.weight, conv1.bn.weight / bias, conv2.weight / bias
