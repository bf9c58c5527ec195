"""The dedicated 2-D 3x3 weight-gradient kernel (csrc/conv2d_wgrad.hip, train.conv2d_k3_wgrad_hip, SS_CONV2D_WGRAD_HIP=1): against
float64 on edge shapes, exact on small integers, reproducible and fully written, powers of two commute, the adjoint identity, NaN / Inf
containment per channel, the two seams (train._Conv2dK3, train_decoder._Conv2dK3Cat), and the layers that use them against float64
with the switch on.  Run on the MI355X box: pytest -m gpu."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden import decoder_cases as dc
from golden import decoder_train_cases as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, C0, C1, Cout, H, W): everything ragged, a source boundary that is no multiple of 32 and a 32-column boundary crossed; one position
# (only the centre tap is non-zero); W < 8 and a second output-channel tile of one channel; Cout = 6, an odd row count and exactly four
# K-steps per row; more than one partial per weight tile; the model's class (C0 = C1 = Cout / 2), several tiles on both axes
SHAPES = [(2, 24, 16, 40, 5, 37), (3, 8, 0, 8, 1, 1), (1, 3, 5, 33, 2, 3), (1, 40, 40, 6, 33, 64), (2, 16, 0, 16, 40, 70), (1, 64, 64, 128, 16, 16)]
MULTI = SHAPES[4]
IDS = ["x".join(map(str, s)) for s in SHAPES]
_CASES = {}


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    E = semstereo_amd.engine
    assert E.CONV_ENGINE == "f16x3" and E.CONV2D_WGRAD_HIP is False and E.DECODER_TRAIN_HIP is False and E.HEADS_TRAIN_HIP is False
    return semstereo_amd


def _t(sa):
    return sa.train


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ref(G, x, rem, dtype):
    """torch.nn.grad.conv2d_weight on the materialised concatenation, on the CPU."""
    xin = x if rem is None else torch.cat((x, rem), 1)
    return torch.nn.grad.conv2d_weight(xin.to(dtype), (G.shape[1], xin.shape[1], 3, 3), G.to(dtype), stride=1, padding=1)


def _case(shape, integers=False):
    """Inputs and the float64 / fp32 CPU gradients of one shape, computed once and shared (never modified)."""
    key = (shape, integers)
    if key not in _CASES:
        B, C0, C1, Cout, H, W = shape
        g = _gen(7 * C0 + 3 * Cout + 100 * H + W + C1 + int(integers))
        if integers:
            draw = lambda *s: torch.randint(-2, 3, s, generator=g).float()
        else:
            draw = lambda *s: torch.randn(*s, generator=g)
        x, rem, G = draw(B, C0, H, W), (draw(B, C1, H, W) if C1 else None), draw(B, Cout, H, W)
        _CASES[key] = (G, x, rem, _ref(G, x, rem, torch.float64), _ref(G, x, rem, torch.float32))
    return _CASES[key]


def _hip(sa, G, x, rem):
    gw = _t(sa).conv2d_k3_wgrad_hip(G.cuda(), x.cuda(), None if rem is None else rem.cuda())
    torch.cuda.synchronize()
    return gw


def _partials(sa, B, C0, C1, Cout, H, W):
    tiles = (-(-C0 // 32) + -(-C1 // 32)) * -(-Cout // 32)
    n = _t(sa).conv2d_k3_wgrad_workspace_bytes(B, C0, C1, H, W, Cout)
    assert n % (36864 * tiles) == 0
    return n // (36864 * tiles)


def test_the_shapes_reach_more_than_one_partial(sa):
    assert _partials(sa, *MULTI) > 1 and _partials(sa, 3, *MULTI[1:]) > 1
    assert _partials(sa, *SHAPES[0]) == 1


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_against_float64(sa, shape):
    """max |err| <= 5e-6 max |ref| (tests/train_calls.py::BOUNDS["train_layers.conv3d_wgrad_hip"], the project's bound for this
    arithmetic) or at most 1.5 x the error of the same call in fp32 on the CPU."""
    G, x, rem, f64, f32 = _case(shape)
    got = _hip(sa, G, x, rem)
    assert got.shape == f64.shape and got.dtype == torch.float32 and got.is_contiguous()
    err, e32, scale = float((got.double().cpu() - f64).abs().max()), float((f32.double() - f64).abs().max()), float(f64.abs().max())
    print(f"conv2d_k3_wgrad {shape}: max err {err:.3e} fp32 cpu {e32:.3e} max |ref| {scale:.3e} ratio {err / scale:.2e} fp32 ratio {e32 / scale:.2e}")
    assert err <= 5e-6 * scale or err <= 1.5 * e32, (shape, err, scale, e32)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exact_on_small_integers(sa, shape):
    """Inputs and gradients from {-2, ..., 2}: every term is exact in bf16 and every sum far below 2^24, so the result EQUALS float64:
    indexing, padding, masks and the output layout without a tolerance; two sources or one."""
    G, x, rem, f64, _ = _case(shape, integers=True)
    assert float(f64.abs().max()) < 2 ** 24
    got = _hip(sa, G, x, rem).double().cpu()
    assert torch.equal(got, f64), (shape, int((got != f64).sum()), float((got - f64).abs().max()))
    if rem is not None:                                          # the concatenation as ONE source gives the same numbers
        one = _hip(sa, G, torch.cat((x, rem), 1), None).double().cpu()
        assert torch.equal(one, f64), shape


def _multi_inputs():
    B, C0, _, Cout, H, W = MULTI
    g = _gen(H * W + C0)
    x = torch.randn(3, C0, H, W, generator=g).cuda()
    G = (torch.randn(3, Cout, H, W, generator=g) * torch.tensor([1.0, 40.0, 1e-3]).reshape(3, 1, 1, 1)).cuda()
    return G, x


def test_reproducible_and_fully_written(sa):
    """Two calls give equal bits on the multi-partial shape (B = 3, the elements' gradients scaled by 1, 40, 1e-3); the same bits with
    the workspace and grad_w pre-filled with NaN: every partial slot that is read was written, every element of grad_w is written."""
    T = _t(sa)
    G, x = _multi_inputs()
    first, second = T.conv2d_k3_wgrad_hip(G, x), T.conv2d_k3_wgrad_hip(G, x)
    assert torch.equal(first, second) and bool(torch.isfinite(first).all())
    B, C0, H, W = x.shape
    Cout = G.shape[1]
    nbytes = T.conv2d_k3_wgrad_workspace_bytes(B, C0, 0, H, W, Cout)
    assert nbytes > 36864
    for G_, x_, rem_ in ((G, x, None), (G, x[:, :5].contiguous(), x[:, 5:].contiguous())):
        C0_, C1_ = x_.shape[1], 0 if rem_ is None else rem_.shape[1]
        n = T.conv2d_k3_wgrad_workspace_bytes(B, C0_, C1_, H, W, Cout)
        work = torch.full((n // 4,), float("nan"), device="cuda")
        gw = torch.full((Cout, C0, 3, 3), float("nan"), device="cuda")
        sa._lib.call("ss_conv2d_k3_wgrad_fwd", G_.data_ptr(), x_.data_ptr(), None if rem_ is None else rem_.data_ptr(), gw.data_ptr(),
                     work.data_ptr(), B, C0_, C1_, H, W, Cout)
        torch.cuda.synchronize()
        assert torch.equal(gw, first), (C0_, C1_)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4]], ids=[IDS[0], IDS[4]])
def test_powers_of_two_commute(sa, shape):
    """grad_out scaled by 2^60 / 2^-60: bit-equal to the unscaled result times the same power (bf16 has fp32's exponent range)."""
    G, x, rem, _, _ = _case(shape)
    base = _hip(sa, G, x, rem)
    for p in (60, -60):
        s = 2.0 ** p
        got = _hip(sa, G * s, x, rem)
        assert torch.equal(got, base * s), (shape, p)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3], SHAPES[5]], ids=[IDS[0], IDS[3], IDS[5]])
def test_adjoint_identity(sa, shape):
    """<G, conv2d(cat(x, rem), w)> = <grad_w, w>, in float64 from the GPU's grad_w with a random w, to 1e-5 of the inner product."""
    G, x, rem, _, _ = _case(shape)
    got = _hip(sa, G, x, rem).double().cpu()
    w = torch.randn(got.shape, generator=_gen(sum(shape)), dtype=torch.float64)
    xin = (x if rem is None else torch.cat((x, rem), 1)).double()
    lhs, rhs = float((G.double() * F.conv2d(xin, w, padding=1)).sum()), float((got * w).sum())
    print(f"adjoint {shape}: <G,Cx> {lhs:.9e} <gw,w> {rhs:.9e} relative {abs(lhs - rhs) / abs(lhs):.2e}")
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (shape, lhs, rhs)


def test_non_finite_values_stay_in_their_channel(sa):
    shape = SHAPES[0]
    B, C0, C1, Cout, H, W = shape
    G, x, rem, _, _ = _case(shape)
    clean = _hip(sa, G, x, rem)
    for bad in (float("nan"), float("inf"), float("-inf")):
        for src, c in ((0, 7), (1, 9)):
            xs = [x.clone(), rem.clone()]
            xs[src][1, c, 2, 17] = bad
            got = _hip(sa, G, xs[0], xs[1])
            ci = c if src == 0 else C0 + c
            keep = torch.ones(C0 + C1, dtype=torch.bool)
            keep[ci] = False
            assert torch.equal(got[:, keep], clean[:, keep]), (bad, src)
            assert not bool(torch.isfinite(got[:, ci]).all()), (bad, src)
        co = 33
        Gb = G.clone()
        Gb[0, co, 4, 0] = bad
        got = _hip(sa, Gb, x, rem)
        keep = torch.ones(Cout, dtype=torch.bool)
        keep[co] = False
        assert torch.equal(got[keep], clean[keep]), bad
        assert not bool(torch.isfinite(got[co]).all()), bad


# ---- the seams ------------------------------------------------------------------------------------------------------------------

def _seam_inputs():
    g = _gen(77)
    y, rem = torch.randn(2, 8, 12, 20, generator=g).cuda(), torch.randn(2, 8, 12, 20, generator=g).cuda()
    w = (torch.randn(16, 16, 3, 3, generator=g) * 0.1).cuda()
    G = torch.randn(2, 16, 12, 20, generator=g).cuda()
    return y, rem, w, G


def _count_depth1(sa, monkeypatch):
    M, calls = sa.modules, []
    real = M.conv3d_wgrad_hip
    monkeypatch.setattr(M, "conv3d_wgrad_hip", lambda *a: (calls.append(a[2:]), real(*a))[1])
    return calls


def _backward_plain(sa, x, w, G, need_x=True, need_w=True):
    xs, ws = x.clone().requires_grad_(need_x), w.clone().requires_grad_(need_w)
    sa.train._Conv2dK3.apply(xs, ws).backward(G)
    torch.cuda.synchronize()
    return xs.grad, ws.grad


def _backward_cat(sa, y, rem, w, G, need=(True, True, True)):
    TD = __import__("semstereo_amd.train_decoder", fromlist=["x"])
    ts = [t.clone().requires_grad_(n) for t, n in zip((y, rem, w), need)]
    TD._Conv2dK3Cat.apply(*ts).backward(G)
    torch.cuda.synchronize()
    return [t.grad for t in ts]


def test_seams(sa, monkeypatch):
    M, E = sa.modules, sa.engine
    TL = sa.train_layers
    y, rem, w, G = _seam_inputs()
    x = torch.cat((y, rem), 1)
    depth1 = _count_depth1(sa, monkeypatch)
    w2d = lambda: M.PATH_COUNTS.get("wgrad2d", 0)

    # the switch off: the depth-1 route, once and twice
    n0 = w2d()
    _, gw_plain_old = _backward_plain(sa, x, w, G)
    assert len(depth1) == 1 and w2d() == n0
    _, _, gw_cat_old = _backward_cat(sa, y, rem, w, G)
    assert len(depth1) == 3 and w2d() == n0

    monkeypatch.setattr(E, "CONV2D_WGRAD_HIP", True)
    del depth1[:]
    gx, gw_plain = _backward_plain(sa, x, w, G)
    assert len(depth1) == 0 and w2d() == n0 + 1 and gx is not None
    gy, grem, gw_cat = _backward_cat(sa, y, rem, w, G)
    assert len(depth1) == 0 and w2d() == n0 + 2 and gy is not None and grem is not None
    assert tuple(gw_plain.shape) == tuple(gw_cat.shape) == (16, 16, 3, 3) and gw_cat.is_contiguous()
    assert torch.equal(gw_plain, gw_cat)                         # the same rows in the same order, one source or two
    f64 = _ref(G.cpu(), x.cpu(), None, torch.float64)
    scale = float(f64.abs().max())
    for got in (gw_plain, gw_cat, gw_plain_old, gw_cat_old):
        assert float((got.double().cpu() - f64).abs().max()) <= 5e-6 * scale

    # only the gradients autograd needs: a weight that does not require grad makes no call
    _backward_plain(sa, x, w, G, need_w=False)
    _backward_cat(sa, y, rem, w, G, need=(True, True, False))
    assert len(depth1) == 0 and w2d() == n0 + 2
    _, gw_only = _backward_plain(sa, x, w, G, need_x=False)
    assert w2d() == n0 + 3 and torch.equal(gw_only, gw_plain)

    # the exact-fp32 weight gradient was asked for: the old route, the switch on
    monkeypatch.setattr(TL, "WGRAD_ENGINE", "f32")
    _backward_plain(sa, x, w, G)
    _backward_cat(sa, y, rem, w, G)
    assert len(depth1) == 3 and w2d() == n0 + 3

    # ... and a non-contiguous or float64 map is not the kernel's
    T = sa.train
    monkeypatch.setattr(TL, "WGRAD_ENGINE", "bf16x6")
    assert T.conv2d_k3_wgrad_applies(G, y, rem) and T.conv2d_k3_wgrad_applies(G, x)
    assert not T.conv2d_k3_wgrad_applies(G, y.transpose(2, 3).contiguous().transpose(2, 3), rem)
    assert not T.conv2d_k3_wgrad_applies(G.double(), y.double(), rem.double()) and not T.conv2d_k3_wgrad_applies(G.cpu(), y.cpu(), rem.cpu())
    assert not T.conv2d_k3_wgrad_applies(G, y, rem[:, :, :11].contiguous())


# ---- the layers, CONV2D_WGRAD_HIP on --------------------------------------------------------------------------------------------

@pytest.fixture
def all_on(sa, monkeypatch):
    for name in ("CONV2D_WGRAD_HIP", "DECODER_TRAIN_HIP", "HEADS_TRAIN_HIP"):
        monkeypatch.setattr(sa.engine, name, True)
    return sa


def _run_layer(mod, inputs, wt, dev, dtype):
    """One forward + backward of loss = <layer(*inputs), wt> (a seeded linear functional) -> outputs, gradients, buffers."""
    xs = [t.detach().to(dev, dtype).clone().requires_grad_(True) for t in inputs]
    mod.zero_grad(set_to_none=True)
    y = mod(*xs)
    (y * wt.to(dev, dtype)).sum().backward()
    res = {"out": y.detach()}
    res.update({f"grad_in:{k}": t.grad for k, t in enumerate(xs)})
    res.update({"grad:" + k: p.grad for k, p in mod.named_parameters()})
    res.update({"buf:" + k: b.detach().clone() for k, b in mod.named_buffers()})
    return res


def _check(hip, f64, f32):
    """2e-5 max |ref| or 1.5 x the fp32 CPU layer's error; buffers to 1e-6 relative, the batch counter equal."""
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
        print(f"  {k:28s} max err {err:.3e} fp32 cpu {e32:.3e} max |ref| {scale:.3e}")
        assert err <= 2e-5 * scale or err <= 1.5 * e32, (k, err, scale, e32)


def _layer_against_float64(sa, base, inputs, wt, calls):
    M = sa.modules
    m64, m32, mg = copy.deepcopy(base).double(), copy.deepcopy(base), copy.deepcopy(base).cuda()
    r64, r32 = _run_layer(m64, inputs, wt, "cpu", torch.float64), _run_layer(m32, inputs, wt, "cpu", torch.float32)
    before = dict(M.PATH_COUNTS)
    rg = _run_layer(mg, inputs, wt, "cuda", torch.float32)
    torch.cuda.synchronize()
    assert M.PATH_COUNTS["torch"] == before["torch"]
    assert M.PATH_COUNTS.get("wgrad2d", 0) == before.get("wgrad2d", 0) + calls
    _check(rg, r64, r32)


def test_conv2x_twin_in_train_against_float64(all_on):
    M = all_on.modules
    base = dc.fill(M.Conv2x(16, 8, deconv=True), 61).train()
    x, rem = torch.randn(2, 16, 6, 10, generator=_gen(11)), torch.randn(2, 8, 12, 20, generator=_gen(12))
    wt = torch.randn(2, 16, 12, 20, generator=_gen(13))
    _layer_against_float64(all_on, base, (x, rem), wt, 1)


LAYERS = {
    "concat_feature32": (lambda M: M.ConcatFeature(32), 32, 2),
    "segmenthead16": (lambda M: M.segmenthead(16, 32, 6, 2), 16, 1),
}


@pytest.mark.parametrize("name", sorted(LAYERS))
def test_heads_in_train_against_float64(all_on, name):
    M = all_on.modules
    make, C, calls = LAYERS[name]
    base = dc.fill(make(M), 31 + len(name)).train()
    x = torch.randn(2, C, 12, 20, generator=_gen(C + 232))
    with torch.no_grad():
        wt = torch.randn(copy.deepcopy(base)(x).shape, generator=_gen(5 + C))
    _layer_against_float64(all_on, base, (x,), wt, calls)


def _check_fixture(case, res, fx):
    """The criterion of test_decoder_train_gpu.test_golden_training_cases_on_hip, per recorded array: 1e-4 max(1, max |ref|)."""
    for key, t in res.items():
        name = f"{case}/{key}"
        if key.endswith("num_batches_tracked"):
            assert int(t) == int(fx[name][0]), name
            continue
        err, big, dsum, dsq = tc.compare(t, fx[name], tc.salt_of(name))
        tol = 1e-4 * max(1.0, big)
        print(f"fixture {name}: max err {err:.2e} max |ref| {big:.3e} sum {dsum:.2e} sum of squares {dsq:.2e}")
        assert err <= tol and dsum <= tol and dsq <= 2 * tol, (name, err, big, dsum, dsq)


def test_golden_training_cases(all_on):
    """The Conv2x cases of decoder_train.npz (the reference's own layers in train(), float64) with the twins on the kernels and conv2's
    weight gradient from the new one."""
    M = all_on.modules
    fx = np.load(os.path.join(ROOT, "tests", "golden", "decoder_train.npz"))
    before = dict(M.PATH_COUNTS)
    for name, (Cin, Cout, _) in tc.CONV2X.items():
        mod = dc.fill(M.Conv2x(Cin, Cout, deconv=True), tc.SALTS[name])
        _check_fixture(name, tc.run(mod, tc.conv2x_inputs(name), name, dtype=torch.float32, device="cuda"), fx)
    mod = dc.fill(M.Spx2(tc.SPX2[0], tc.SPX2[1]), tc.SALTS["spx2"])
    _check_fixture("spx2", tc.run(mod, [tc.spx2_input()], "spx2", dtype=torch.float32, device="cuda"), fx)
    assert M.PATH_COUNTS["torch"] == before["torch"] and M.PATH_COUNTS["decoder_train"] == before.get("decoder_train", 0) + 3
    assert M.PATH_COUNTS.get("wgrad2d", 0) == before.get("wgrad2d", 0) + 2
