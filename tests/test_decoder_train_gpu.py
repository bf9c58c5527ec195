"""The 2-D decoder under autograd / in train() on HIP (csrc/deconv2d_train.hip, semstereo_amd/train_decoder.py, SS_DECODER_TRAIN_HIP=1):
the transposed conv's forward and its two gradient kernels against float64 on edge shapes, the adjoint identity, bit identities,
NaN / Inf containment, only the needed gradients; one Conv2x twin as a layer against float64 with the fp32 CPU layer as the yardstick;
the routing; FeatUp per view; the decoder of the stand-in model and the cases of golden/decoder_train.npz.  Run on the MI355X box:
pytest -m gpu."""
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


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    assert semstereo_amd.engine.CONV_ENGINE == "f16x3" and semstereo_amd.engine.DECODER_TRAIN_HIP is False
    return semstereo_amd


@pytest.fixture
def switch_on(sa, monkeypatch):
    monkeypatch.setattr(sa.engine, "DECODER_TRAIN_HIP", True)
    return sa


def _td():
    return __import__("semstereo_amd.train_decoder", fromlist=["x"])


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- the autograd function of the transposed conv, called directly ------------------------------------------------------------------

# (B, Cin, Cout, H, W, bias): every dimension ragged and a 32-column tile crossed; the shape class of spx2 (with its bias); a row-tile
# boundary and exactly two column tiles; every tap in the halo; more than one partial per weight tile; a layer large enough for the
# data gradient's 8-row tile (two rows per wave: `_data_gradient_workgroups` >= 256), ragged in every dimension
SHAPES = [(2, 24, 40, 5, 37, False), (1, 128, 6, 8, 8, True), (1, 64, 32, 33, 64, False), (3, 8, 8, 1, 1, False), (2, 16, 16, 40, 70, False),
          (2, 520, 8, 66, 70, False)]
_CASES = {}


def _data_gradient_workgroups(Cin, H, W):
    """What ss_conv2d_k4s2_f16s_fwd chooses its tile by: the workgroups one element offers with the 8-row tile (32 gradient channels x 8
    rows x 32 columns each).  From 256 up the layer runs the 8-row tile, below it the 4-row tile."""
    return -(-W // 32) * -(-H // 8) * -(-Cin // 32)


def test_the_shapes_reach_both_tiles_of_the_data_gradient():
    sizes = [_data_gradient_workgroups(Cin, H, W) for _, Cin, _, H, W, _ in SHAPES]
    assert min(sizes) < 256 <= max(sizes), sizes
    assert _data_gradient_workgroups(520, 66, 70) >= 256 and _data_gradient_workgroups(264, 80, 70) >= 256       # (used below)
    assert _data_gradient_workgroups(40, 9, 37) < 256 and _data_gradient_workgroups(64, 33, 64) < 256


def _case(shape):
    """Inputs, the float64 CPU results and the fp32 CPU layer's results of one shape, computed once and shared (never modified)."""
    if shape not in _CASES:
        B, Cin, Cout, H, W, has_bias = shape
        g = _gen(7 * Cin + 3 * Cout + 100 * H + W)
        x = torch.randn(B, Cin, H, W, generator=g)
        w = (torch.rand(Cin, Cout, 4, 4, generator=g) * 2 - 1) * (3.0 / (4 * Cin)) ** 0.5
        bias = (torch.rand(Cout, generator=g) * 0.2 - 0.1) if has_bias else None
        G = torch.randn(B, Cout, 2 * H, 2 * W, generator=g)
        refs = []
        for dtype in (torch.float64, torch.float32):
            ts = [None if t is None else t.detach().clone().to(dtype).requires_grad_(True) for t in (x, w, bias)]
            out = F.conv_transpose2d(ts[0], ts[1], ts[2], stride=2, padding=1)
            grads = torch.autograd.grad(out, [t for t in ts if t is not None], G.to(dtype))
            res = {"out": out.detach(), "grad_x": grads[0], "grad_w": grads[1]}
            if has_bias:
                res["grad_bias"] = grads[2]
            refs.append(res)
        _CASES[shape] = (x, w, bias, G, refs[0], refs[1])
    return _CASES[shape]


def _hip(sa, x, w, bias, G, need=(True, True, True)):
    """_Deconv2dK4S2 forward + backward on device copies -> {"out", "grad_x", "grad_w", "grad_bias"} (None where not requested)."""
    TD = _td()
    xs = [None if t is None else t.detach().cuda().contiguous().requires_grad_(n) for t, n in zip((x, w, bias), need)]
    out = TD._Deconv2dK4S2.apply(*xs)
    if out.requires_grad:
        out.backward(G.cuda())
    torch.cuda.synchronize()
    return {"out": out.detach(), "grad_x": xs[0].grad, "grad_w": xs[1].grad, "grad_bias": None if xs[2] is None else xs[2].grad}


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s[:5])) for s in SHAPES])
def test_functions_against_float64(sa, shape):
    """The forward and each gradient: max |err| <= 2e-5 max |ref| (what tests/train_calls.py::BOUNDS gives train._Conv2dK3), or at most
    1.5 x the stock fp32 layer's own error against float64."""
    x, w, bias, G, f64, f32 = _case(shape)
    got = _hip(sa, x, w, bias, G)
    for k, r in f64.items():
        assert got[k] is not None and got[k].shape == r.shape, (shape, k)
        err, e32, scale = float((got[k].double().cpu() - r).abs().max()), float((f32[k].double() - r).abs().max()), float(r.abs().max())
        print(f"deconv {shape} {k:9s} max err {err:.3e} fp32 cpu {e32:.3e} max |ref| {scale:.3e} ratio {err / max(scale, 1e-30):.2e}")
        assert err <= 2e-5 * scale or err <= 1.5 * e32, (shape, k, err, scale, e32)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[4]], ids=str)
def test_adjoint_identity(sa, shape):
    """Without a bias D is bilinear in (x, w): <G, D x> = <D^T G, x> = <grad_w, w>, evaluated in float64 from the GPU's outputs, each to
    1e-5 of the inner product itself."""
    x, w, _, G, _, _ = _case(shape)
    got = _hip(sa, x, w, None, G)
    lhs = float((got["out"].double().cpu() * G.double()).sum())
    rx, rw = float((x.double() * got["grad_x"].double().cpu()).sum()), float((w.double() * got["grad_w"].double().cpu()).sum())
    print(f"adjoint {shape}: <G,Dx> {lhs:.9e} <DtG,x> {rx:.9e} <gw,w> {rw:.9e} relative {abs(lhs - rx) / abs(lhs):.2e} {abs(lhs - rw) / abs(lhs):.2e}")
    assert abs(lhs - rx) <= 1e-5 * abs(lhs) and abs(lhs - rw) <= 1e-5 * abs(lhs), (shape, lhs, rx, rw)


def test_bit_identities(sa):
    """Two calls of the weight gradient give the same bits; an element's data gradient has the same bits alone and in a batch of 3."""
    for (Cin, Cout, H, W) in ((16, 16, 40, 70), (24, 40, 5, 37), (64, 32, 33, 64), (520, 8, 66, 70)):      # (the last: the 8-row tile)
        g = _gen(H * W + Cin)
        x = torch.randn(3, Cin, H, W, generator=g)
        w = torch.randn(Cin, Cout, 4, 4, generator=g) * 0.1
        G = torch.randn(3, Cout, 2 * H, 2 * W, generator=g) * torch.tensor([1.0, 40.0, 1e-3]).reshape(3, 1, 1, 1)
        first, second = _hip(sa, x, w, None, G), _hip(sa, x, w, None, G)
        assert torch.equal(first["grad_w"], second["grad_w"]) and torch.equal(first["grad_x"], second["grad_x"]), (Cin, Cout, H, W)
        for b in range(3):
            alone = _hip(sa, x[b:b + 1], w, None, G[b:b + 1], need=(True, False, False))
            assert torch.equal(alone["grad_x"], first["grad_x"][b:b + 1]), (Cin, Cout, H, W, b)


def _record(sa, monkeypatch):
    E, symbols = sa.engine, []
    real_call = E.call
    monkeypatch.setattr(E, "call", lambda name, *a: (symbols.append((name, a)), real_call(name, *a))[1])
    return symbols


def _names(symbols):
    return [n for n, _ in symbols]


def test_only_the_gradients_autograd_needs_are_computed(sa, monkeypatch):
    x, w, bias, G, _, _ = _case(SHAPES[1])
    symbols = _record(sa, monkeypatch)
    DG, WG, BG = "ss_conv2d_k4s2_f16s_fwd", "ss_deconv2d_k4s2_wgrad_fwd", "ss_channel_sum_fwd"
    full = _hip(sa, x, w, bias, G)
    assert [_names(symbols).count(n) for n in (DG, "ss_pack_conv2d_k4s2_weights_f16s", WG, BG, "ss_deconv2d_bf16s_fwd")] == [1, 1, 1, 1, 1]
    for need in ((True, False, True), (False, True, True), (True, True, False), (False, False, True), (False, True, False)):
        del symbols[:]
        got = _hip(sa, x, w, bias, G, need=need)
        assert [_names(symbols).count(n) for n in (DG, WG, BG)] == [int(v) for v in need], need
        assert _names(symbols).count("ss_pack_conv2d_k4s2_weights_f16s") == int(need[0])
        for k, v in zip(("grad_x", "grad_w", "grad_bias"), need):
            assert (got[k] is not None) == v and (not v or torch.equal(got[k], full[k])), (need, k)


def test_nan_and_inf_stay_in_their_receptive_field(sa):
    """A value of grad_out at (r, c) reaches grad_in[:, y, x] with 2y - 1 <= r <= 2y + 2 and 2x - 1 <= c <= 2x + 2, and no other position."""
    # the 4-row tile (spots at a row-tile and a column-tile boundary), then the 8-row tile (a wave's two rows, the row-tile boundary)
    for (B, Cin, Cout, H, W), spot_sets in (
            ((2, 40, 12, 9, 37), (((0, 0),), ((7, 63), (8, 64)), ((2 * 9 - 1, 2 * 37 - 1), (5, 30)))),
            ((2, 264, 12, 80, 70), (((0, 0), (2 * 80 - 1, 2 * 70 - 1)), ((15, 63), (16, 64)), ((2, 30), (3, 31), (45, 139))))):
        g = _gen(78 + H)
        x, w = torch.randn(B, Cin, H, W, generator=g), torch.randn(Cin, Cout, 4, 4, generator=g) * 0.1
        G = torch.randn(B, Cout, 2 * H, 2 * W, generator=g)
        clean = _hip(sa, x, w, None, G, need=(True, False, False))["grad_x"].cpu()
        ys, xs = torch.arange(H).reshape(H, 1), torch.arange(W).reshape(1, W)
        for bad in (float("nan"), float("inf"), float("-inf")):
            for spots in spot_sets:
                Gb = G.clone()
                hit = torch.zeros(B, Cin, H, W, dtype=torch.bool)
                for k, (r, c) in enumerate(spots):
                    Gb[1, (5 * k + 3) % Cout, r, c] = bad
                    hit[1] |= ((2 * ys - 1 <= r) & (r <= 2 * ys + 2) & (2 * xs - 1 <= c) & (c <= 2 * xs + 2)).unsqueeze(0)
                assert 0 < int(hit[1, 0].sum()) <= 4 * len(spots)
                got = _hip(sa, x, w, None, Gb, need=(True, False, False))["grad_x"].cpu()
                assert bool((~torch.isfinite(got[hit])).all()), (H, bad, spots)
                assert torch.equal(got[~hit], clean[~hit]), (H, bad, spots)


def test_each_gradient_seam_falls_back_to_the_stock_gradient_alone(sa, monkeypatch):
    """train_decoder.DGRAD_HIP / WGRAD_HIP = False sends that gradient to aten.convolution_backward: it stays within the bound, the other
    gradient still comes from its kernel (same entry point, same bits), and the bias gradient is untouched."""
    TD = _td()
    DG, WG = "ss_conv2d_k4s2_f16s_fwd", "ss_deconv2d_k4s2_wgrad_fwd"
    for shape in (SHAPES[0], SHAPES[1]):
        x, w, bias, G, f64, f32 = _case(shape)
        symbols = _record(sa, monkeypatch)
        both = _hip(sa, x, w, bias, G)
        for seam, stock_key, kept_key, stock_call, kept_call in (("DGRAD_HIP", "grad_x", "grad_w", DG, WG), ("WGRAD_HIP", "grad_w", "grad_x", WG, DG)):
            with monkeypatch.context() as mp:
                mp.setattr(TD, seam, False)
                del symbols[:]
                got = _hip(sa, x, w, bias, G)
            assert _names(symbols).count(stock_call) == 0 and _names(symbols).count(kept_call) == 1, (seam, _names(symbols))
            assert _names(symbols).count("ss_pack_conv2d_k4s2_weights_f16s") == int(seam == "WGRAD_HIP")
            assert torch.equal(got[kept_key], both[kept_key]) and torch.equal(got["out"], both["out"]), seam
            if bias is not None:
                assert torch.equal(got["grad_bias"], both["grad_bias"]), seam
            r = f64[stock_key]
            err, e32, scale = float((got[stock_key].double().cpu() - r).abs().max()), float((f32[stock_key].double() - r).abs().max()), float(r.abs().max())
            gap = float((got[stock_key] - both[stock_key]).abs().max())
            print(f"seam {seam} {shape}: stock {stock_key} max err {err:.3e} fp32 cpu {e32:.3e} max |ref| {scale:.3e}; against the kernel {gap:.3e}")
            assert got[stock_key].shape == r.shape and (err <= 2e-5 * scale or err <= 1.5 * e32), (seam, shape, err, scale, e32)
            # (each of the two is within max(2e-5 max |ref|, 1.5 x the fp32 layer's error) of the float64 result)
            assert gap <= 2 * max(2e-5 * scale, 1.5 * e32), (seam, shape, gap, scale, e32)
        monkeypatch.undo()


# ---- the layers through the twins, the switch on ---------------------------------------------------------------------------------

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
    """The criterion of test_heads_train_gpu._check: 2e-5 max |ref| or 1.5 x the fp32 CPU layer's error; buffers to 1e-6 relative, the
    batch counter equal."""
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


def _conv2x_case():
    x, rem = torch.randn(2, 16, 6, 10, generator=_gen(11)), torch.randn(2, 8, 12, 20, generator=_gen(12))
    wt = torch.randn(2, 16, 12, 20, generator=_gen(13))
    return x, rem, wt


def test_conv2x_twin_in_train_against_float64(switch_on):
    """This fails without the feature: a train() call of the twin used to run the stock layers."""
    sa = switch_on
    M = sa.modules
    base = dc.fill(M.Conv2x(16, 8, deconv=True), 61).train()
    x, rem, wt = _conv2x_case()
    m64, m32, mg = copy.deepcopy(base).double(), copy.deepcopy(base), copy.deepcopy(base).cuda()
    r64, r32 = _run_layer(m64, (x, rem), wt, "cpu", torch.float64), _run_layer(m32, (x, rem), wt, "cpu", torch.float32)
    before = dict(M.PATH_COUNTS)
    rg = _run_layer(mg, (x, rem), wt, "cuda", torch.float32)
    torch.cuda.synchronize()
    assert M.PATH_COUNTS.get("hip_train", 0) > before.get("hip_train", 0) and M.PATH_COUNTS["torch"] == before["torch"]
    assert M.PATH_COUNTS.get("decoder_train", 0) == before.get("decoder_train", 0) + 1
    _check(rg, r64, r32)


def test_routing(sa, monkeypatch):
    M, E = sa.modules, sa.engine
    x, rem, _ = _conv2x_case()
    x, rem = x.cuda(), rem.cuda()
    symbols = _record(sa, monkeypatch)

    def fresh():
        # (a train() forward moves the running statistics, not the output: every comparison starts from the same module)
        return dc.fill(M.Conv2x(16, 8, deconv=True), 61).cuda().train(), dc.fill(M.Spx2(16, 6), 62).cuda().train()

    def counts(fn):
        b = dict(M.PATH_COUNTS)
        y = fn()
        return (y, M.PATH_COUNTS.get("hip_train", 0) - b.get("hip_train", 0), M.PATH_COUNTS.get("decoder_train", 0) - b.get("decoder_train", 0),
                M.PATH_COUNTS["torch"] - b["torch"], M.PATH_COUNTS["hip"] - b["hip"])

    # inference, the switch off: the bits the inference kernels give
    c2x, spx2 = fresh()
    with torch.no_grad():
        y_inf, s_inf = c2x.eval()(x, rem), spx2.eval()(x)
    monkeypatch.setattr(E, "DECODER_TRAIN_HIP", True)
    for mode in (True, False):                                   # train(), and eval() with parameters that require grad
        c2x, spx2 = fresh()
        c2x.train(mode), spx2.train(mode)
        del symbols[:]
        y, h, d, t, i = counts(lambda: c2x(x, rem))
        assert h >= 1 and (d, t, i) == (1, 0, 0) and y.requires_grad, (mode, h, d, t, i)
        assert _names(symbols).count("ss_deconv2d_bf16s_fwd") == 1 and _names(symbols).count("ss_conv2d_bf16s_cat_fwd") == 1
        y.sum().backward()
        assert _names(symbols).count("ss_deconv2d_k4s2_wgrad_fwd") == 1 and "ss_conv2d_k4s2_f16s_fwd" not in _names(symbols)   # (x needs no gradient)
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in c2x.parameters())
        s, h, d, t, i = counts(lambda: spx2(x.clone().requires_grad_(True)))
        assert (h, d, t, i) == (1, 1, 0, 0) and s.requires_grad
    c2x, spx2 = fresh()
    y_hip, s_hip = c2x(x, rem).detach(), spx2(x).detach()
    # ... an inference call still takes the inference kernels, with unchanged bits
    c2x, spx2 = fresh()
    with torch.no_grad():
        y, h, d, t, i = counts(lambda: c2x.eval()(x, rem))
        assert (h, d, t, i) == (0, 0, 0, 1) and torch.equal(y, y_inf)
        s, h, d, t, i = counts(lambda: spx2.eval()(x))
        assert (h, d, t, i) == (0, 0, 0, 1) and torch.equal(s, s_inf)

    # anything else: the stock layers, counted, with the same values
    def stock(what, c2, sp, xx, rr):
        y, h, d, t, i = counts(lambda: c2(xx, rr))
        assert (h, d, t, i) == (0, 0, 2, 0), (what, h, d, t, i)
        if y.shape == y_hip.shape:
            assert torch.allclose(y.detach().float().cpu(), y_hip.cpu(), atol=2e-5, rtol=1e-5), what
        s, h, d, t, i = counts(lambda: sp(xx))
        assert (h, d, t, i) == (0, 0, 1, 0), (what, h, d, t, i)
        assert torch.allclose(s.detach().float().cpu(), s_hip.cpu(), atol=2e-5, rtol=1e-5), what

    for name, value in (("DECODER_TRAIN_HIP", False), ("TRAIN_HIP", False), ("CONV_ENGINE", "f32"), ("DECODER_HIP", False)):
        with monkeypatch.context() as mp:
            mp.setattr(E, name, value)
            stock(name, *fresh(), x, rem)
    c2x, spx2 = fresh()
    stock("cpu", c2x.cpu(), spx2.cpu(), x.cpu(), rem.cpu())
    c2x, spx2 = fresh()
    stock("float64", c2x.double(), spx2.double(), x.double(), rem.double())
    c2x, spx2 = fresh()
    stock("non-contiguous", c2x, spx2, x.transpose(2, 3).contiguous().transpose(2, 3), rem)
    c2x, _ = fresh()
    y, h, d, t, i = counts(lambda: c2x(x, rem[:, :, :11].contiguous()))            # a skip map of another size: the F.interpolate branch
    assert (h, d, t, i) == (0, 0, 2, 0) and tuple(y.shape) == (2, 16, 11, 20)


def test_featup_in_train_equals_the_per_view_calls(switch_on):
    sa = switch_on
    M = sa.modules
    base = dc.fill(M.FeatUp(), dc.FEATUP_SALT).train()
    featL, featR = ([t.cuda() for t in f] for f in dc.featup_inputs())
    fu, pv = copy.deepcopy(base).cuda(), copy.deepcopy(base).cuda()
    before = dict(M.PATH_COUNTS)
    L, R = fu(featL, featR)
    assert M.PATH_COUNTS["torch"] == before["torch"] and M.PATH_COUNTS["decoder_train"] == before.get("decoder_train", 0) + 8
    xs, ys = list(featL), list(featR)
    for k, name in zip((3, 2, 1, 0), ("deconv32_16", "deconv16_8", "deconv8_4", "deconv4_2")):
        m = getattr(pv, name)
        xs[k], ys[k] = m(xs[k + 1], xs[k]), m(ys[k + 1], ys[k])           # the left view, then the right one (models/SemStereo.py:74-84)
    for k in range(5):
        assert torch.equal(L[k], xs[k]) and torch.equal(R[k], ys[k]), k
    for (ka, a), (kb, b) in zip(fu.state_dict().items(), pv.state_dict().items()):
        assert ka == kb and torch.equal(a, b), ka
        if ka.endswith("num_batches_tracked"):
            assert int(a) == 2, ka


def _fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "decoder_train.npz"))


def _check_fixture(case, res, fx):
    """The bound of the stand-in model's train step, per recorded array: 1e-4 max(1, max |ref|)."""
    for key, t in res.items():
        name = f"{case}/{key}"
        if key.endswith("num_batches_tracked"):
            assert int(t) == int(fx[name][0]), name
            continue
        err, big, dsum, dsq = tc.compare(t, fx[name], tc.salt_of(name))
        tol = 1e-4 * max(1.0, big)
        print(f"fixture {name}: max err {err:.2e} max |ref| {big:.3e} sum {dsum:.2e} sum of squares {dsq:.2e}")
        assert err <= tol and dsum <= tol and dsq <= 2 * tol, (name, err, big, dsum, dsq)


def test_golden_training_cases_on_hip(switch_on):
    """The cases of decoder_train.npz (the reference's own layers in train(), float64) with the twins on the kernels."""
    sa = switch_on
    M, fx = sa.modules, _fixture()
    before = dict(M.PATH_COUNTS)
    for name, (Cin, Cout, _) in tc.CONV2X.items():
        mod = dc.fill(M.Conv2x(Cin, Cout, deconv=True), tc.SALTS[name])
        _check_fixture(name, tc.run(mod, tc.conv2x_inputs(name), name, dtype=torch.float32, device="cuda"), fx)
    mod = dc.fill(M.Spx2(tc.SPX2[0], tc.SPX2[1]), tc.SALTS["spx2"])
    _check_fixture("spx2", tc.run(mod, [tc.spx2_input()], "spx2", dtype=torch.float32, device="cuda"), fx)
    assert M.PATH_COUNTS["torch"] == before["torch"] and M.PATH_COUNTS["decoder_train"] == before.get("decoder_train", 0) + 3


# ---- the whole decoder of the stand-in model ------------------------------------------------------------------------------------

class _Decoder(torch.nn.Module):
    """FeatUp on both views, the chal_* projections, the spx chain and spx2 of tests/decoder_model.py as the stand-in's forward wires
    them (models/SemStereo.py:252-271), on pyramid features."""

    def __init__(self, net):
        super().__init__()
        self.feature_up, self.spx2 = net.feature_up, net.spx2
        for n in ("chal_0", "chal_1", "chal_2", "chal_3", "chal_4", "spx32_16", "spx16_8", "spx8_4", "spx4_2"):
            setattr(self, n, getattr(net, n))

    def forward(self, *feats):
        fl, fr = self.feature_up(list(feats[:5]), list(feats[5:]))
        c = [getattr(self, f"chal_{i}")(fl[i]) for i in range(5)]
        x = self.spx32_16(c[4], c[3])
        x = self.spx16_8(x, c[2])
        x = self.spx8_4(x, c[1])
        x = self.spx4_2(x, c[0])
        return torch.cat((self.spx2(x).flatten(1), fr[0].flatten(1)), 1)


def test_train_step_of_the_standin_decoder(switch_on):
    import decoder_model
    from oracle import detdata as dd
    sa = switch_on
    M = sa.modules
    base = dc.fill(_Decoder(decoder_model.DecoderStandIn(64, M, twins=True)), 71).train()
    B, H, W = 2, 64, 96
    feats = [dd.t_normalish((B, c, H >> (k + 1), W >> (k + 1)), 1500 + 10 * v + k) for v in range(2) for k, c in enumerate(dc.CHANS)]
    m64, mg = copy.deepcopy(base).double(), copy.deepcopy(base).cuda()
    with torch.no_grad():
        wt = dd.t_normalish(tuple(copy.deepcopy(base)(*feats).shape), 1530)
    r64 = _run_layer(m64, feats, wt, "cpu", torch.float64)
    before = dict(M.PATH_COUNTS)
    rg = _run_layer(mg, feats, wt, "cuda", torch.float32)
    torch.cuda.synchronize()
    assert M.PATH_COUNTS["torch"] == before["torch"]
    assert M.PATH_COUNTS["decoder_train"] == before.get("decoder_train", 0) + 8 + 4 + 1        # FeatUp per view, the spx chain, spx2
    worst = 0.0
    for k, ref in r64.items():
        if k.startswith("buf:"):
            if k.endswith("num_batches_tracked"):
                assert int(rg[k]) == int(ref) == (2 if k.startswith("buf:feature_up") else 1), k
            continue
        err, scale = float((rg[k].double().cpu() - ref).abs().max()), float(ref.abs().max())
        worst = max(worst, err / max(1.0, scale))
        assert err <= 1e-4 * max(1.0, scale), (k, err, scale)
    print(f"stand-in decoder train step: {len(r64)} arrays, worst error / max(1, max |ref|) {worst:.2e}")
