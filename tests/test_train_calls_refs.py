"""CPU checks of the per-call checker (tests/train_calls.py): its float64 references agree with the stock F.* / oracle compositions in
float64, and every seam it wraps is the name the call site actually reads -- a renamed or moved function must fail here, not leave the
GPU checker with nothing to check."""
import inspect

import pytest
import torch
import torch.nn.functional as F

import train_calls as TC
from oracle import detdata as dd
from oracle import ops as oops
from oracle import stack as ostack

TOL = 1e-12


def _rel(a, ref):
    a, ref = a.detach(), ref.detach()
    return float((a - ref).abs().max()) / (float(ref.abs().max()) + 1e-300)


def _d(t, grad=False):
    return t.double().clone().requires_grad_(grad)


@pytest.mark.parametrize("shape,relu,with_res", [((2, 8, 3, 5, 7), True, True), ((3, 4, 6, 9), False, False), ((1, 6, 4, 5, 6), True, False)])
def test_batchnorm_reference_matches_f_batch_norm(shape, relu, with_res):
    C = shape[1]
    x = _d(dd.t_normalish(shape, 601) * 2 + 0.3, True)
    w, b = _d(dd.t_uniform((C,), 602, 0.5, 1.5), True), _d(dd.t_uniform((C,), 603, -0.3, 0.3), True)
    res = _d(dd.t_normalish(shape, 604), True) if with_res else None
    y, mean, var_u, _ = TC.batchnorm_ref(x, w, b, 1e-5, relu, res)
    want = F.batch_norm(x, None, None, w, b, True, 0.0, 1e-5)
    want = want + res if with_res else want
    want = F.relu(want) if relu else want
    assert _rel(y, want) <= TOL
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    F.batch_norm(x.detach(), rm, rv, None, None, True, 1.0, 1e-5)            # momentum 1: the running statistics become the batch's
    assert _rel(mean, rm) <= TOL and _rel(var_u, rv) <= TOL
    go = dd.t_normalish(shape, 605).double()
    ins = [x, w, b] + ([res] if with_res else [])
    g_ref = torch.autograd.grad(y, ins, go)
    g_want = torch.autograd.grad(want, ins, go)
    assert all(_rel(a, r) <= TOL for a, r in zip(g_ref, g_want))
    # the mask taken from an output: the same function where the output is the float64 one
    y2, _, _, _ = TC.batchnorm_ref(x, w, b, 1e-5, relu, res, (want > 0) if relu else None)
    assert _rel(y2, want) <= TOL


def test_convolution_references_match_autograd_of_f_conv():
    x = _d(dd.t_normalish((2, 5, 4, 6, 8), 611), True)
    w = _d(dd.t_uniform((7, 5, 3, 3, 3), 612, -0.3, 0.3), True)
    for stride in (1, 2):
        y = F.conv3d(x, w, None, stride, 1)
        assert _rel(TC.conv_ref(x, w, stride), y) <= TOL
        g = dd.t_normalish(tuple(y.shape), 613).double()
        gx, gw = torch.autograd.grad(y, (x, w), g)
        assert _rel(TC.wgrad_ref(g, x.detach(), 7, 5, stride), gw) <= TOL
        if stride == 1:      # the data gradient as _Conv3dK3.backward forms it: the same convolution, taps flipped, channel axes swapped
            assert _rel(TC.conv_ref(g, w.detach().transpose(0, 1).flip(2, 3, 4), 1), gx) <= TOL
        else:                # ... stride 2: the transposed convolution of the output gradient
            assert _rel(TC.deconv_ref(g, w.detach()), gx) <= TOL
    xd = _d(dd.t_normalish((1, 6, 2, 3, 5), 614), True)
    wd = _d(dd.t_uniform((6, 4, 3, 3, 3), 615, -0.3, 0.3), True)
    yd = F.conv_transpose3d(xd, wd, None, stride=2, padding=1, output_padding=1)
    assert _rel(TC.deconv_ref(xd, wd), yd) <= TOL
    g = dd.t_normalish(tuple(yd.shape), 616).double()
    gx, gw = torch.autograd.grad(yd, (xd, wd), g)
    assert _rel(TC.conv_ref(g, wd.detach(), 2), gx) <= TOL                            # _Deconv3dK3.backward's data gradient
    assert _rel(TC.wgrad_ref(xd.detach(), g, 6, 4, 2), gw) <= TOL                    # ... and weight gradient, roles swapped


def test_pointwise_references_match():
    x5, x4 = _d(dd.t_normalish((2, 6, 3, 4, 5), 621)), _d(dd.t_normalish((2, 6, 4, 5), 622))
    w, b = _d(dd.t_uniform((9, 6, 1, 1, 1), 623, -0.4, 0.4)), _d(dd.t_uniform((9,), 624))
    assert _rel(TC.k1_ref(x5, w, b), torch.einsum("oc,bcdhw->bodhw", w.reshape(9, 6), x5) + b.reshape(1, 9, 1, 1, 1)) <= TOL
    assert _rel(TC.k1_ref(x4, w.reshape(9, 6, 1, 1), None), torch.einsum("oc,bchw->bohw", w.reshape(9, 6), x4)) <= TOL
    w2 = _d(dd.t_uniform((5, 6, 3, 3), 625, -0.3, 0.3))
    assert _rel(TC.conv2d_k3_ref(x4, w2), F.conv2d(x4, w2, None, 1, 1)) <= TOL
    wp = _d(dd.t_uniform((6, 1, 1, 3, 3), 626, -1, 1))
    assert _rel(TC.patch_ref(x5, wp), F.conv3d(x5, wp, None, 1, (0, 1, 1), 1, 6)) <= TOL
    att = _d(dd.t_normalish((2, 6, 4, 5), 627))
    assert _rel(TC.gate_ref(att, x5), torch.sigmoid(att)[:, :, None] * x5) <= TOL


@pytest.mark.parametrize("block,shape", [((4, 4, 4), (1, 128, 8, 8, 12)), ((4, 4, 4), (1, 128, 8, 6, 10)), ((6, 4, 4), (1, 128, 6, 8, 9)),
                                         ((4, 4, 4), (2, 128, 4, 7, 8))])
def test_window_attention_core_reference_matches_the_oracle_block(block, shape):
    """The core on qkv = Linear(x) over the real positions, with the bias as the pad tokens' q / k / v, then final1x1 = the oracle's
    attention_block, which pads x with zeros before the Linear -- both pad masks, the `-0:` quirk, no padding."""
    C = shape[1]
    key = "a"
    P = {key + ".qkv_3d.weight": dd.t_uniform((3 * C, C), 631, -0.1, 0.1).double(), key + ".qkv_3d.bias": dd.t_uniform((3 * C,), 632, -0.1, 0.1).double(),
         key + ".final1x1.weight": dd.t_uniform((C, C, 1, 1, 1), 633, -0.1, 0.1).double(), key + ".final1x1.bias": dd.t_uniform((C,), 634, -0.1, 0.1).double()}
    x = _d(dd.t_normalish(shape, 635))
    want = ostack.attention_block(P, key, x, block)
    qkv = TC.k1_ref(x, P[key + ".qkv_3d.weight"], P[key + ".qkv_3d.bias"])
    core = TC.window_core_ref(qkv, P[key + ".qkv_3d.bias"], 16, block)
    got = TC.k1_ref(core, P[key + ".final1x1.weight"], P[key + ".final1x1.bias"])
    assert _rel(got, want) <= TOL


def test_attention_tail_references_match_the_oracle_composition():
    m, B, Hc, Wc, K = 8, 2, 5, 7, 6
    H, W, D, rng = 2 * Hc, 2 * Wc, 2 * m, (-m, 2 * m)
    coarse = _d(dd.t_normalish((B, 1, m, Hc, Wc), 641) * 2)
    up, disp, var = TC.upsoft_ref(coarse, H, W, rng)
    upr = F.interpolate(coarse, [D, H, W], mode="trilinear")
    pr = F.softmax(upr.squeeze(1), dim=1)
    dispr = oops.disparity_regression(pr, m)
    assert _rel(up, upr) <= TOL and _rel(disp, dispr) <= TOL and _rel(var, oops.disparity_variance(pr, m, dispr.unsqueeze(1))) <= TOL
    logits = _d(dd.t_normalish((B, 1, D, H, W), 642) * 3.0)
    strength = torch.softmax(_d(dd.t_normalish((B, 5, H, W), 643)), dim=1)
    aw = (oops.propagation_prob(logits) * strength.unsqueeze(2)).sum(dim=1, keepdim=True)
    prob = F.softmax(aw, dim=2)
    ind_k = prob.sort(dim=2, descending=True, stable=True)[1][:, :, :K].sort(2, False)[0]
    smp = ind_k.squeeze(1).double() - m
    att, pred, own, gap = TC.topk_ref(logits, strength, K, rng, smp)
    assert torch.equal(own.double(), smp) and bool((gap >= 0).all())
    assert _rel(att, torch.gather(prob, 2, ind_k)) <= TOL
    assert _rel(pred, (F.softmax(torch.gather(aw, 2, ind_k).squeeze(1), dim=1) * smp).sum(dim=1)) <= TOL


def _grid_sample_on(y, d):
    """F.grid_sample in float64 on a grid that un-normalises to the fp32 coordinates of train_calls.warp_coords32."""
    B, C, H, W = y.shape
    ix, iy = TC.warp_coords32(d, H, W)
    grid = torch.stack([ix.double() / ((W - 1.0) / 2.0) - 1.0, iy.double() / ((H - 1.0) / 2.0) - 1.0], dim=4).reshape(B, -1, W, 2)
    return F.grid_sample(y, grid, mode="bilinear", padding_mode="zeros", align_corners=True).reshape(B, C, d.shape[1], H, W)


@pytest.mark.parametrize("kind", ["frac", "int"])
def test_warp_reference_matches_grid_sample_on_the_fp32_coordinates(kind):
    B, C, H, W, nd = 2, 5, 6, 37, 7
    y = _d(dd.t_normalish((B, C, H, W), 651), True)
    if kind == "int":
        d = dd.distinct_sorted_candidates(B, nd, H, W, 20, 652)
    else:
        d = torch.round(dd.t_uniform((B, nd, H, W), 652, -20.0, 20.0)) + dd.t_uniform((B, nd, H, W), 653, 0.2, 0.8)
    got, want = TC.warp_ref(y, d), _grid_sample_on(y, d)
    assert _rel(got, want) <= TOL
    g = dd.t_normalish(tuple(want.shape), 654).double()
    assert _rel(torch.autograd.grad(got, y, g)[0], torch.autograd.grad(want, y, g)[0]) <= TOL
    # the fp32 coordinates are the reference's round trip: within fp32 rounding of (w - d, h), not equal to it
    ix, iy = TC.warp_coords32(d, H, W)
    cols = torch.arange(W, dtype=torch.float64).reshape(1, 1, 1, W)
    assert float((ix.double() - (cols - d.double())).abs().max()) <= 1e-4
    # the gradient to the candidates (frac: away from the tap edges) is d/dd of the bilinear form: -dy/dix
    if kind == "frac":
        dd_ = d.double().clone().requires_grad_(True)
        s = (TC.warp_ref(y.detach(), d, dd_) * g).sum()
        got_gd = torch.autograd.grad(s, dd_)[0]
        grid_d = _d(d, True)
        Bq, Cq, Hq, Wq = y.shape
        gx_ = (torch.arange(Wq, dtype=torch.float64).reshape(1, 1, 1, Wq) - grid_d) / ((Wq - 1.0) / 2.0) - 1.0
        gy_ = (torch.arange(Hq, dtype=torch.float64).reshape(1, 1, Hq, 1).expand_as(gx_)) / ((Hq - 1.0) / 2.0) - 1.0
        ws = F.grid_sample(y.detach(), torch.stack([gx_, gy_], dim=4).reshape(Bq, -1, Wq, 2), mode="bilinear", padding_mode="zeros",
                           align_corners=True).reshape(Bq, Cq, nd, Hq, Wq)
        want_gd = torch.autograd.grad((ws * g).sum(), grid_d)[0]
        assert _rel(got_gd, want_gd) <= 1e-6          # (taps at the float64 coordinates: the same cells, row weights ~1e-6 apart)


def test_concat_strength_gwc_references_match_the_oracle():
    B, C, H, W, nd = 1, 6, 4, 20, 5
    left, right = _d(dd.t_normalish((B, C, H, W), 661)), _d(dd.t_normalish((B, C, H, W), 662))
    d = dd.distinct_sorted_candidates(B, nd, H, W, 8, 663)
    att = _d(dd.t_uniform((B, 1, nd, H, W), 664, 0.0, 1.0))
    want = att * torch.cat((left.unsqueeze(2).expand(B, C, nd, H, W), _grid_sample_on(right, d)), dim=1)
    assert _rel(TC.concat_ref(left, right, d, att), want) <= TOL
    yw, xw = TC.warp_sampled_ref(left, right, d)
    assert _rel(yw, _grid_sample_on(right, d)) <= TOL and torch.equal(xw, left.unsqueeze(2).expand_as(xw))
    pred0 = torch.round(dd.t_uniform((B, H, W), 665, -5.0, 5.0)) + dd.t_uniform((B, H, W), 666, 0.2, 0.8)
    var = _d(dd.t_uniform((B, 1, H, W), 667, 0.0, 20.0))
    gamma, beta = torch.tensor([0.25], dtype=torch.float64), torch.tensor([2.0], dtype=torch.float64)
    cand = oops.propagation(pred0.unsqueeze(1).double())
    v = torch.sigmoid(beta + gamma * var)
    want_s = torch.softmax((left.unsqueeze(2) * _grid_sample_on(right, cand)).mean(dim=1) * oops.propagation(v), dim=1)
    assert _rel(TC.strength_ref(left, right, pred0.double(), var, gamma, beta), want_s) <= TOL
    a, b = _d(dd.t_normalish((2, 16, 5, 12), 671)), _d(dd.t_normalish((2, 16, 5, 12), 672))
    assert _rel(TC.gwc_ref(a, b, (-4, 8), 4), oops.build_gwc_volume(a, b, 4, 4)) <= TOL
    assert _rel(TC.gwc_ref(TC.group_normalise_ref(a, 4), TC.group_normalise_ref(b, 4), (-4, 8), 4), oops.build_gwc_volume_norm(a, b, 4, 4)) <= TOL
    c = _d(dd.t_normalish((2, 8, 5, 12), 673))
    s = _d(dd.t_uniform((2, 8, 5, 12), 674, -10, 10))
    assert _rel(TC.regression_topk_ref(c, s, 2), oops.regression_topk(c, s, 2)) <= TOL


# ---- the seams are the names the call sites read ---------------------------------------------------------------------------------

def test_leaf_seams_are_read_from_train_layers_globals():
    import semstereo_amd as sa
    TL = sa.train_layers
    reads = {
        TL._Conv3dK3.forward: {"_conv_k3_forward"},
        TL._Conv3dK3.backward: {"_conv_k3_forward", "_deconv_k3_forward", "conv3d_wgrad_hip"},
        TL._Deconv3dK3.forward: {"_deconv_k3_forward"},
        TL._Deconv3dK3.backward: {"_conv_k3_forward", "conv3d_wgrad_hip"},
    }
    for fn, names in reads.items():
        assert names <= set(fn.__code__.co_names), (fn.__qualname__, fn.__code__.co_names)
        assert fn.__globals__ is vars(TL)
    assert set(TC.LEAF_SEAMS) == set().union(*reads.values())
    # _Conv2dK3's weight gradient goes through modules (train._M()): that name is a seam of its own
    assert "conv3d_wgrad_hip" in sa.train._Conv2dK3.backward.__code__.co_names and "_M" in sa.train._Conv2dK3.backward.__code__.co_names
    assert sa.train._M() is sa.modules and callable(sa.modules.conv3d_wgrad_hip)


CALLERS = {"_BatchNormTrain": "train.batchnorm_train", "_ConvK1": "train.conv_k1", "_Conv2dK3": "train.conv2d_k3",
           "_DepthwisePatch": "train.depthwise_patch", "_ChannelGate": "train.channel_gate", "_WindowAttentionCore": "train.window_attention",
           "_UpsampleSoftmaxRegression": "train.attention_tail", "_SampleStrength": "train.attention_tail",
           "_TopkCandidates": "train.attention_tail", "_ConcatVolumeSampled": "train.concat_volume_sampled",
           "_GwcVolume": "ops._build_gwc_volume_norm", "_GroupNormalise": "ops._group_normalise", "_WarpSampled": "ops.SpatialTransformer_grid",
           "_RegressionTopk": "ops.regression_topk"}


def test_function_seams_are_the_classes_the_call_sites_apply():
    import semstereo_amd as sa
    assert {c for _m, c in TC.FUNCTION_SEAMS} == set(CALLERS)
    for modname, cls_name in TC.FUNCTION_SEAMS:
        mod = getattr(sa, modname)
        cls = getattr(mod, cls_name)
        assert issubclass(cls, torch.autograd.Function)
        assert "forward" in vars(cls) and "backward" in vars(cls), cls_name       # (patched on the class: autograd looks both up there)
        cmod, cfn = CALLERS[cls_name].split(".")
        caller = inspect.unwrap(getattr(getattr(sa, cmod), cfn))
        assert cls_name in caller.__code__.co_names and caller.__globals__ is vars(mod), (cls_name, caller.__code__.co_names)
    assert TC.STEP_SEAMS <= {f"train_layers.{n}" for n in TC.LEAF_SEAMS} | {"modules.conv3d_wgrad_hip"} | {f"{m}.{c}" for m, c in TC.FUNCTION_SEAMS}
    assert set(TC.BOUNDS) == {f"train_layers.{n}" for n in TC.LEAF_SEAMS} | {"modules.conv3d_wgrad_hip"} | {f"{m}.{c}" for m, c in TC.FUNCTION_SEAMS}


def test_recorder_installs_on_every_seam_and_monkeypatch_undoes_it(monkeypatch):
    import semstereo_amd as sa
    TL, M = sa.train_layers, sa.modules
    orig = {n: getattr(TL, n) for n in TC.LEAF_SEAMS}
    orig_fn = {(m, c): (vars(getattr(getattr(sa, m), c))["forward"], vars(getattr(getattr(sa, m), c))["backward"]) for m, c in TC.FUNCTION_SEAMS}
    with monkeypatch.context() as mp:
        TC.Recorder(sa).install(mp)
        for n in TC.LEAF_SEAMS:
            assert getattr(TL, n) is not orig[n] and getattr(TL, n).__wrapped__ is orig[n]
        assert M.conv3d_wgrad_hip.__wrapped__ is orig["conv3d_wgrad_hip"]
        for (m, c), (f, b) in orig_fn.items():
            cls = getattr(getattr(sa, m), c)
            assert cls.forward.__wrapped__ is f.__func__ and cls.backward.__wrapped__ is b.__func__
    assert all(getattr(TL, n) is orig[n] for n in TC.LEAF_SEAMS) and M.conv3d_wgrad_hip is orig["conv3d_wgrad_hip"]
