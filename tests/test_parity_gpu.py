"""GPU parity: the HIP path (through the C ABI) against the CPU oracle on the same inputs and
against the golden fixtures produced by the reference.  Run on the MI355X box: pytest -m gpu.

Tolerances (fp32 everywhere):
  * dense concat volume, broadcast halves, propagation, depthwise patch: BIT-EXACT (pure data movement);
  * gwc volumes, regressions, top-k regression, warps: <= 1e-6 absolute + 1e-6 relative to the
    largest reference value (fp32 summation order / sqrt / div / exp rounding differ between the
    host's vectorised ATen kernels and the GPU; measured 6e-8 .. 4e-7 on O(1) values);
  * 3-D stack modules: <= 2e-4 absolute on O(1) activations (different fp32 summation order over
    K = 864..3456 products);
  * hot segment: candidate indices identical, pred / pred_att within 1e-3 px (the EPE target of
    BASELINE.json) of the reference fixture.
"""
import json
import os

import numpy as np
import pytest
import torch

from golden import cases
from oracle import hot_segment as oseg
from oracle import ops as oops
from oracle import stack as ostack

pytestmark = pytest.mark.gpu

REPORT = {}


def dev(t):
    return t.cuda()


def maxerr(a, ref):
    a = a.detach().float().cpu()
    ref = torch.as_tensor(ref).float()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    both_nan = torch.isnan(a) & torch.isnan(ref)
    d = (a - ref).abs()
    d[both_nan] = 0
    return float(d.max()) if d.numel() else 0.0


def check(name, a, ref, atol, rtol=0.0):
    e = maxerr(a, ref)
    REPORT[name] = e
    scale = float(torch.as_tensor(ref).float().abs().nan_to_num(0.0).max()) if rtol else 0.0
    assert e <= atol + rtol * scale, f"{name}: max abs err {e:.3e} > {atol:.1e} + {rtol:.1e}*{scale:.3g}"


@pytest.fixture(scope="module", autouse=True)
def _dump_report():
    yield
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/parity_report.json", "w") as f:
        json.dump(REPORT, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    return semstereo_amd


@pytest.mark.parametrize("name", sorted(cases.GWC))
def test_gwc(sa, golden, name):
    a, b, m, G = cases.gwc_inputs(name)
    g = golden["ops"]
    check(f"gwc/{name}", sa.ops.build_gwc_volume(dev(a), dev(b), m, G), g[f"gwc/{name}"], 1e-6)
    check(f"gwc_norm/{name}", sa.ops.build_gwc_volume_norm(dev(a), dev(b), m, G), g[f"gwc_norm/{name}"], 2e-6)
    check(f"gcorr/{name}", sa.ops.groupwise_correlation(dev(a), dev(b), G), g[f"gcorr/{name}"], 1e-6)
    check(f"gcorr_norm/{name}", sa.ops.groupwise_correlation_norm(dev(a), dev(b), G), g[f"gcorr_norm/{name}"], 2e-6)


@pytest.mark.parametrize("shape", [(2, 256, 24, 128, 16, 32), (1, 64, 9, 256, 24, 8), (1, 32, 5, 260, 8, 8)])
def test_gwc_vs_oracle_fast_path(sa, shape):
    """The float4/LDS kernel (W % 4 == 0, maxdisp % 4 == 0, Cg in {4, 8}) incl. multi-tile W."""
    from oracle import detdata as dd
    B, C, H, W, m, G = shape
    a, b = dd.t_normalish((B, C, H, W), 11), dd.t_normalish((B, C, H, W), 12)
    check(f"gwc_fast/{shape}", sa.ops.build_gwc_volume(dev(a), dev(b), m, G), oops.build_gwc_volume(a, b, m, G), 1e-6)
    check(f"gwc_norm_fast/{shape}", sa.ops.build_gwc_volume_norm(dev(a), dev(b), m, G),
          oops.build_gwc_volume_norm(a, b, m, G), 2e-6)


def test_gwc_streaming_stores_identical(sa, tuning_env):
    """Volumes beyond the infinity cache are written with nontemporal stores: same bits either way."""
    from oracle import detdata as dd
    a, b = dd.t_normalish((1, 64, 9, 256, ), 13), dd.t_normalish((1, 64, 9, 256), 14)
    outs = []
    for flag in ("0", "1"):
        tuning_env("SS_GWC_STREAM", flag)
        outs.append(sa.ops.build_gwc_volume_norm(dev(a), dev(b), 24, 8).cpu())
    assert torch.equal(outs[0], outs[1])
    check("gwc_stream", outs[1], oops.build_gwc_volume_norm(a, b, 24, 8), 2e-6)


@pytest.mark.parametrize("name", sorted(cases.CONCAT))
def test_concat(sa, golden, name):
    a, b, m = cases.concat_inputs(name)
    check(f"concat/{name}", sa.ops.build_concat_volume(dev(a), dev(b), m), golden["ops"][f"concat/{name}"], 0.0)


def test_concat_fast_path(sa):
    from oracle import detdata as dd
    a, b = dd.t_normalish((2, 5, 11, 256, ), 21), dd.t_normalish((2, 5, 11, 256), 22)
    check("concat_fast", sa.ops.build_concat_volume(dev(a), dev(b), 12), oops.build_concat_volume(a, b, 12), 0.0)


@pytest.mark.parametrize("name", sorted(cases.REGRESSION))
def test_regression(sa, golden, name):
    p, m, d = cases.regression_inputs(name)
    check(f"regression/{name}", sa.ops.disparity_regression(dev(p), m), golden["ops"][f"regression/{name}"], 1e-6, 1e-6)
    check(f"variance/{name}", sa.ops.disparity_variance(dev(p), m, dev(d)), golden["ops"][f"variance/{name}"], 1e-6, 1e-6)
    with pytest.raises(AssertionError):
        sa.ops.disparity_regression(dev(p).unsqueeze(0), m)


def test_softmax_regression_fused(sa):
    from oracle import detdata as dd
    m = 32
    logits = dd.t_normalish((2, 2 * m, 12, 20), 31) * 4.0
    prob = torch.softmax(logits, dim=1)
    mean = oops.disparity_regression(prob, m)
    var = oops.disparity_variance(prob, m, mean.unsqueeze(1))
    d, v, p = sa.ops.softmax_regression(dev(logits), m, want_prob=True)
    check("fused_softmax/prob", p, prob, 1e-6)
    check("fused_softmax/mean", d, mean, 1e-6, 1e-6)
    check("fused_softmax/var", v, var, 1e-6, 2e-6)


@pytest.mark.parametrize("name", sorted(cases.WARP))
def test_warp(sa, golden, name):
    x, y, d = cases.warp_inputs(name)
    yw, xw = sa.ops.SpatialTransformer_grid(dev(x), dev(y), dev(d))
    check(f"warp_y/{name}", yw, golden["ops"][f"warp_y/{name}"], 1e-6, 1e-6)
    check(f"warp_x/{name}", xw, golden["ops"][f"warp_x/{name}"], 0.0)


def test_warp_fused_forms(sa):
    from oracle import detdata as dd
    B, C, H, W, nd = 2, 16, 12, 40, 6
    x, y = dd.t_normalish((B, C, H, W), 41), dd.t_normalish((B, C, H, W), 42)
    disp = dd.distinct_sorted_candidates(B, nd, H, W, 16, 43)
    att = dd.t_uniform((B, 1, nd, H, W), 44, 0.0, 1.0)
    yw, xw = oops.SpatialTransformer_grid(x, y, disp)
    check("concat_sampled", sa.ops.concat_volume_sampled(dev(x), dev(y), dev(disp), dev(att)),
          att * torch.cat((xw, yw), dim=1), 1e-6, 2e-6)
    check("concat_sampled_nogate", sa.ops.concat_volume_sampled(dev(x), dev(y), dev(disp)),
          torch.cat((xw, yw), dim=1), 1e-6, 2e-6)
    check("warp_correlation", sa.ops.warp_correlation(dev(x), dev(y), dev(disp)), (xw * yw).mean(dim=1), 1e-6, 2e-6)


def test_warp_streaming_stores_identical(sa, tuning_env):
    from oracle import detdata as dd
    B, C, H, W, nd = 1, 8, 6, 64, 5
    x, y = dd.t_normalish((B, C, H, W), 45), dd.t_normalish((B, C, H, W), 46)
    disp = dd.distinct_sorted_candidates(B, nd, H, W, 16, 47)
    att = dd.t_uniform((B, 1, nd, H, W), 48, 0.0, 1.0)
    outs = []
    for flag in ("0", "1"):
        tuning_env("SS_WARP_STREAM", flag)
        outs.append(sa.ops.concat_volume_sampled(dev(x), dev(y), dev(disp), dev(att)).cpu())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("shape", [(2, 8, 7, 64, 5), (1, 5, 9, 37, 3), (1, 4, 3, 2, 2), (1, 32, 4, 130, 24)])
@pytest.mark.parametrize("gated", [True, False])
def test_warp_right_half_fast_path(sa, shape, gated):
    """The live form of the concat volume (left half omitted, warp.hip: warp_right_gated -- one unconditional 8-byte load
    per tap row at a clamped column, selects instead of branches) against the oracle and, bit for bit, against the generic
    kernel: fractional disparities, disparities that push one or both taps of a row out of the image on either side,
    odd and minimal widths, W not a multiple of the 64-column workgroup."""
    from oracle import detdata as dd
    B, C, H, W, nd = shape
    y = dd.t_normalish((B, C, H, W), 151)
    disp = dd.t_uniform((B, nd, H, W), 152, -1.5 * W, 1.5 * W)
    disp[:, 0] = torch.round(disp[:, 0])                                    # integers too (the live case)
    disp[:, -1, :, 0] = 1.0                                                 # w - d = -1: only the east tap inside
    disp[:, -1, :, -1] = 0.0                                                # w - d = W - 1: only the west tap inside
    att = dd.t_uniform((B, 1, nd, H, W), 153, 0.0, 1.0) if gated else None
    yw, _ = oops.SpatialTransformer_grid(y, y, disp)
    ref = yw if att is None else att * yw
    out = sa.ops.concat_volume_sampled(None, dev(y), dev(disp), None if att is None else dev(att))
    # the same launch through the generic kernel: feed a left half and drop it
    both = sa.ops.concat_volume_sampled(dev(torch.zeros_like(y)), dev(y), dev(disp), None if att is None else dev(att))
    assert torch.equal(out, both[:, C:])
    # vs the oracle: the same fp32 coordinate round trip, operation by operation (r04: the products are really unfused now);
    # what is left is ATen's fused multiply-adds in the four-tap sum: one ulp of an O(1) value
    check(f"concat_sampled_right/{shape}/{gated}", out, ref, 2e-6)


def test_warp_float4_form_identical(sa, tuning_env):
    """SS_WARP_VEC=4 (4 columns per lane) against the default one-column-per-lane form, fractional disparities."""
    from oracle import detdata as dd
    B, C, H, W, nd = 2, 8, 7, 64, 5
    x, y = dd.t_normalish((B, C, H, W), 145), dd.t_normalish((B, C, H, W), 146)
    disp = dd.t_uniform((B, nd, H, W), 147, -9.0, 9.0)
    att = dd.t_uniform((B, 1, nd, H, W), 148, 0.0, 1.0)
    outs = []
    for flag in ("1", "4"):
        tuning_env("SS_WARP_VEC", flag)
        outs.append(sa.ops.concat_volume_sampled(dev(x), dev(y), dev(disp), dev(att)).cpu())
    assert torch.equal(outs[0], outs[1])
    yw, xw = oops.SpatialTransformer_grid(x, y, disp)
    check("concat_sampled_fractional", outs[0], att * torch.cat((xw, yw), dim=1), 2e-6)


@pytest.mark.parametrize("W", [256, 512])
def test_warp_follows_grid_sample_at_the_bench_widths(sa, W):
    """Round 4.  The reference's coordinate round trip leaves ix = (w - d) + delta with |delta| up to ~W * 1e-7, and the last
    rounding of that arithmetic snaps most ix back onto the integer.  Until r04 the `unfused` helpers of the kernels were still
    contracted by hipcc (`ix - floor(ix)` became an fma on the UNROUNDED product): invisible at the fixtures' W = 16, it moved
    the bilinear weights by up to 4e-5 at W = 256 (8e-5 at 512), made only 7 % of the warped values bit-equal to
    F.grid_sample's and put the whole HIP path 3x further from the float64 answer than the reference itself.  Held here at the
    quarter-resolution widths of the bench shapes: integer candidates (the live :316 call) and fractional ones (:291), the
    generic kernel, the live right-half kernel and the 5-candidate probe."""
    g = torch.Generator().manual_seed(W)
    B, C, H, nd, m4 = 1, 8, 6, 24, W // 8
    x, y = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    smp = torch.stack([torch.randperm(2 * m4, generator=g)[:nd].sort()[0].float() - m4 for _ in range(H * W)], 1).reshape(B, nd, H, W)
    att = torch.rand(B, 1, nd, H, W, generator=g)
    yw, xw = oops.SpatialTransformer_grid(x, y, smp)
    yw64, _ = oops.SpatialTransformer_grid(x.double(), y.double(), smp.double())
    got, _ = sa.ops.SpatialTransformer_grid(dev(x), dev(y), dev(smp))
    got = got.cpu()
    same = float((got == yw).float().mean())
    REPORT[f"warp_bitwise_equal_fraction/W{W}"] = same
    assert same >= 0.85, f"only {same:.3f} of the warped values equal F.grid_sample's bit for bit"
    check(f"warp_bench_width/W{W}", got, yw, 6e-7)
    # ... and therefore exactly as far from the exact gather (float64 coordinates) as the reference's own arithmetic
    e_hip, e_ref = (got.double() - yw64).pow(2).mean().sqrt().item(), (yw.double() - yw64).pow(2).mean().sqrt().item()
    assert e_hip <= 1.02 * e_ref + 1e-9, (e_hip, e_ref)
    right = sa.ops.concat_volume_sampled(None, dev(y), dev(smp), dev(att))
    check(f"warp_right_gated_bench_width/W{W}", right, att * yw, 6e-7)
    # the probe of :291-293: fractional candidates around a regressed disparity
    pred0 = (torch.rand(B, H, W, generator=g) - 0.5) * 2 * m4
    var = torch.rand(B, 1, H, W, generator=g) * 30
    gamma, beta = torch.tensor([0.25]), torch.tensor([2.0])
    rw, lb = oops.SpatialTransformer_grid(x, y, oops.propagation(pred0.unsqueeze(1)))
    strength = torch.softmax((lb * rw).mean(dim=1) * oops.propagation(torch.sigmoid(beta + gamma * var)), dim=1)
    check(f"sample_strength_bench_width/W{W}", sa.ops.sample_strength(dev(x), dev(y), dev(pred0), dev(var), dev(gamma), dev(beta)),
          strength, 1e-6)


@pytest.mark.parametrize("name", sorted(cases.TOPK))
def test_topk(sa, golden, name):
    c, s, k = cases.topk_inputs(name)
    check(f"topk/{name}", sa.ops.regression_topk(dev(c), dev(s), k), golden["ops"][f"topk/{name}"], 1e-6, 1e-6)


def test_topk_generic_k_and_ties(sa):
    from oracle import detdata as dd
    c = dd.t_normalish((1, 12, 5, 7), 51)
    s = dd.distinct_sorted_candidates(1, 12, 5, 7, 16, 52)
    check("topk/k6", sa.ops.regression_topk(dev(c), dev(s), 6), oops.regression_topk(c, s, 6), 1e-5)
    c[:, 3] = c[:, 1]           # exact ties: lower index first, like the oracle's stable sort
    check("topk/ties", sa.ops.regression_topk(dev(c), dev(s), 2), oops.regression_topk(c, s, 2), 1e-5)


@pytest.mark.parametrize("H,W", [(2, 2), (3, 2), (2, 3), (5, 3), (4, 65)])      # (H or W = 1: the reference itself divides by W - 1 = 0)
def test_sample_strength_on_narrow_maps(sa, H, W):
    """The probe fetches the west / east taps of a row as one 8-byte pair: pairs at the first and last element of a plane, both
    taps / one tap / no tap inside, a wave that spans several rows (W = 65)."""
    from oracle import detdata as dd
    B, C = 2, 8
    left, right = dd.stereo_features(B, C, H, W, 5, max_shift=1)
    pred0 = dd.t_uniform((B, H, W), 311, -2.5, 2.5)
    var = dd.t_uniform((B, 1, H, W), 312, 0.0, 30.0)
    gamma, beta = torch.tensor([0.25]), torch.tensor([2.0])
    rw, lb = oops.SpatialTransformer_grid(left, right, oops.propagation(pred0.unsqueeze(1)))
    strength = torch.softmax((lb * rw).mean(dim=1) * oops.propagation(torch.sigmoid(beta + gamma * var)), dim=1)
    got = sa.ops.sample_strength(dev(left), dev(right), dev(pred0), dev(var), dev(gamma), dev(beta))
    check(f"sample_strength_narrow/{H}x{W}", got, strength, 1e-6, 1e-6)


@pytest.mark.parametrize("m", [16, 20, 32])      # D = 32, 64: register kernel; D = 40: generic LDS kernel
def test_attention_tail_fused_kernels(sa, m):
    """ss_sample_strength_fwd (:286-293) and ss_topk_candidates_fwd (:295-310) against the oracle's
    op-by-op composition of the same lines."""
    import torch.nn.functional as F
    from oracle import detdata as dd
    B, C, H, W, K = 2, 24, 11, 20, 24
    left, right = dd.stereo_features(B, C, H, W, 5, max_shift=4)
    pred0 = dd.t_uniform((B, H, W), 111, -6.0, 6.0)
    var = dd.t_uniform((B, 1, H, W), 112, 0.0, 30.0)
    gamma, beta = torch.tensor([0.25]), torch.tensor([2.0])
    v = torch.sigmoid(beta + gamma * var)
    rw, lb = oops.SpatialTransformer_grid(left, right, oops.propagation(pred0.unsqueeze(1)))
    strength = torch.softmax((lb * rw).mean(dim=1) * oops.propagation(v), dim=1)
    got = sa.ops.sample_strength(dev(left), dev(right), dev(pred0), dev(var), dev(gamma), dev(beta))
    check("sample_strength", got, strength, 1e-6, 1e-6)

    logits = dd.t_normalish((B, 1, 2 * m, H, W), 113) * 3.0
    aw = (oops.propagation_prob(logits) * strength.unsqueeze(2)).sum(dim=1, keepdim=True)
    prob = F.softmax(aw, dim=2)
    _, ind = prob.sort(dim=2, descending=True, stable=True)
    ind_k = ind[:, :, :K].sort(2, False)[0]
    att_topk = torch.gather(prob, 2, ind_k)
    samples = ind_k.squeeze(1).float() - m
    pred_att = (F.softmax(torch.gather(aw, 2, ind_k).squeeze(1), dim=1) * samples).sum(dim=1)
    a, s, p = sa.ops.topk_candidates(dev(logits), dev(strength), m, K)
    assert torch.equal(s.cpu(), samples), "candidate sets differ"
    check("topk_candidates/att_topk", a, att_topk, 1e-6, 1e-6)
    check("topk_candidates/pred_att", p, pred_att, 1e-5, 1e-6)
    # exact ties in probability (two identical logit planes): lower index wins, as in a stable sort
    logits[:, :, 7] = logits[:, :, 3]
    aw = (oops.propagation_prob(logits) * strength.unsqueeze(2)).sum(dim=1, keepdim=True)
    prob = F.softmax(aw, dim=2)
    _, ind = prob.sort(dim=2, descending=True, stable=True)
    samples = ind[:, :, :K].sort(2, False)[0].squeeze(1).float() - m
    _, s, _ = sa.ops.topk_candidates(dev(logits), dev(strength), m, K)
    assert torch.equal(s.cpu(), samples), "tie handling differs"


def test_channel_gate(sa):
    from oracle import detdata as dd
    att, cv = dd.t_normalish((2, 8, 6, 12), 61), dd.t_normalish((2, 8, 5, 6, 12), 62)
    check("channel_gate", sa.ops.channel_gate(dev(att), dev(cv)), torch.sigmoid(att).unsqueeze(2) * cv, 2e-6)


def test_cpu_tensor_is_an_error_not_a_fallback(sa):
    a, b, m, G = cases.gwc_inputs("odd")
    with pytest.raises(sa._lib.SemStereoHipError):
        sa.ops.build_gwc_volume(a, b, m, G)


def test_assertions_match_reference(sa):
    a, b, m, G = cases.gwc_inputs("odd")
    with pytest.raises(AssertionError):
        sa.ops.build_gwc_volume(dev(a), dev(b), m, 5)      # C % G != 0
    with pytest.raises(AssertionError):
        sa.ops.groupwise_correlation(dev(a), dev(b), 5)


# --------------------------------------------------------------------------------------
# backward of the volume builders / regressions (autograd.Function) vs the oracle's autograd
# --------------------------------------------------------------------------------------

def _grads(fn, inputs, seed_like):
    xs = [t.clone().requires_grad_(True) for t in inputs]
    y = fn(*xs)
    y.backward(seed_like(y))
    return [x.grad for x in xs]


def test_backward_gwc_concat_regression(sa):
    from oracle import detdata as dd
    a, b = dd.t_normalish((2, 16, 5, 12), 71), dd.t_normalish((2, 16, 5, 12), 72)
    for norm in (False, True):
        hip = sa.ops.build_gwc_volume_norm if norm else sa.ops.build_gwc_volume
        orc = oops.build_gwc_volume_norm if norm else oops.build_gwc_volume
        seed = dd.t_normalish((2, 4, 8, 5, 12), 73)
        gh = _grads(lambda p, q: hip(p, q, 4, 4), [dev(a), dev(b)], lambda y: dev(seed))
        go = _grads(lambda p, q: orc(p, q, 4, 4), [a, b], lambda y: seed)
        for i, (x, r) in enumerate(zip(gh, go)):
            check(f"bwd/gwc{'_norm' if norm else ''}/{i}", x, r, 2e-5)
    seed = dd.t_normalish((2, 32, 8, 5, 12), 74)
    gh = _grads(lambda p, q: sa.ops.build_concat_volume(p, q, 4), [dev(a), dev(b)], lambda y: dev(seed))
    go = _grads(lambda p, q: oops.build_concat_volume(p, q, 4), [a, b], lambda y: seed)
    for i, (x, r) in enumerate(zip(gh, go)):
        check(f"bwd/concat/{i}", x, r, 1e-5)
    p = torch.softmax(dd.t_normalish((2, 8, 5, 12), 75), dim=1)
    seed = dd.t_normalish((2, 5, 12), 76)
    gh = _grads(lambda q: sa.ops.disparity_regression(q, 4), [dev(p)], lambda y: dev(seed))
    go = _grads(lambda q: oops.disparity_regression(q, 4), [p], lambda y: seed)
    check("bwd/regression", gh[0], go[0], 1e-6)


# --------------------------------------------------------------------------------------
# 3-D stack
# --------------------------------------------------------------------------------------

def _segment(sa, maxdisp=64):
    seg = sa.HotSegment(maxdisp)
    P = oseg.deterministic_params()
    res = seg.load_state_dict(P, strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    assert all(k.endswith("num_batches_tracked") for k in res.missing_keys), res.missing_keys
    return seg.cuda().eval(), P


def _run_stack_module(seg, name, x):
    kind, shape, block = cases.STACK[name]
    mod = seg
    for part in kind.split("."):
        mod = getattr(mod, part)
    return mod(x)


@pytest.mark.parametrize("name", sorted(cases.STACK))
def test_stack_modules(sa, golden, name):
    seg, P = _segment(sa)
    before = dict(sa.modules.PATH_COUNTS)
    with torch.no_grad():
        y = _run_stack_module(seg, name, dev(cases.stack_input(name)))
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"], "the PyTorch training path ran in inference"
    assert sa.modules.PATH_COUNTS["hip"] > before["hip"]
    check(f"stack/{name}", y, golden["stack"][f"stack/{name}"], 2e-4)


CONV_CASES = [
    # (Cin, Cout, D, H, W, k, stride, relu, residual)
    (32, 32, 5, 9, 37, 3, 1, True, False),
    (32, 64, 6, 10, 34, 3, 2, True, False),
    (64, 64, 3, 8, 33, 3, 1, True, True),
    (64, 128, 4, 7, 40, 3, 2, False, False),
    (128, 128, 2, 5, 8, 3, 1, True, False),
    (64, 32, 3, 9, 66, 3, 1, True, False),
    (32, 32, 2, 6, 35, 1, 1, False, False),
    (64, 64, 2, 4, 32, 1, 1, False, True),
    (32, 1, 5, 9, 37, 3, 1, False, False),
    (6, 40, 3, 4, 9, 3, 1, False, False),       # odd channel counts: zero-filled chunk tails
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv3d_kernel(sa, case):
    import torch.nn.functional as F
    from oracle import detdata as dd
    Cin, Cout, D, H, W, k, stride, relu, use_res = case
    x = dd.t_normalish((2, Cin, D, H, W), 81)
    w = dd.t_uniform((Cout, Cin, k, k, k), 82, -1, 1) * (3.0 / (Cin * k ** 3)) ** 0.5
    scale, shift = dd.t_uniform((Cout,), 83, 0.5, 1.5), dd.t_uniform((Cout,), 84, -0.2, 0.2)
    ref = F.conv3d(x, w, None, stride, k // 2) * scale.reshape(1, -1, 1, 1, 1) + shift.reshape(1, -1, 1, 1, 1)
    res = dd.t_normalish(tuple(ref.shape), 85) if use_res else None
    if use_res:
        ref = ref + res
    if relu:
        ref = F.relu(ref)
    wp = sa.modules.pack_conv_weight(dev(w))
    y = sa.modules.conv3d_hip(dev(x), wp, dev(scale), dev(shift), k, stride, relu, None if res is None else dev(res))
    check(f"conv3d/{case}", y, ref, 2e-4)


@pytest.mark.parametrize("engine", ["f32", "bf16x6", "f16x3"])
def test_conv3d_fused_channel_gate(sa, engine):
    """concat_stem + concat_feature_att_4 (models/SemStereo.py:319-320) as ONE kernel:
    sigmoid(gate)[:, :, None] * relu(bn(conv(x)))."""
    import torch.nn.functional as F
    from oracle import detdata as dd
    Cin, Cout, D, H, W = 64, 32, 3, 9, 37
    x = dd.t_normalish((2, Cin, D, H, W), 191)
    w = dd.t_uniform((Cout, Cin, 3, 3, 3), 192, -1, 1) * (3.0 / (Cin * 27)) ** 0.5
    scale, shift = dd.t_uniform((Cout,), 193, 0.5, 1.5), dd.t_uniform((Cout,), 194, -0.2, 0.2)
    gate = dd.t_normalish((2, Cout, H, W), 195)
    ref = F.relu(F.conv3d(x, w, None, 1, 1) * scale.reshape(1, -1, 1, 1, 1) + shift.reshape(1, -1, 1, 1, 1))
    ref = torch.sigmoid(gate).unsqueeze(2) * ref
    if engine == "f32":
        y = sa.modules.conv3d_hip(dev(x), sa.modules.pack_conv_weight(dev(w)), dev(scale), dev(shift), 3, 1, True,
                                  None, dev(torch.sigmoid(gate)))
    else:
        nt = 19 if engine == "f16x3" else 6
        y = sa.modules.conv3d_bf16s_hip(dev(x), sa.modules.pack_conv_weight_bf16s(dev(w), nt), Cout, dev(scale), dev(shift),
                                        True, nt, None, dev(torch.sigmoid(gate)))
    check(f"conv3d_gate/{engine}", y, ref, 2e-5)


@pytest.mark.parametrize("shape", [((4, 4, 4), 8, 8, 12), ((6, 4, 4), 6, 8, 8), ((4, 4, 4), 4, 6, 7), ((6, 4, 4), 12, 5, 8),
                                   ((4, 4, 4), 4, 9, 3)])
def test_attention_block_forms_agree(sa, shape):
    """attention_block (models/submodule_other.py:790-837) in both HIP forms -- the fused one-kernel-per-window
    form and the three-launch form (projection, per-(window, 4 heads) attention, projection) -- against the
    oracle's restatement of the block, including H/W padding (both, one, none)."""
    from oracle import detdata as dd
    block, D, H, W = shape
    mod = sa.modules.attention_block(128, 16, block).cuda().eval()
    with torch.no_grad():
        for i, p in enumerate(mod.parameters()):
            a = (3.0 / 128) ** 0.5 if p.dim() > 1 else 0.2
            p.copy_(dev(dd.t_uniform(tuple(p.shape), 600 + i, -a, a)))
    x = dev(dd.t_normalish((2, 128, D, H, W), 610))
    old = sa.modules.ATTENTION_FORM
    outs = {}
    try:
        with torch.no_grad():
            for form in ("split", "fused"):
                sa.engine.ATTENTION_FORM = form
                outs[form] = mod(x)
    finally:
        sa.engine.ATTENTION_FORM = old
    # the reference: the ORACLE's restatement of the block (oracle/stack.py, pinned to the reference's fixtures attn_pad /
    # attn_pad_w), not the module's own PyTorch path
    P = {"ab." + k: v.detach().cpu() for k, v in mod.state_dict().items()}
    ref = ostack.attention_block(P, "ab", x.cpu(), block)
    for form in outs:
        check(f"attention_{form}/{shape}", outs[form], ref, 2e-5)
    with torch.no_grad():
        check(f"attention_torch_path/{shape}", mod._forward_torch(x), ref, 2e-5)       # the training path agrees too


@pytest.mark.parametrize("nterms", [6, 3])
@pytest.mark.parametrize("case", [(2, 128, 384, (3, 5, 7)), (1, 128, 128, (6, 16, 16)), (1, 64, 40, (1, 1, 33)), (1, 32, 32, (2, 9, 70))])
def test_pointwise_split_bf16(sa, case, nterms):
    """1x1x1 conv / Linear over channels (qkv_3d, final1x1 of attention_block) on the split-bf16 engine vs float64."""
    from oracle import detdata as dd
    B, Cin, Cout, sp = case
    x = dd.t_normalish((B, Cin) + sp, 291)
    w = dd.t_uniform((Cout, Cin), 292, -1, 1) * (3.0 / Cin) ** 0.5
    bias = dd.t_uniform((Cout,), 293, -0.2, 0.2)
    ref = torch.einsum("oc,bcdhw->bodhw", w.double(), x.double()) + bias.double().reshape(1, -1, 1, 1, 1)
    y = sa.modules.conv3d_pointwise_bf16s_hip(dev(x), sa.modules.pack_pointwise_weight_bf16s(dev(w)), Cout, None, dev(bias), False, nterms)
    e = float((y.double().cpu() - ref).abs().max())
    REPORT[f"pointwise_bf16x{nterms}/{case}"] = e
    assert e <= (2e-6 if nterms == 6 else 4e-5), e


@pytest.mark.parametrize("shape", [(2, 32, 24, 9, 37), (1, 32, 6, 5, 70), (1, 32, 32, 3, 3)])
def test_stem_by_halves_equals_the_full_convolution(sa, shape):
    """concat_stem on cat(att * left broadcast over the candidates, right volume) (models/SemStereo.py:241-244,
    316-320) computed by linearity -- 1x1 projection of the 2-D left map + 27 multiply-adds per output as the
    residual of the right half's conv -- against the float64 convolution of the materialised 64-channel volume."""
    if sa.modules.CONV_ENGINE == "f32":
        pytest.skip("SS_CONV_ENGINE=f32: the by-halves form exists on the split engines only")
    import torch.nn.functional as F
    from oracle import detdata as dd
    B, C, nd, H, W = shape
    left = dd.t_normalish((B, C, H, W), 301)
    right = dd.t_normalish((B, C, nd, H, W), 302)
    att = dd.t_uniform((B, 1, nd, H, W), 303, 0.0, 1.0)
    gate = dd.t_normalish((B, C, H, W), 304)
    stem = sa.modules.BasicConv(2 * C, C, is_3d=True, kernel_size=3, stride=1, padding=1)
    with torch.no_grad():
        stem.conv.weight.copy_(dd.t_uniform((C, 2 * C, 3, 3, 3), 305, -1, 1) * (3.0 / (2 * C * 27)) ** 0.5)
        stem.bn.weight.copy_(dd.t_uniform((C,), 306, 0.6, 1.4)); stem.bn.bias.copy_(dd.t_uniform((C,), 307, -0.1, 0.1))
        stem.bn.running_mean.copy_(dd.t_uniform((C,), 308, -0.1, 0.1)); stem.bn.running_var.copy_(dd.t_uniform((C,), 309, 0.6, 1.4))
    stem = stem.cuda().eval()
    vol = torch.cat((att * left.unsqueeze(2).expand(B, C, nd, H, W), right), dim=1)
    sc, sh = sa.modules.fold_bn(stem.bn)
    ref = F.conv3d(vol.double(), stem.conv.weight.detach().cpu().double(), None, 1, 1)
    ref = F.relu(ref * sc.cpu().double().reshape(1, -1, 1, 1, 1) + sh.cpu().double().reshape(1, -1, 1, 1, 1))
    ref = torch.sigmoid(gate.double()).unsqueeze(2) * ref
    with torch.no_grad():
        y = sa.modules.stem_of_broadcast_and_volume(stem, dev(left), dev(att), dev(right), torch.sigmoid(dev(gate)))
        full = stem(dev(vol), dev(gate))
    e_halves, e_full = float((y.double().cpu() - ref).abs().max()), float((full.double().cpu() - ref).abs().max())
    REPORT[f"stem_halves/{shape}"] = e_halves
    REPORT[f"stem_full/{shape}"] = e_full
    assert e_halves <= 2.0 * e_full + 1e-6, (e_halves, e_full)
    # the residual operand alone against the float64 convolution of the left half
    wl = stem.conv.weight.detach().cpu().double()[:, :C]
    want = F.conv3d((att * left.unsqueeze(2)).double(), wl, None, 1, 1)
    wq = stem.conv.weight.detach().float()[:, :C].reshape(C, C, 27).permute(2, 0, 1).reshape(27 * C, C)
    q = sa.modules.conv3d_pointwise_bf16s_hip(dev(left), sa.modules.pack_pointwise_weight_bf16s(wq), 27 * C, None, None, False, 6)
    got = sa.ops.stem_left(q, dev(att))
    assert float((got.double().cpu() - want).abs().max()) <= 2e-6
    # both forms of the residual (Q through HBM / on the fly) inside the whole stem
    old = sa.modules.STEM_LEFT_FUSED
    try:
        for flag in (False, True):
            sa.engine.STEM_LEFT_FUSED = flag
            with torch.no_grad():
                yy = sa.modules.stem_of_broadcast_and_volume(stem, dev(left), dev(att), dev(right), torch.sigmoid(dev(gate)))
            assert float((yy.double().cpu() - ref).abs().max()) <= 2.0 * e_full + 1e-6, flag
    finally:
        sa.engine.STEM_LEFT_FUSED = old


@pytest.mark.parametrize("shape", [(2, 32, 24, 9, 37), (1, 32, 6, 5, 70), (1, 32, 32, 3, 3), (1, 32, 24, 40, 96), (1, 32, 6, 13, 65)])
@pytest.mark.parametrize("gated", [True, False])
def test_stem_on_the_presplit_warped_half(sa, shape, gated):
    """models/SemStereo.py:316-320 with the warped half handed over PRE-SPLIT (ss_concat_sampled_presplit_fwd ->
    ss_conv3d_presplit_fwd: two fp16 terms per value with one block exponent per batch element, staged by LDS-DMA):
    (a) the pre-split volume decodes to the fp32 kernel's values to 2^-22 of the bound; (b) the stem on it equals the stem
    on the fp32 volume (on-the-fly split, per-tile exponents) to rounding, and is as close to the float64 convolution;
    shapes with ragged tiles in every direction, a depth that is not a multiple of the 4-plane tile, image borders."""
    if sa.modules.CONV_ENGINE != "f16x3":
        pytest.skip("the pre-split form exists for the f16x3 engine")
    import torch.nn.functional as F
    from oracle import detdata as dd
    B, C, nd, H, W = shape
    cl, cr = dd.t_normalish((B, C, H, W), 311), dd.t_normalish((B, C, H, W), 312) * 3.0
    samples = dd.distinct_sorted_candidates(B, nd, H, W, max(nd, W // 2), 313)
    att = dd.t_uniform((B, 1, nd, H, W), 314, 0.0, 0.7)
    gate = torch.sigmoid(dd.t_normalish((B, C, H, W), 315)) if gated else None
    stem = sa.modules.BasicConv(2 * C, C, is_3d=True, kernel_size=3, stride=1, padding=1)
    with torch.no_grad():
        stem.conv.weight.copy_(dd.t_uniform((C, 2 * C, 3, 3, 3), 316, -1, 1) * (3.0 / (2 * C * 27)) ** 0.5)
        stem.bn.weight.copy_(dd.t_uniform((C,), 317, 0.6, 1.4)); stem.bn.bias.copy_(dd.t_uniform((C,), 318, -0.1, 0.1))
        stem.bn.running_mean.copy_(dd.t_uniform((C,), 319, -0.1, 0.1)); stem.bn.running_var.copy_(dd.t_uniform((C,), 320, 0.6, 1.4))
    stem = stem.cuda().eval()
    with torch.no_grad():
        right = sa.ops.concat_volume_sampled(None, dev(cr), dev(samples), dev(att))            # fp32 [B,C,nd,H,W]
        xs, xexp = sa.ops.concat_volume_sampled_presplit(dev(cr), dev(samples), dev(att))
        # (a) decode: (hi + lo) * 2^(e - 141)
        e = xexp[:B].cpu()
        bound = (cr.abs().reshape(B, -1).max(dim=1).values * att.abs().reshape(B, -1).max(dim=1).values)
        assert bool(((torch.frexp(bound).exponent + 126) == e).all()), (e, bound)                # biased exponent of the bound
        terms = xs.view(torch.float16).reshape(B, C // 8, 2, nd, H, W, 8).float()
        dec = (terms[:, :, 0] + terms[:, :, 1]) * torch.pow(2.0, (xexp[:B].float() - 141.0)).reshape(B, 1, 1, 1, 1, 1)
        dec = dec.permute(0, 1, 5, 2, 3, 4).reshape(B, C, nd, H, W)
        err_dec = (dec - right).abs().reshape(B, -1).max(dim=1).values.cpu()
        assert bool((err_dec <= bound * 2.0 ** -21).all()), (err_dec, bound)
        # (b) the stem
        partial = sa.modules.stem_broadcast_half(stem, dev(cl), dev(att))
        g = None if gate is None else dev(gate)
        y_pre = sa.modules.stem_volume_half_presplit(stem, xs, xexp, partial, g)
        y_f32 = sa.modules.stem_volume_half(stem, right, partial, g)
    assert y_pre.shape == y_f32.shape == (B, C, nd, H, W)
    d = float((y_pre - y_f32).abs().max())
    REPORT[f"stem_presplit_vs_f32_volume/{shape}/{gated}"] = d
    assert d <= 2e-5, d
    vol = torch.cat((att * cl.unsqueeze(2).expand(B, C, nd, H, W), right.cpu()), dim=1)
    sc, sh = sa.modules.fold_bn(stem.bn)
    ref = F.conv3d(vol.double(), stem.conv.weight.detach().cpu().double(), None, 1, 1)
    ref = F.relu(ref * sc.cpu().double().reshape(1, -1, 1, 1, 1) + sh.cpu().double().reshape(1, -1, 1, 1, 1))
    if gate is not None:
        ref = gate.double().unsqueeze(2) * ref
    e_pre, e_f32 = float((y_pre.double().cpu() - ref).abs().max()), float((y_f32.double().cpu() - ref).abs().max())
    REPORT[f"stem_presplit/{shape}/{gated}"] = e_pre
    # (r04: the fp32-volume form of these small shapes runs the chunk-blocked accumulation now and is ~3x closer to float64 than
    # a single chain; the pre-split option keeps the chain)
    assert e_pre <= max(2.0 * e_f32 + 1e-6, 8e-6), (e_pre, e_f32)


@pytest.mark.parametrize("shape", [(2, 32, 24, 9, 37), (1, 32, 6, 5, 70), (1, 32, 32, 3, 3), (1, 32, 24, 40, 96), (1, 32, 6, 13, 65),
                                   (1, 32, 24, 96, 128),      # >= 512 four-row tiles: the 4 x 4 x 4 tile, single chain (the bench's form)
                                   (2, 32, 24, 64, 96),       # ... the same tile on a layer that is "small" per pair: chunk-blocked
                                   (1, 16, 6, 160, 160),      # 2 x 8 tile (depth not a multiple of 4), two chunks per tile
                                   (1, 32, 24, 17, 300)])     # columns pushed far outside the image on both sides
@pytest.mark.parametrize("gated", [True, False])
def test_stem_gathers_the_warped_half_in_its_staging(sa, shape, gated):
    """SURVEY.md section 8 f1, second half (models/SemStereo.py:241-244, 316-320): ss_conv3d_gather_fwd forms
    att * warp(right, integer candidates) while the conv stages its tiles -- one launch, no volume.  Against (a) the
    float64 convolution of the EXACT gather (which is what grid_sample computes for integer candidates in exact arithmetic):
    as close as the three-launch form (warp kernel -> volume -> conv) is to ITS float64 convolution; (b) the three-launch
    form itself: equal up to the reference's coordinate rounding in the warp (<= 1e-5 relative on a quarter of the columns
    / rows, see include/semstereo_hip.h) -- bounded here at 2e-4 absolute on O(1) outputs."""
    if sa.modules.CONV_ENGINE != "f16x3":
        pytest.skip("the gathered stem exists for the f16x3 engine")
    import torch.nn.functional as F
    from oracle import detdata as dd
    B, C, nd, H, W = shape
    cl, cr = dd.t_normalish((B, C, H, W), 331), dd.t_normalish((B, C, H, W), 332) * 3.0
    samples = dd.distinct_sorted_candidates(B, nd, H, W, max(nd, min(W // 2, 48)), 333)
    assert bool((samples == samples.round()).all())
    att = dd.t_uniform((B, 1, nd, H, W), 334, 0.0, 0.7)
    gate = torch.sigmoid(dd.t_normalish((B, C, H, W), 335)) if gated else None
    stem = sa.modules.BasicConv(2 * C, C, is_3d=True, kernel_size=3, stride=1, padding=1)
    with torch.no_grad():
        stem.conv.weight.copy_(dd.t_uniform((C, 2 * C, 3, 3, 3), 336, -1, 1) * (3.0 / (2 * C * 27)) ** 0.5)
        stem.bn.weight.copy_(dd.t_uniform((C,), 337, 0.6, 1.4)); stem.bn.bias.copy_(dd.t_uniform((C,), 338, -0.1, 0.1))
        stem.bn.running_mean.copy_(dd.t_uniform((C,), 339, -0.1, 0.1)); stem.bn.running_var.copy_(dd.t_uniform((C,), 340, 0.6, 1.4))
    stem = stem.cuda().eval()
    g = None if gate is None else dev(gate)
    with torch.no_grad():
        assert sa.modules.stem_gather_applies(stem, dev(cr), dev(samples)) and sa.ops.integer_candidates(dev(samples))
        # (the broadcast half's projection kernel is written for the model's 32 channels: the 16-channel case continues a stand-in)
        partial = sa.modules.stem_broadcast_half(stem, dev(cl), dev(att)) if C == 32 else dev(dd.t_normalish((B, C, nd, H, W), 341))
        y_g = sa.modules.stem_gather_half(stem, dev(cr), dev(samples), dev(att), partial, g)
        right = sa.ops.concat_volume_sampled(None, dev(cr), dev(samples), dev(att))
        y_3 = sa.modules.stem_volume_half(stem, right, partial, g)
        y_g0 = sa.modules.stem_gather_half(stem, dev(cr), dev(samples), dev(att), None, g)      # no partial sum
        y_30 = sa.modules.conv3d_bf16s_hip(right, sa.engine._stem_halves_params(stem, C)[2], C, *sa.modules.fold_bn(stem.bn), True, 19, None, g)
    assert y_g.shape == y_3.shape == (B, C, nd, H, W)
    # exact gather in float64
    idx = torch.arange(W).reshape(1, 1, 1, W) - samples.long()                               # [B,nd,H,W]
    ok = (idx >= 0) & (idx < W)
    gathered = torch.gather(cr.unsqueeze(2).expand(B, C, nd, H, W), 4, idx.clamp(0, W - 1).unsqueeze(1).expand(B, C, nd, H, W))
    xg = (att * (gathered * ok.unsqueeze(1))).float()                                        # the reference's fp32 product (:318)
    sc, sh = sa.modules.fold_bn(stem.bn)
    w64 = stem.conv.weight.detach().cpu().double()

    def finish(acc):
        r = F.relu(acc * sc.cpu().double().reshape(1, -1, 1, 1, 1) + sh.cpu().double().reshape(1, -1, 1, 1, 1))
        return r if gate is None else gate.double().unsqueeze(2) * r
    left64 = F.conv3d((att * cl.unsqueeze(2)).float().double(), w64[:, :C], None, 1, 1) if C == 32 else partial.double().cpu()
    ref_g = finish(left64 + F.conv3d(xg.double(), w64[:, C:], None, 1, 1))
    ref_3 = finish(left64 + F.conv3d(right.cpu().double(), w64[:, C:], None, 1, 1))
    e_g, e_3 = float((y_g.double().cpu() - ref_g).abs().max()), float((y_3.double().cpu() - ref_3).abs().max())
    REPORT[f"stem_gather/{shape}/{gated}"] = e_g
    REPORT[f"stem_gather_three_launch/{shape}/{gated}"] = e_3
    assert e_g <= max(2.0 * e_3 + 1e-6, 8e-6), (e_g, e_3)
    ref_g0 = finish(F.conv3d(xg.double(), w64[:, C:], None, 1, 1))
    assert float((y_g0.double().cpu() - ref_g0).abs().max()) <= max(2.0 * e_3 + 1e-6, 8e-6)
    d = float((y_g - y_3).abs().max())
    REPORT[f"stem_gather_vs_three_launch/{shape}/{gated}"] = d
    assert d <= 2e-4, d
    assert float((y_g0 - y_30).abs().max()) <= 2e-4


def test_gathered_stem_is_only_taken_for_integer_candidates(sa, monkeypatch):
    """The precondition of ss_conv3d_gather_fwd is checked, not assumed: candidates produced by topk_candidates carry the mark,
    any other tensor is verified on the device; FRACTIONAL candidates (a caller of SpatialTransformer_grid may pass anything,
    models/submodule.py:265-288 is bilinear) keep the warp launch -- the matching branch then gives, bit for bit, what it gives
    with the gathered stem switched off."""
    if sa.modules.CONV_ENGINE != "f16x3":
        pytest.skip("the gathered stem exists for the f16x3 engine")
    from oracle import detdata as dd
    seg, _ = _segment(sa, 64)
    fl8, fr8 = dd.stereo_features(1, 256, 16, 24, 770, max_shift=3)
    fl4, fr4 = dd.stereo_features(1, 128, 32, 48, 771, max_shift=6)
    with torch.no_grad():
        r = seg(dev(fl4), dev(fr4), dev(fl8), dev(fr8))
        assert r["samples"]._ss_integer == (True, r["samples"]._version)
        whole = r["samples"].clone()                                   # an unmarked copy: verified on the device
        assert sa.ops.integer_candidates(whole) is True and whole._ss_integer[0] is True
        frac = r["samples"] + 0.25
        assert sa.ops.integer_candidates(frac) is False
        moved = r["samples"].clone()
        assert sa.ops.integer_candidates(moved) is True
        moved.add_(0.5)                                                # in place: the earlier verdict must not survive
        assert sa.ops.integer_candidates(moved) is False
        moved.sub_(0.5)
        assert sa.ops.integer_candidates(moved) is True
        calls = []
        real_gather = sa.modules.stem_gather_half
        monkeypatch.setattr(sa.modules, "stem_gather_half", lambda *a, **k: (calls.append(1), real_gather(*a, **k))[1])
        p_int = seg.matching_branch(dev(fl4), dev(fr4), r["att_topk"], whole)
        assert len(calls) == 1 and torch.equal(p_int, r["pred"])
        p_frac = seg.matching_branch(dev(fl4), dev(fr4), r["att_topk"], frac)
        assert len(calls) == 1, "fractional candidates must not reach the gather"
        monkeypatch.setattr(sa.engine, "STEM_GATHER", False)
        p_frac_3 = seg.matching_branch(dev(fl4), dev(fr4), r["att_topk"], frac)
    assert torch.equal(p_frac, p_frac_3)


def test_gathered_stem_on_degenerate_shapes(sa):
    """Edge cases of the gather: a two-row image, an image narrower than the 32-column tile, every candidate pointing outside the
    image (the operand is all zeros: the result is the partial sum through BatchNorm / ReLU / gate), candidates at +-(W - 1)."""
    if sa.modules.CONV_ENGINE != "f16x3":
        pytest.skip("the gathered stem exists for the f16x3 engine")
    from oracle import detdata as dd
    C = 32
    stem = sa.modules.BasicConv(2 * C, C, is_3d=True, kernel_size=3, stride=1, padding=1)
    with torch.no_grad():
        stem.conv.weight.copy_(dd.t_uniform((C, 2 * C, 3, 3, 3), 346, -1, 1) * (3.0 / (2 * C * 27)) ** 0.5)
    stem = stem.cuda().eval()
    # (H = 1: the reference's own warp is NaN there -- division by (H - 1) / 2 -- and the three-launch form keeps reproducing it)
    assert not sa.modules.stem_gather_applies(stem, torch.zeros(1, C, 1, 70, device="cuda"), torch.zeros(1, 24, 1, 70, device="cuda"))
    for (B, nd, H, W, lo, hi) in ((1, 24, 2, 70, -40, 40), (2, 6, 5, 9, -8, 9), (1, 24, 6, 40, 41, 90), (1, 4, 3, 33, -32, 33)):
        cr = dd.t_normalish((B, C, H, W), 347)
        g = torch.Generator().manual_seed(348)
        samples = torch.randint(lo, hi, (B, nd, H, W), generator=g).float().sort(dim=1).values
        att = dd.t_uniform((B, 1, nd, H, W), 349, 0.0, 1.0)
        partial = dd.t_normalish((B, C, nd, H, W), 350)
        gate = torch.sigmoid(dd.t_normalish((B, C, H, W), 351))
        with torch.no_grad():
            y = sa.modules.stem_gather_half(stem, dev(cr), dev(samples), dev(att), dev(partial), dev(gate))
            vol = sa.ops.concat_volume_sampled(None, dev(cr), dev(samples), dev(att))
            y3 = sa.modules.stem_volume_half(stem, vol, dev(partial), dev(gate))
        assert float((y - y3).abs().max()) <= 2e-4, (B, nd, H, W)
        if lo > W:                                               # nothing inside the image: exactly the partial sum's path
            assert float(vol.abs().max()) == 0.0
            sc, sh = sa.modules.fold_bn(stem.bn)
            want = dev(gate).unsqueeze(2) * torch.relu(dev(partial) * sc.reshape(1, -1, 1, 1, 1) + sh.reshape(1, -1, 1, 1, 1))
            assert float((y - want).abs().max()) <= 1e-6


HEAD_CASES = [
    # (B, Cin, D, H, W, relu): the 32 -> 1 classifier heads; W not a multiple of 30, both tile shapes, tiny volumes
    (2, 32, 5, 9, 37, False),
    (1, 32, 9, 70, 95, False),         # >= 1024 tiles of 4x8x30 -> the 4-plane tile
    (1, 16, 1, 1, 1, True),
    (1, 64, 3, 8, 31, False),
    (1, 32, 2, 3, 30, True),
]


@pytest.mark.parametrize("nterms", [6, 3, 19])
@pytest.mark.parametrize("case", HEAD_CASES)
def test_conv3d_head_split_bf16(sa, case, nterms):
    """classif.2 / classif_att_.2 (models/SemStereo.py:228-234) with the taps as matrix rows: as close to the
    float64 result as the exact-fp32 kernel (6 bf16 products, or the two-term fp16 form: nterms 19), within 4e-5
    absolute (3 bf16 products)."""
    import torch.nn.functional as F
    from oracle import detdata as dd
    B, Cin, D, H, W, relu = case
    x = dd.t_normalish((B, Cin, D, H, W), 281)
    w = dd.t_uniform((1, Cin, 3, 3, 3), 282, -1, 1) * (3.0 / (Cin * 27)) ** 0.5
    scale, shift = dd.t_uniform((1,), 283, 0.5, 1.5), dd.t_uniform((1,), 284, -0.2, 0.2)
    ref = F.conv3d(x.double(), w.double(), None, 1, 1) * scale.double() + shift.double()
    if relu:
        ref = F.relu(ref)
    y = sa.modules.conv3d_head_bf16s_hip(dev(x), sa.modules.pack_head_weight_bf16s(dev(w), nterms), dev(scale), dev(shift), relu, nterms)
    y32 = sa.modules.conv3d_hip(dev(x), sa.modules.pack_conv_weight(dev(w)), dev(scale), dev(shift), 3, 1, relu)
    e_split = float((y.double().cpu() - ref).abs().max())
    e_f32 = float((y32.double().cpu() - ref).abs().max())
    REPORT[f"conv3d_head_bf16x{nterms}/{case}"] = e_split
    REPORT[f"conv3d_head_f32_vs_f64/{case}"] = e_f32
    tol = 1.5 * e_f32 + 1e-6 if nterms in (6, 19) else 4e-5        # 3 bf16 products: ~1e-5 relative, absolute bound on O(1) outputs
    assert e_split <= tol, (e_split, e_f32)
    yn = sa.modules.conv3d_head_bf16s_hip(dev(x), sa.modules.pack_head_weight_bf16s(dev(w), nterms), None, None, False, nterms)
    refn = F.conv3d(x.double(), w.double(), None, 1, 1)
    assert float((yn.double().cpu() - refn).abs().max()) <= (4e-6 if nterms in (6, 19) else 4e-5)
    if nterms == 19:        # block floating point: rows 12 decades apart in either order keep the fp32 kernel's relative accuracy
        ramp = torch.logspace(-6, 6, H).reshape(1, 1, 1, H, 1)
        for rr in (ramp, ramp.flip(3)):
            xs = x * rr
            want = F.conv3d(xs.double(), w.double(), None, 1, 1)
            got = sa.modules.conv3d_head_bf16s_hip(dev(xs), sa.modules.pack_head_weight_bf16s(dev(w), 19), None, None, False, 19)
            g32 = sa.modules.conv3d_hip(dev(xs), sa.modules.pack_conv_weight(dev(w)), None, None, 3, 1, False)
            loc = torch.nn.functional.max_pool3d(xs.abs().amax(dim=1, keepdim=True), 3, 1, 1).double() + 1e-30     # the scale of each output's inputs
            e19 = float(((got.double().cpu() - want).abs() / loc).max())
            e32 = float(((g32.double().cpu() - want).abs() / loc).max())
            assert e19 <= 2.0 * e32 + 1e-7, (e19, e32)

@pytest.mark.parametrize("shape", [(2, 5, 9, 37), (1, 8, 24, 64), (1, 4, 70, 95), (1, 1, 1, 1), (1, 24, 64, 96)])
def test_classifier_channels_last_handoff_is_bit_identical(sa, shape, monkeypatch):
    """`classif` / `classif_att_` (models/SemStereo.py:228-234): the pair of launches that hands its intermediate over
    channels-last computes exactly what the plain-layout pair computes (same arithmetic, another address pattern), on every
    tile shape of the first layer (4x4x32, 2x8x32, 1x8x32, 1x4x32) and of the head, ragged widths included."""
    from oracle import detdata as dd
    B, D, H, W = shape
    m = sa.modules.Classifier(32).cuda().eval()
    with torch.no_grad():
        for i, p in enumerate(m.parameters()):
            p.copy_(dev(dd.t_uniform(tuple(p.shape), 900 + i, -1, 1) * (0.05 if p.dim() > 1 else 1.0)))
        m[0][1].running_mean.copy_(dev(dd.t_uniform((32,), 910, -0.1, 0.1)))
        m[0][1].running_var.copy_(dev(dd.t_uniform((32,), 911, 0.6, 1.4)))
    x = dev(dd.t_normalish((B, 32, D, H, W), 912))
    outs = []
    for flag in (True, False):
        monkeypatch.setattr(sa.engine, "CLASSIFIER_CL", flag)
        with torch.no_grad():
            outs.append(m(x))
    assert outs[0].shape == (B, 1, D, H, W)
    assert torch.equal(outs[0], outs[1])


def _det_classifier(sa, seed=900):
    from oracle import detdata as dd
    m = sa.modules.Classifier(32).cuda().eval()
    with torch.no_grad():
        for i, p in enumerate(m.parameters()):
            p.copy_(dev(dd.t_uniform(tuple(p.shape), seed + i, -1, 1) * (0.05 if p.dim() > 1 else 1.0)))
        m[0][1].running_mean.copy_(dev(dd.t_uniform((32,), seed + 10, -0.1, 0.1)))
        m[0][1].running_var.copy_(dev(dd.t_uniform((32,), seed + 11, 0.6, 1.4)))
    return m


@pytest.mark.parametrize("shape", [(1, 24, 128, 96), (2, 24, 64, 256)])
def test_classifier_patch_sum_folded_into_the_soft_argmax_is_bit_identical(sa, shape, monkeypatch):
    """VERDICT r5 #3 (the part built; off by default, it measured slower): `classif` -> regression_topk (models/SemStereo.py:322-323) with
    the one-pass classifier's patch sum inside the top-2 soft-argmax (ss_regression_topk_patched_fwd, SS_CLASSIFIER_FOLD=1) against the
    three-launch form: the same bits."""
    if sa.modules.CONV_ENGINE != "f16x3":
        pytest.skip("the one-pass classifier exists for the f16x3 engine")
    monkeypatch.setattr(sa.engine, "CLASSIFIER_FOLD", True)
    from oracle import detdata as dd
    B, D, H, W = shape
    cl = sa.modules.Classifier(32).cuda().eval()
    with torch.no_grad():
        for i, t in enumerate(list(cl.parameters()) + list(cl.buffers())):
            if t.dtype.is_floating_point:
                t.copy_(dev(dd.t_uniform(tuple(t.shape), 470 + i, 0.5, 1.5) if t.dim() == 1 else dd.t_uniform(tuple(t.shape), 470 + i, -0.06, 0.06)))
    x = dev(torch.relu(dd.t_normalish((B, 32, D, H, W), 480)))
    samples = dev(dd.distinct_sorted_candidates(B, D, H, W, 32, 481))
    with torch.no_grad():
        pc = cl.patches(x)
        assert pc is not None, "the one-pass form does not serve this shape"
        folded = sa.ops.regression_topk_patched(pc, samples, 2)
        plain = sa.ops.regression_topk(cl(x).squeeze(1), samples, 2)
    assert folded.shape == plain.shape == (B, 1, H, W) and torch.equal(folded, plain)
    # ... and exact ties between costs resolve to the lower candidate index in both forms (a zero input: every cost is the same number)
    with torch.no_grad():
        z = torch.zeros_like(x)
        assert torch.equal(sa.ops.regression_topk_patched(cl.patches(z), samples, 2), sa.ops.regression_topk(cl(z).squeeze(1), samples, 2))


@pytest.mark.parametrize("shape", [(1, 12, 134, 200), (2, 8, 140, 250), (1, 4, 300, 260), (1, 32, 128, 128)])
def test_classifier_one_pass_form_against_the_two_launch_form_and_float64(sa, shape, monkeypatch):
    """`classif` / `classif_att_` (models/SemStereo.py:228-234) in ONE pass over the volume (ss_conv3d_classifier_fused_fwd: the
    32-channel intermediate stays in the accumulators, tiles write patches of head outputs, a second launch adds them): ragged
    rows and columns (partial tiles), batch 2, a single 4-plane slab; against the two-launch form (same y bit for bit, the head's
    864 products summed in another order) and against float64 -- no further from it than the two-launch form is."""
    import torch.nn.functional as F
    from oracle import detdata as dd
    B, D, H, W = shape
    m = _det_classifier(sa)
    x = dev(dd.t_normalish((B, 32, D, H, W), 912))
    assert sa.engine.classifier_fused_applies(x, 19)
    outs = []
    for flag in (True, False):
        monkeypatch.setattr(sa.engine, "CLASSIFIER_FUSED", flag)
        with torch.no_grad():
            outs.append(m(x))
    assert outs[0].shape == (B, 1, D, H, W)
    scale = float(outs[1].abs().max())
    assert float((outs[0] - outs[1]).abs().max()) <= 4e-6 * scale
    md = _det_classifier(sa).double().cpu()
    with torch.no_grad():
        ref = F.conv3d(F.relu(md[0][1](F.conv3d(x.double().cpu(), md[0][0].weight, padding=1))), md[2].weight, padding=1)
    rms = [float((o.double().cpu() - ref).pow(2).mean().sqrt()) for o in outs]
    REPORT[f"classifier_one_pass/{shape}"] = rms
    assert rms[0] <= 1.1 * rms[1] + 1e-9 and rms[0] <= 2e-6 * float(ref.abs().max())


@pytest.mark.parametrize("shape", [(1, 24, 256, 256), (1, 32, 128, 128), (2, 36, 128, 160)])
def test_classifier_one_pass_form_at_the_live_shapes(sa, shape, monkeypatch):
    """The two classifiers of the 1024^2 / maxdisp 128 pair at their live shapes (`classif` on [32,24,256,256], `classif_att_` on
    [32,32,128,128]) and a 36-plane slab at batch 2 (the 2048^2 pair's depth): one pass against two launches, every output."""
    from oracle import detdata as dd
    B, D, H, W = shape
    m = _det_classifier(sa, 940)
    x = torch.relu(dev(dd.t_normalish((B, 32, D, H, W), 941)))
    outs = []
    for flag in (True, False):
        monkeypatch.setattr(sa.engine, "CLASSIFIER_FUSED", flag)
        with torch.no_grad():
            outs.append(m(x))
    scale = float(outs[1].abs().max())
    err = float((outs[0] - outs[1]).abs().max())
    REPORT[f"classifier_one_pass_live/{shape}"] = err / scale
    assert err <= 4e-6 * scale


def test_classifier_one_pass_form_is_batch_invariant_and_decided_by_the_layer(sa, monkeypatch):
    """A pair gets the same bits alone and in a batch: the one-pass form is chosen by what ONE pair of the layer offers the chip
    (>= 512 tiles of 2 x 8 x 32), never by the batch; layers below that keep the two-launch form at every batch size."""
    from oracle import detdata as dd
    m = _det_classifier(sa, 930)
    x = dev(dd.t_normalish((3, 32, 12, 134, 200), 931))
    with torch.no_grad():
        whole = m(x)
        for i in range(3):
            assert torch.equal(m(x[i:i + 1].contiguous()), whole[i:i + 1])
    small = dev(dd.t_normalish((8, 32, 8, 64, 64), 932))          # 2 x 8 x 4 = 64 tiles per pair: 512 only with the batch counted
    assert not sa.engine.classifier_fused_applies(small, 19)
    assert not sa.engine.classifier_fused_applies(x[:, :, :10].contiguous(), 19)      # depth not a multiple of 4
    hw = sa.engine.pack_classifier_head_weight(m[2].weight)
    ws0 = sa.engine.pack_conv_weight_bf16s(m[0][0].weight, 19)
    sc, sh = sa.engine.fold_bn(m[0][1])
    with pytest.raises(sa._lib.SemStereoHipError):                 # the C ABI refuses what the rule refuses (no silent other path)
        sa.engine.classifier_fused_hip(small, ws0, sc, sh, 19, hw)


@pytest.mark.parametrize("nterms", [6, 19])
@pytest.mark.parametrize("case", [(64, 128, 4, 7, 40), (32, 64, 6, 10, 34), (20, 40, 3, 5, 9), (64, 128, 16, 64, 64),
                                  # >= 256 workgroups: the form whose waves split the 64 channels of a workgroup (ragged channel groups, odd sizes)
                                  (20, 72, 12, 100, 200), (33, 64, 13, 95, 129)])
def test_conv3d_split_bf16_stride2(sa, case, nterms):
    """the stride-2 instantiation of the split-bf16 conv (odd sizes, ragged channels) against float64 and the exact-fp32 kernel"""
    import torch.nn.functional as F
    from oracle import detdata as dd
    Cin, Cout, D, H, W = case
    x = dd.t_normalish((1, Cin, D, H, W), 481)
    w = dd.t_uniform((Cout, Cin, 3, 3, 3), 482, -1, 1) * (3.0 / (Cin * 27)) ** 0.5
    scale, shift = dd.t_uniform((Cout,), 483, 0.5, 1.5), dd.t_uniform((Cout,), 484, -0.2, 0.2)
    ref = F.relu(F.conv3d(x.double(), w.double(), None, 2, 1) * scale.double().reshape(1, -1, 1, 1, 1) + shift.double().reshape(1, -1, 1, 1, 1))
    y = sa.modules.conv3d_bf16s_hip(dev(x), sa.modules.pack_conv_weight_bf16s(dev(w), nterms), Cout, dev(scale), dev(shift), True, nterms, stride=2)
    y32 = sa.modules.conv3d_hip(dev(x), sa.modules.pack_conv_weight(dev(w)), dev(scale), dev(shift), 3, 2, True)
    assert y.shape == ref.shape
    e_split, e_f32 = float((y.double().cpu() - ref).abs().max()), float((y32.double().cpu() - ref).abs().max())
    REPORT[f"conv3d_s2_{_eng(nterms)}/{case}"] = e_split
    assert e_split <= 1.5 * e_f32 + 1e-6, (e_split, e_f32)


@pytest.mark.parametrize("nterms", [6, 3, 19])
@pytest.mark.parametrize("case", [(2, 128, 64, 64, 64, True), (1, 64, 32, 33, 70, False), (1, 20, 40, 5, 9, True), (2, 128, 64, 256, 256, True)])
def test_conv2d_split_bf16(sa, case, nterms):
    """Conv2d(3x3, s1, p1) + affine + ReLU (concat_feature, models/SemStereo.py:222-226) on the split-bf16 engine vs float64"""
    import torch.nn.functional as F
    from oracle import detdata as dd
    B, Cin, Cout, H, W, relu = case
    x = dd.t_normalish((B, Cin, H, W), 581)
    w = dd.t_uniform((Cout, Cin, 3, 3), 582, -1, 1) * (3.0 / (Cin * 9)) ** 0.5
    scale, shift = dd.t_uniform((Cout,), 583, 0.5, 1.5), dd.t_uniform((Cout,), 584, -0.2, 0.2)
    ref = F.conv2d(x.double(), w.double(), None, 1, 1) * scale.double().reshape(1, -1, 1, 1) + shift.double().reshape(1, -1, 1, 1)
    if relu:
        ref = F.relu(ref)
    y = sa.modules.conv2d_bf16s_hip(dev(x), sa.modules.pack_conv2d_weight_bf16s(dev(w), nterms), Cout, dev(scale), dev(shift), relu, nterms)
    yt = F.conv2d(dev(x), dev(w), None, 1, 1) * dev(scale).reshape(1, -1, 1, 1) + dev(shift).reshape(1, -1, 1, 1)
    yt = F.relu(yt) if relu else yt
    e, e_t = float((y.double().cpu() - ref).abs().max()), float((yt.double().cpu() - ref).abs().max())
    REPORT[f"conv2d_{_eng(nterms)}/{case}"] = e
    REPORT[f"conv2d_torch_fp32_vs_f64/{case}"] = e_t
    # fp32 accumulation over K = 9 * Cin <= 1152 products of O(1) values; MIOpen's Winograd form (e_t) adds fewer terms
    assert e <= (1e-5 if nterms != 3 else 4e-5), (e, e_t)


@pytest.mark.parametrize("shape", [(1, 128, 64, 64, 96), (2, 64, 32, 9, 37), (1, 128, 64, 256, 256)])
def test_conv2d_on_both_views_in_one_launch(sa, shape):
    """ss_conv2d_bf16s_pair_fwd (concat_feature on the left and the right view, models/SemStereo.py:314-315): the launch that reads
    its batch from two tensors equals the two single-view launches -- element for element where the batch does not change the
    tile, to 2e-6 where it does (the block-floating scale is per tile) -- and is as close to float64."""
    if sa.modules.CONV_ENGINE == "f32" or not sa.engine._conv2d_hip_on():
        pytest.skip("concat_feature's 2-D layers run on the HIP kernel under the f16x3 engine (SS_CONV2D_HIP=1 forces it elsewhere)")
    import torch.nn.functional as F
    import torch.nn as nn
    from oracle import detdata as dd
    B, Cin, Cout, H, W = shape
    xa, xb = dd.t_normalish((B, Cin, H, W), 591), dd.t_normalish((B, Cin, H, W), 592) * 2.0
    conv = nn.Conv2d(Cin, Cout, 3, 1, 1, bias=False).cuda().eval()
    bn = nn.BatchNorm2d(Cout).cuda().eval()
    with torch.no_grad():
        conv.weight.copy_(dev(dd.t_uniform((Cout, Cin, 3, 3), 593, -1, 1) * (3.0 / (Cin * 9)) ** 0.5))
        bn.weight.copy_(dev(dd.t_uniform((Cout,), 594, 0.6, 1.4))); bn.bias.copy_(dev(dd.t_uniform((Cout,), 595, -0.1, 0.1)))
        bn.running_var.copy_(dev(dd.t_uniform((Cout,), 596, 0.6, 1.4)))
        y = sa.engine.run_conv2d_pair(conv, "t", conv, bn, dev(xa), dev(xb), True)
        ya = sa.engine.run_conv2d(conv, "t", conv, bn, dev(xa), True)
        yb = sa.engine.run_conv2d(conv, "t", conv, bn, dev(xb), True)
    assert y is not None and y.shape == (2 * B, Cout, H, W)
    assert float((y[:B] - ya).abs().max()) <= 2e-6 and float((y[B:] - yb).abs().max()) <= 4e-6
    sc, sh = sa.modules.fold_bn(bn)
    ref = F.relu(F.conv2d(torch.cat((xa, xb)).double(), conv.weight.detach().cpu().double(), None, 1, 1) * sc.cpu().double().reshape(1, -1, 1, 1)
                 + sh.cpu().double().reshape(1, -1, 1, 1))
    assert float((y.double().cpu() - ref).abs().max()) <= 1e-5


BF16S_CASES = [
    # (Cin, Cout, D, H, W, relu, residual)
    (32, 32, 5, 9, 37, True, False),
    (64, 32, 3, 17, 66, True, False),
    (64, 64, 3, 8, 33, True, True),
    (128, 128, 2, 5, 8, False, False),
    (6, 40, 3, 4, 9, False, False),          # ragged channel block, Cout not a multiple of 32
    (20, 8, 2, 3, 70, True, False),
]


def _eng(nterms):
    return {6: "bf16x6", 3: "bf16x3", 19: "f16x3"}[nterms]


@pytest.mark.parametrize("nterms", [6, 3, 19])
@pytest.mark.parametrize("case", BF16S_CASES)
def test_conv3d_split_bf16_engine(sa, case, nterms):
    """fp32 conv emulated with 3-term bf16 operands (or two block-floating fp16 terms: nterms 19) on the 16-bit matrix
    core: the 6-product bf16 form and the fp16 form must be as close to the float64 result as the exact-fp32 MFMA kernel
    is, the 3-product bf16 form within 4e-5."""
    import torch.nn.functional as F
    from oracle import detdata as dd
    Cin, Cout, D, H, W, relu, use_res = case
    x = dd.t_normalish((2, Cin, D, H, W), 181)
    w = dd.t_uniform((Cout, Cin, 3, 3, 3), 182, -1, 1) * (3.0 / (Cin * 27)) ** 0.5
    scale, shift = dd.t_uniform((Cout,), 183, 0.5, 1.5), dd.t_uniform((Cout,), 184, -0.2, 0.2)
    ref = F.conv3d(x.double(), w.double(), None, 1, 1) * scale.double().reshape(1, -1, 1, 1, 1) + shift.double().reshape(1, -1, 1, 1, 1)
    res = dd.t_normalish(tuple(ref.shape), 185) if use_res else None
    if use_res:
        ref = ref + res.double()
    if relu:
        ref = F.relu(ref)
    ws = sa.modules.pack_conv_weight_bf16s(dev(w), nterms)
    y = sa.modules.conv3d_bf16s_hip(dev(x), ws, Cout, dev(scale), dev(shift), relu, nterms, None if res is None else dev(res))
    wp = sa.modules.pack_conv_weight(dev(w))
    y32 = sa.modules.conv3d_hip(dev(x), wp, dev(scale), dev(shift), 3, 1, relu, None if res is None else dev(res))
    e_split = float((y.double().cpu() - ref).abs().max())
    e_f32 = float((y32.double().cpu() - ref).abs().max())
    REPORT[f"conv3d_{_eng(nterms)}/{case}"] = e_split
    REPORT[f"conv3d_f32mfma_vs_f64/{case}"] = e_f32
    if nterms != 3:
        assert e_split <= 1.5 * e_f32 + 1e-7, (e_split, e_f32)
    else:       # 3 products drop terms of 2^-16 relative size: ~1e-5 absolute on O(1) outputs at small K
        assert e_split <= 4e-5, (e_split, e_f32)


@pytest.mark.parametrize("engine", ["f32", "bf16x6", "bf16x3", "f16x3"])
def test_hot_segment_on_each_conv_engine(sa, golden, engine):
    name = "s128"
    old = sa.modules.CONV_ENGINE
    sa.engine.CONV_ENGINE = engine
    try:
        seg, P = _segment(sa, cases.SEGMENT[name][3])
        fl4, fr4, fl8, fr8, maxdisp = cases.segment_inputs(name)
        with torch.no_grad():
            r = seg(dev(fl4), dev(fr4), dev(fl8), dev(fr8))
    finally:
        sa.engine.CONV_ENGINE = old
    g = golden["segment"]
    same = (r["samples"].cpu().numpy().astype(np.int16) == g[f"{name}/samples"]).mean()
    REPORT[f"segment_{engine}/samples_equal_fraction"] = float(same)
    assert same == 1.0
    check(f"segment_{engine}/pred_att", r["pred_att"], g[f"{name}/pred_att"], 1e-3)
    if engine == "bf16x3":
        # the opt-in 3-product form carries ~1e-5 relative conv error: regression_topk's hard top-2 choice
        # (models/submodule.py:436-437) may flip on an isolated pixel; everything else must still agree
        err = (r["pred"].cpu() - torch.as_tensor(g[f"{name}/pred"])).abs()
        REPORT[f"segment_{engine}/pred_fraction_within_1e-3"] = float((err <= 1e-3).float().mean())
        assert (err <= 1e-3).float().mean() >= 0.995 and float(err.median()) <= 1e-4
    else:
        err = (r["pred"].cpu() - torch.as_tensor(g[f"{name}/pred"])).abs()
        REPORT[f"segment_{engine}/pred"] = float(err.max())
        assert float(err.median()) <= 1e-5 and int((err > 1e-3).sum()) <= 1, float(err.max())      # see the fixture test


_NON_DEFAULT = {
    # name: (object path, attribute, value) -- every switch of DESIGN.md section 5 whose non-default side is a different code path
    "SS_DEFER=0": ("deferred", "ENABLED", False),
    "SS_OVERLAP=0": ("segment.HotSegment", "OVERLAP", False),
    "SS_OVERLAP=1": ("segment.HotSegment", "OVERLAP", True),
    "SS_FUSED=0": ("segment.HotSegment", "FUSED", False),
    "SS_PRELUDE_AT=start": ("segment.HotSegment", "PRELUDE_AT", "start"),
    "SS_PRELUDE_AT=u5": ("segment.HotSegment", "PRELUDE_AT", "u5"),
    "SS_PRELUDE_AT=c4": ("segment.HotSegment", "PRELUDE_AT", "c4"),
    "SS_PRELUDE_AT=c2,cls,st": ("segment.HotSegment", "PRELUDE_AT", "c2,cls,st"),
    "SS_GWC_PATCH_FUSED=0": ("segment.HotSegment", "GWC_PATCH_FUSED", False),
    "SS_STEM_HALVES=0": ("segment.HotSegment", "STEM_BY_HALVES", False),
    "SS_STEM_LEFT_FUSED=0": ("engine", "STEM_LEFT_FUSED", False),
    "SS_STEM_PRESPLIT=1": ("engine", "STEM_PRESPLIT", True),      # (with the gathered stem off: it has precedence)
    "SS_STEM_GATHER=0": ("engine", "STEM_GATHER", False),
    "SS_PAIR_VIEWS=0": ("segment.HotSegment", "PAIR_VIEWS", False),
    "SS_ATTENTION=fused": ("engine", "ATTENTION_FORM", "fused"),
    "SS_HEAD_F16=1": ("engine", "HEAD_F16", True),
    "SS_DECONV_F16=0": ("engine", "DECONV_F16", False),
    "SS_DECONV_MIN_WGS=256": ("engine", "DECONV_MIN_WORKGROUPS", 256),
    "SS_CLASSIFIER_CL=0": ("engine", "CLASSIFIER_CL", False),
    "SS_CLASSIFIER_FUSED=0": ("engine", "CLASSIFIER_FUSED", False),
    "SS_CONV2D_HIP=0": ("engine", "CONV2D_HIP", False),
}


@pytest.mark.parametrize("setting", sorted(_NON_DEFAULT))
def test_hot_segment_under_every_non_default_switch(sa, golden, setting, monkeypatch):
    """the driver only ever runs the defaults, so the other side of every switch gets its own run of the hot
    segment here, against the reference's fixture: identical candidates, pred_att within 1e-3 px, at most an isolated top-2 flip
    in pred (the criterion of test_hot_segment_on_each_conv_engine)."""
    path, attr, value = _NON_DEFAULT[setting]
    obj = sa
    for part in path.split("."):
        obj = getattr(obj, part)
    monkeypatch.setattr(obj, attr, value)
    if setting == "SS_STEM_PRESPLIT=1":
        monkeypatch.setattr(sa.engine, "STEM_GATHER", False)
    name = "s128"
    seg, P = _segment(sa, cases.SEGMENT[name][3])
    fl4, fr4, fl8, fr8, maxdisp = cases.segment_inputs(name)
    before = dict(sa.modules.PATH_COUNTS)
    with torch.no_grad():
        r = seg(dev(fl4), dev(fr4), dev(fl8), dev(fr8))
    r = {k: sa.deferred.real(v) for k, v in r.items()}
    # (SS_CONV2D_HIP=0 hands concat_feature to MIOpen by design -- counted; nothing else may leave the HIP path)
    if setting != "SS_CONV2D_HIP=0":
        assert sa.modules.PATH_COUNTS["torch"] == before["torch"], "a PyTorch fallback ran"
    g = golden["segment"]
    assert (r["samples"].cpu().numpy().astype(np.int16) == g[f"{name}/samples"]).all(), setting
    check(f"switch/{setting}/pred_att", r["pred_att"], g[f"{name}/pred_att"], 1e-3)
    err = (r["pred"].cpu() - torch.as_tensor(g[f"{name}/pred"])).abs()
    REPORT[f"switch/{setting}/pred"] = float(err.max())
    assert float(err.median()) <= 1e-5 and int((err > 1e-3).sum()) <= 1, (setting, float(err.max()))


@pytest.mark.parametrize("lanes", [2, 4])
def test_pair_pipeline_is_bit_identical_to_sequential_calls(sa, lanes):
    """semstereo_amd.PairPipeline (r04): consecutive pairs issued round-robin on several HIP streams -- the throughput form
    bench.py times -- must give every pair, bit for bit, what a plain call on one stream gives it: 7 different pairs (more than the
    lanes, so every lane is reused while its previous pair's buffers are still alive), pred / pred_att / samples / att_topk."""
    from oracle import detdata as dd
    seg, _ = _segment(sa, 64)
    pairs = []
    for i in range(7):
        fl8, fr8 = dd.stereo_features(1, 256, 16, 24, 900 + 2 * i, max_shift=3)
        fl4, fr4 = dd.stereo_features(1, 128, 32, 48, 901 + 2 * i, max_shift=6)
        pairs.append([dev(t) for t in (fl4, fr4, fl8, fr8)])
    with torch.no_grad():
        want = [{k: v.clone() for k, v in seg(*p).items()} for p in pairs]
    torch.cuda.synchronize()
    pipe = sa.PairPipeline(seg, lanes)
    for rep in range(3):                      # (several sweeps: lane reuse, allocator reuse across streams)
        got = [pipe(*p) for p in pairs]
        pipe.synchronize()
        for i, (g_, w_) in enumerate(zip(got, want)):
            for k in ("pred", "pred_att", "samples", "att_topk"):
                assert torch.equal(g_[k], w_[k]), (rep, i, k, float((g_[k] - w_[k]).abs().max()))
    assert pipe.last_event is not None and pipe.last_event.query()


def test_pair_pipeline_survives_a_weight_update_and_a_new_shape(sa):
    """a per-module cache entry rebuilt WHILE the lanes are in use -- an in-place weight update, then a
    shape whose entries had not been built -- is packed on one lane only.  The pipeline must notice (engine.cache_generation),
    drain its lanes and keep the replaced tensors alive for the pairs in flight: every pair still gets, bit for bit, what a
    plain call with the weights of that moment gives.  Also: the module's OVERLAP attribute is never written (the choice is
    passed down per thread), and join() hands the outputs to another stream."""
    from oracle import detdata as dd
    seg, _ = _segment(sa, 64)

    def pair(i, h8=16, w8=24):
        fl8, fr8 = dd.stereo_features(1, 256, h8, w8, 700 + 2 * i, max_shift=3)
        fl4, fr4 = dd.stereo_features(1, 128, 2 * h8, 2 * w8, 701 + 2 * i, max_shift=6)
        return [dev(t) for t in (fl4, fr4, fl8, fr8)]
    pairs = [pair(i) for i in range(6)]
    pipe = sa.PairPipeline(seg, 3)
    first = [pipe(*p) for p in pairs[:3]]
    assert "OVERLAP" not in seg.__dict__
    with torch.no_grad():                                       # pairs 0-2 may still be in flight on the lanes
        seg.classif[0][0].weight.mul_(2.0)             # (powers of two: undone exactly below)
        seg.hourglass.conv1[0][1].running_var.mul_(0.5)
    gen = sa.engine.cache_generation()
    second = [pipe(*p) for p in pairs[3:]]
    assert sa.engine.cache_generation() > gen and pipe.rebuilds >= 1
    other = pair(9, 12, 20)                                     # another shape: its entries are built inside a lane, too
    third = pipe(*other)
    side = torch.cuda.Stream()
    pipe.join(third, side)
    with torch.cuda.stream(side):
        doubled = third["pred"] * 2.0
    side.synchronize()
    pipe.synchronize()
    with torch.no_grad():
        want_second = [seg(*p) for p in pairs[3:]]
        want_third = seg(*other)
        seg.classif[0][0].weight.mul_(0.5)
        seg.hourglass.conv1[0][1].running_var.mul_(2.0)
        want_first = [seg(*p) for p in pairs[:3]]
    torch.cuda.synchronize()
    for got, want in ((first, want_first), (second, want_second), ([third], [want_third])):
        for g_, w_ in zip(got, want):
            for k in ("pred", "pred_att", "samples"):
                assert torch.equal(g_[k], w_[k]), k
    assert torch.equal(doubled, want_third["pred"] * 2.0)
    pipe.close()
    assert not sa.engine._RETIRED


@pytest.mark.parametrize("hip2d", [True, False])
def test_hot_segment_with_hip_2d_convs(sa, golden, hip2d):
    """SS_CONV2D_HIP: concat_feature's two 3x3 2-D convs on the split engine (default with f16x3) or on MIOpen."""
    name = "s128"
    old = sa.modules.CONV2D_HIP
    sa.engine.CONV2D_HIP = hip2d
    try:
        seg, P = _segment(sa, cases.SEGMENT[name][3])
        fl4, fr4, fl8, fr8, maxdisp = cases.segment_inputs(name)
        with torch.no_grad():
            r = seg(dev(fl4), dev(fr4), dev(fl8), dev(fr8))
    finally:
        sa.engine.CONV2D_HIP = old
    g = golden["segment"]
    assert (r["samples"].cpu().numpy().astype(np.int16) == g[f"{name}/samples"]).all()
    check("segment_conv2d_hip/pred_att", r["pred_att"], g[f"{name}/pred_att"], 1e-3)
    err = (r["pred"].cpu() - torch.as_tensor(g[f"{name}/pred"])).abs()
    assert float(err.median()) <= 1e-5 and int((err > 1e-3).sum()) <= 1, float(err.max())


@pytest.mark.parametrize("split", ["0", "1"])     # one workgroup for all 8 output parity classes / even and odd planes apart
@pytest.mark.parametrize("case", [(128, 64, 2, 3, 5, 64), (64, 32, 3, 9, 33, 32), (32, 32, 2, 4, 40, 0), (8, 24, 2, 3, 6, 6)])
def test_deconv3d_kernel(sa, case, split, tuning_env):
    import torch.nn.functional as F
    from oracle import detdata as dd
    tuning_env("SS_DECONV_SPLIT", split)
    Cin, Cout, D, H, W, Cs = case
    x = dd.t_normalish((2, Cin, D, H, W), 91)
    w = dd.t_uniform((Cin, Cout, 3, 3, 3), 92, -1, 1) * (3.0 / (Cin * 27 / 8)) ** 0.5
    shift = dd.t_uniform((Cout,), 93, -0.2, 0.2)
    ref = F.conv_transpose3d(x, w, None, stride=2, padding=1, output_padding=1) + shift.reshape(1, -1, 1, 1, 1)
    skip = ws = None
    if Cs:
        skip = dd.t_normalish((2, Cs, 2 * D, 2 * H, 2 * W), 94)
        ws = dd.t_uniform((Cout, Cs, 1, 1, 1), 95, -1, 1) * (3.0 / Cs) ** 0.5
        ref = ref + F.conv3d(skip, ws)
    ref = F.relu(ref)
    wp = sa.modules.pack_conv_weight(dev(w), transposed=True)
    wsp = None if ws is None else sa.modules.pack_conv_weight(dev(ws)).reshape(Cs, Cout).contiguous()
    y = sa.modules.deconv3d_hip(dev(x), wp, dev(shift), True, None if skip is None else dev(skip), wsp)
    check(f"deconv3d/{case}/split{split}", y, ref, 2e-4)


@pytest.mark.parametrize("nterms", [6, 3, 19])
@pytest.mark.parametrize("case", [(128, 64, 2, 3, 5, 64), (64, 32, 3, 9, 33, 32), (32, 32, 2, 4, 40, 0), (8, 24, 2, 3, 6, 6), (20, 40, 1, 5, 34, 10)])
def test_deconv3d_split_bf16_engine(sa, case, nterms):
    """ConvTranspose3d + 1x1x1 skip projection + shift + ReLU on the split-bf16 engine (ragged channel chunks, Cout not a
    multiple of 32, D = 1): the 6-product form as close to float64 as the exact-fp32 kernel, the 3-product form within 4e-5."""
    import torch.nn.functional as F
    from oracle import detdata as dd
    Cin, Cout, D, H, W, Cs = case
    x = dd.t_normalish((2, Cin, D, H, W), 391)
    w = dd.t_uniform((Cin, Cout, 3, 3, 3), 392, -1, 1) * (3.0 / (Cin * 27 / 8)) ** 0.5
    shift = dd.t_uniform((Cout,), 393, -0.2, 0.2)
    ref = F.conv_transpose3d(x.double(), w.double(), None, stride=2, padding=1, output_padding=1) + shift.double().reshape(1, -1, 1, 1, 1)
    skip = ws = None
    if Cs:
        skip = dd.t_normalish((2, Cs, 2 * D, 2 * H, 2 * W), 394)
        ws = dd.t_uniform((Cout, Cs, 1, 1, 1), 395, -1, 1) * (3.0 / Cs) ** 0.5
        ref = ref + F.conv3d(skip.double(), ws.double())
    ref = F.relu(ref)
    wp = sa.modules.pack_conv_weight(dev(w), transposed=True)
    wsp = None if ws is None else sa.modules.pack_conv_weight(dev(ws)).reshape(Cs, Cout).contiguous()
    y32 = sa.modules.deconv3d_hip(dev(x), wp, dev(shift), True, None if skip is None else dev(skip), wsp)
    y = sa.modules.deconv3d_bf16s_hip(dev(x), sa.modules.pack_deconv_weight_bf16s(wp, nterms), Cout, dev(shift), True, nterms,
                                      None if skip is None else dev(skip),
                                      None if wsp is None else sa.modules.pack_deconv_weight_bf16s(wsp))
    e_split, e_f32 = float((y.double().cpu() - ref).abs().max()), float((y32.double().cpu() - ref).abs().max())
    REPORT[f"deconv3d_{_eng(nterms)}/{case}"] = e_split
    REPORT[f"deconv3d_f32_vs_f64/{case}"] = e_f32
    assert e_split <= (1.5 * e_f32 + 1e-6 if nterms != 3 else 4e-5), (e_split, e_f32)


# the range cases of every kernel on the two-term fp16 form: one table, tests/f16_model.py (called with a channel index alone it is
# the 32-channel table this test has always used)
from f16_model import F16_RANGE_CASES  # noqa: E402


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("name", sorted(F16_RANGE_CASES))
def test_conv3d_f16_form_block_floating_ranges(sa, name, stride):
    """The fp16 form must not depend on the operands' magnitude: fp16 has 5 exponent bits, so weights are scaled per output
    channel and activations per staged chunk of the tile (conv3d_bf16s.hip).  Inputs far outside fp16's range, channels
    12 decades apart in either order (the accumulators are rescaled when the running maximum grows), a partial sum as the
    initial accumulator: the error against float64, relative to each output channel's rms, stays at the exact-fp32 kernel's."""
    import torch.nn.functional as F
    from oracle import detdata as dd
    in_mul, w_mul = F16_RANGE_CASES[name]
    Cin = Cout = 32
    D, H, W = 5, 12, 70
    x = F.relu(dd.t_normalish((1, Cin, D, H, W), 701)) * torch.tensor([in_mul(c) for c in range(Cin)]).reshape(1, -1, 1, 1, 1)
    w = dd.t_uniform((Cout, Cin, 3, 3, 3), 702, -1, 1) * (3.0 / (Cin * 27)) ** 0.5
    w = w * torch.tensor([w_mul(c) for c in range(Cout)]).reshape(-1, 1, 1, 1, 1)
    x, w = x.float(), w.float()
    ref = F.conv3d(x.double(), w.double(), None, stride, 1)
    one, zero = dev(torch.ones(Cout)), dev(torch.zeros(Cout))
    y = sa.modules.conv3d_bf16s_hip(dev(x), sa.modules.pack_conv_weight_bf16s(dev(w), 19), Cout, one, zero, False, 19, stride=stride)
    y32 = sa.modules.conv3d_hip(dev(x), sa.modules.pack_conv_weight(dev(w)), one, zero, 3, stride, False)
    assert bool(torch.isfinite(y).all())
    rms = ref.pow(2).mean(dim=(0, 2, 3, 4), keepdim=True).sqrt().clamp_min(1e-300)
    e = float(((y.double().cpu() - ref) / rms).abs().max())
    e32 = float(((y32.double().cpu() - ref) / rms).abs().max())
    REPORT[f"conv3d_f16x3_range/{name}/s{stride}"] = e
    assert e <= 1.5 * e32 + 1e-6, (e, e32)
    if stride == 1:      # continuing a partial sum of very different magnitude than this half's contribution
        part = (dd.t_normalish(tuple(ref.shape), 703).double() * rms * 100.0).float()
        yp = sa.modules.conv3d_bf16s_hip(dev(x), sa.modules.pack_conv_weight_bf16s(dev(w), 19), Cout, one, zero, False, 19, partial=dev(part))
        refp = ref + part.double()
        y6 = sa.modules.conv3d_bf16s_hip(dev(x), sa.modules.pack_conv_weight_bf16s(dev(w), 6), Cout, one, zero, False, 6, partial=dev(part))
        ep = float(((yp.double().cpu() - refp) / (100.0 * rms)).abs().max())
        ep6 = float(((y6.double().cpu() - refp) / (100.0 * rms)).abs().max())
        # the accumulator holds the (100x larger) partial sum through ~160 fp32 accumulations: their rounding, in either form
        assert ep <= 2.0 * ep6 + 1e-6 and ep <= 2e-5, (ep, ep6)


@pytest.mark.parametrize("in_mul", [1e-6, 1.0, 1e6])
def test_deconv3d_f16_form_block_floating_ranges(sa, in_mul, tuning_env):
    """the transposed conv's fp16 main loop beside its bf16 skip projection of O(1) values, the two 12 decades apart: under the
    form this small layer gets (two class groups + chunk-blocked accumulation, the skip projection after the main loop) and under
    the form of the large layers (SS_DECONV_GROUPS=0: all 8 classes per workgroup, the skip projection FIRST in every other one)"""
    import torch.nn.functional as F
    from oracle import detdata as dd
    Cin, Cout, D, H, W, Cs = 48, 40, 3, 9, 35, 16
    x = (F.relu(dd.t_normalish((1, Cin, D, H, W), 711)) * in_mul).float()
    w = dd.t_uniform((Cin, Cout, 3, 3, 3), 712, -1, 1) * (3.0 / (Cin * 27 / 8)) ** 0.5
    skip = dd.t_normalish((1, Cs, 2 * D, 2 * H, 2 * W), 713)
    ws = dd.t_uniform((Cout, Cs, 1, 1, 1), 714, -1, 1) * (3.0 / Cs) ** 0.5
    ref = F.conv_transpose3d(x.double(), w.double(), None, stride=2, padding=1, output_padding=1) + F.conv3d(skip.double(), ws.double())
    wp = sa.modules.pack_conv_weight(dev(w), transposed=True)
    wsp = sa.modules.pack_conv_weight(dev(ws)).reshape(Cs, Cout).contiguous()
    zero = dev(torch.zeros(Cout))
    y32 = sa.modules.deconv3d_hip(dev(x), wp, zero, False, dev(skip), wsp)
    rms = float(ref.pow(2).mean().sqrt())
    e32 = float((y32.double().cpu() - ref).abs().max()) / rms
    for groups in (None, 0, 2):             # None: no switch, what the launcher picks (groups 2 at this size)
        if groups is not None:
            tuning_env("SS_DECONV_GROUPS", str(groups))
        y = sa.modules.deconv3d_bf16s_hip(dev(x), sa.modules.pack_deconv_weight_bf16s(wp, 19), Cout, zero, False, 19, dev(skip),
                                          sa.modules.pack_deconv_weight_bf16s(wsp))
        e = float((y.double().cpu() - ref).abs().max()) / rms
        REPORT[f"deconv3d_f16x3_range/{in_mul}" + ("" if groups is None else f"/groups{groups}")] = e
        assert e <= 1.5 * e32 + 1e-6, (groups, e, e32)


def test_patch_and_gate_fusion(sa):
    from oracle import detdata as dd
    P = oseg.deterministic_params()
    cv = dd.t_normalish((2, 32, 4, 7, 13), 101)
    gate = dd.t_normalish((2, 32, 7, 13), 102)
    mod = sa.modules.DepthwisePatch(32)
    mod.load_state_dict({"weight": P["patch.weight"]})
    mod = mod.cuda().eval()
    ref = ostack.patch_conv(P, cv)
    with torch.no_grad():
        check("patch", mod(dev(cv)), ref, 2e-6)
        check("patch_gate", mod(dev(cv), dev(gate)), torch.sigmoid(gate).unsqueeze(2) * ref, 2e-6)


# --------------------------------------------------------------------------------------
# hot segment: features -> pred, against the REFERENCE's fixture and against the oracle
# --------------------------------------------------------------------------------------

# The graph has two HARD picks: the 24 largest of D4 attention probabilities (models/SemStereo.py:299-303) and the 2 largest
# of 24 matching costs (models/submodule.py:436-437).  Where the reference's own margin at a pick is below the rounding
# error of an fp32 evaluation, ANY implementation (a different summation order, another BLAS, the reference on another
# machine) may pick differently, and the output then moves by whole candidates.  The fixtures therefore store the
# reference's margins per pixel (gap24_rel, gap2: tests/golden/make_golden.py:decision_gaps) and the tests assert that
# EVERY deviation is explained by a margin below DELTA; everything else must meet the 1e-3 px target of BASELINE.json,
# with no percentage allowance.  DELTA2 = 1e-4: ~10x the error the HIP path shows on the costs (<= 1e-5, per-module bounds
# above) and ~1e-3 of the typical margin; DELTA24_REL = 1e-5 on the probabilities (every differing pick measured so far sat
# at a margin of <= 1.2e-7 = one ulp; the full-size fixtures list the pixels below 1e-4).
DELTA24_REL = cases.DELTA24_REL      # ONE definition (tests/golden/cases.py) for every hot-segment test
DELTA2 = cases.DELTA2
RF_RADIUS = 36      # quarter-resolution pixels a changed candidate set can reach through concat_stem + hourglass2 (two
                    # stride-2 stages, 4x4 attention windows at 1/16 of the quarter resolution) + classif


def _dilate(mask, r):
    """[B,H,W] bool -> every pixel within Chebyshev distance r of a set pixel."""
    import torch.nn.functional as F
    if not bool(mask.any()):
        return mask
    return F.max_pool2d(mask.float().unsqueeze(1), 2 * r + 1, stride=1, padding=r).squeeze(1) > 0


def _explained_deviation_check(name, r, g, prefix):
    """Assert the explained-flip criterion for one run `r` of the hot segment against fixture arrays g[prefix + ...]
    (full maps).  Returns the statistics it put into REPORT."""
    samples_ref = torch.as_tensor(g[f"{prefix}/samples"].astype(np.int64))
    gap24 = torch.as_tensor(g[f"{prefix}/gap24_rel"])
    gap2 = torch.as_tensor(g[f"{prefix}/gap2"])
    set_differs = (r["samples"].cpu().long() != samples_ref).any(dim=1)                        # [B,H,W]
    err_att = (r["pred_att"].cpu() - torch.as_tensor(g[f"{prefix}/pred_att"])).abs()
    err = (r["pred"].cpu() - torch.as_tensor(g[f"{prefix}/pred"])).abs().squeeze(1)
    REPORT[f"segment/{name}/pixels_with_other_candidates"] = int(set_differs.sum())
    REPORT[f"segment/{name}/largest_gap24_rel_among_them"] = float(gap24[set_differs].max()) if bool(set_differs.any()) else 0.0
    REPORT[f"segment/{name}/epe_vs_ref"] = float(err.mean())
    REPORT[f"segment/{name}/pred_pixels_beyond_1e-3"] = int((err > 1e-3).sum())
    # (i) a candidate set may differ only where the reference's 24th / 25th probabilities are within DELTA24_REL
    bad = set_differs & (gap24 >= DELTA24_REL)
    assert not bool(bad.any()), (f"{int(bad.sum())} pixel(s) select other candidates although the reference's margin is "
                                 f"{float(gap24[bad].min()):.2e} .. {float(gap24[bad].max()):.2e} >= {DELTA24_REL}")
    # pred_att (the soft-argmax over the 24 selected) is continuous except through that pick
    bad = (err_att > 1e-3) & ~set_differs
    assert not bool(bad.any()), f"pred_att off by up to {float(err_att[bad].max()):.2e} px on {int(bad.sum())} pixel(s) with identical candidates"
    # (ii) pred may be off by more than 1e-3 px only where the reference's 2nd / 3rd costs are within DELTA2, or inside
    # the receptive field of a pixel whose candidate set differs
    near = _dilate(set_differs, RF_RADIUS)
    tie = gap2 < DELTA2
    bad = (err > 1e-3) & ~tie & ~near
    assert not bool(bad.any()), (f"pred off by up to {float(err[bad].max()):.2e} px on {int(bad.sum())} pixel(s) with identical "
                                 f"candidates around and a reference top-2 margin of >= {float(gap2[bad].min()):.2e}")
    REPORT[f"segment/{name}/pred_beyond_1e-3_at_top2_ties"] = int(((err > 1e-3) & tie).sum())
    REPORT[f"segment/{name}/pred_beyond_1e-3_near_other_candidates"] = int(((err > 1e-3) & ~tie & near).sum())
    ok = ~tie & ~near
    if bool(ok.any()):
        REPORT[f"segment/{name}/max_err_where_no_excuse"] = float(err[ok].max())
    return set_differs, err


def _segment_case(sa, golden, name):
    maxdisp = cases.segment_shape(name)[3]
    seg = sa.HotSegment(maxdisp)
    P = cases.segment_params(name, golden["segment"])
    res = seg.load_state_dict(P, strict=False)
    assert not res.unexpected_keys and all(k.endswith("num_batches_tracked") for k in res.missing_keys)
    return seg.cuda().eval(), P


@pytest.mark.parametrize("name", sorted(cases.SEGMENT) + sorted(cases.SEGMENT_CAL))
def test_hot_segment_vs_reference_fixture(sa, golden, name):
    if sa.modules.CONV_ENGINE == "bf16x3" and name not in ("s128", "s96x160_b2"):
        pytest.skip("SS_CONV_ENGINE=bf16x3: the 3-product form's ~1e-5 conv error is beyond the margins assumed here")
    seg, P = _segment_case(sa, golden, name)
    fl4, fr4, fl8, fr8, maxdisp = cases.segment_inputs(name)
    before = dict(sa.modules.PATH_COUNTS)
    with torch.no_grad():
        r = seg(dev(fl4), dev(fr4), dev(fl8), dev(fr8))
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"]
    g = golden["segment"]
    check(f"segment/{name}/pred_att0", r["pred_att0"], g[f"{name}/pred_att0"], 1e-3)
    set_differs, err = _explained_deviation_check(name, r, g, name)
    assert float(err.median()) <= 1e-5
    if name in ("s128", "s96x160_b2"):
        # the two small fixtures have been bit-stable on every build so far: keep them as strict canaries
        assert not bool(set_differs.any())
        check(f"segment/{name}/pred_att", r["pred_att"], g[f"{name}/pred_att"], 1e-3)


@pytest.mark.parametrize("name", sorted(cases.SEGMENT) + sorted(cases.SEGMENT_CAL))
def test_matching_branch_on_the_reference_candidates(sa, golden, name):
    """models/SemStereo.py:314-323 fed the REFERENCE's 24 candidates and attention weights (fixture): no top-24 difference
    can exist upstream, so every pixel must be within 1e-3 px of the reference's `pred` unless the reference's own 2nd / 3rd
    largest costs are within DELTA2 -- no receptive-field excuse, no percentage."""
    if sa.modules.CONV_ENGINE == "bf16x3" and name not in ("s128", "s96x160_b2"):
        pytest.skip("SS_CONV_ENGINE=bf16x3: beyond the margins assumed here")
    seg, P = _segment_case(sa, golden, name)
    fl4, fr4, _, _, maxdisp = cases.segment_inputs(name)
    g = golden["segment"]
    samples = torch.as_tensor(g[f"{name}/samples"].astype(np.float32))
    att = torch.as_tensor(g[f"{name}/att_topk"]).unsqueeze(1)
    with torch.no_grad():
        pred = seg.matching_branch(dev(fl4), dev(fr4), dev(att), dev(samples))
    err = (pred.cpu() - torch.as_tensor(g[f"{name}/pred"])).abs().squeeze(1)
    gap2 = torch.as_tensor(g[f"{name}/gap2"])
    tie = gap2 < DELTA2
    REPORT[f"matching/{name}/epe_vs_ref"] = float(err.mean())
    REPORT[f"matching/{name}/max_err_off_ties"] = float(err[~tie].max())
    REPORT[f"matching/{name}/pixels_beyond_1e-3_at_ties"] = int(((err > 1e-3) & tie).sum())
    REPORT[f"matching/{name}/smallest_flipped_gap2"] = float(gap2[err > 1e-3].max()) if bool((err > 1e-3).any()) else 0.0
    bad = (err > 1e-3) & ~tie
    assert not bool(bad.any()), (f"{int(bad.sum())} pixel(s) off by up to {float(err[bad].max()):.2e} px although the "
                                 f"reference's top-2 margin there is >= {float(gap2[bad].min()):.2e}")
    assert float(err[~tie].max()) <= 1e-3 and float(err.median()) <= 1e-5


@pytest.mark.parametrize("name", sorted(cases.SEGMENT) + sorted(cases.SEGMENT_CAL))
def test_hot_segment_strict_on_the_reference_picks(sa, golden, name):
    """The whole segment with NO receptive-field excuse (tests/strict.py): HIP attention branch; wherever it
    selected other candidates -- allowed only at a reference margin below DELTA24_REL -- the reference's own candidates and
    weights are put back; HIP matching branch; every pixel of `pred` within 1e-3 px of the reference's unless the
    reference's own 2nd / 3rd largest costs are within DELTA2 (bound: max(1e-3, 3 x the reference's own largest distance from
    the fixture's float64 truth), see tests/test_fullsize_gpu.py)."""
    if sa.modules.CONV_ENGINE == "bf16x3" and name not in ("s128", "s96x160_b2"):
        pytest.skip("SS_CONV_ENGINE=bf16x3: beyond the margins assumed here")
    import strict
    seg, P = _segment_case(sa, golden, name)
    g = golden["segment"]
    if strict.fixture_view(g, name) is None:
        pytest.skip(f"{name}: no round-3 fixture")
    before = dict(sa.modules.PATH_COUNTS)
    rep, v, pred, differs, unexplained = strict.run_strict(seg, g, name)
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"]
    for k_, val in rep.items():
        REPORT[f"strict/{name}/{k_}"] = val
    ref_self = rep["reference_vs_truth_max_off_ties_px"]
    bound = max(1e-3, 3.0 * ref_self)
    assert not bool(unexplained.any()), f"{int(unexplained.sum())} pixel(s) select other candidates at a reference margin >= {DELTA24_REL}"
    assert bound <= 3e-3 and rep["max_err_off_ties_px"] <= bound, rep
    assert rep["median_abs_err_px"] <= 1e-4 and rep["epe_vs_reference_off_ties_px"] <= 1e-4, rep
    assert rep["hip_vs_truth_max_off_ties_px"] <= max(1e-3, 2.0 * ref_self), rep


def test_matching_branch_as_close_to_float64_truth_as_the_fp32_oracle(sa):
    """The property bench.py reports at full size.  `pred` is discontinuous in the costs (hard top-2 pick,
    models/submodule.py:436-437), so against the float64 evaluation of the same graph ("truth") any fp32
    path is off by whole candidates wherever the 2nd/3rd largest costs sit within rounding error.  With
    every path fed the truth's 24 candidates: the HIP path's cost error is no larger than 2x the fp32 CPU
    oracle's, and where the truth's top-2/top-3 gap exceeds 1e-4 the EPE is <= 1e-4 px (max <= 1e-3 px)."""
    if sa.modules.CONV_ENGINE == "bf16x3":
        pytest.skip("SS_CONV_ENGINE=bf16x3: this bound is for the fp32-accurate engines")
    from oracle import detdata as dd
    H, maxdisp = 512, 128
    seg, P = _segment(sa, maxdisp)
    ins = [dd.t_normalish((1, 128, H // 4, H // 4), 201), dd.t_normalish((1, 128, H // 4, H // 4), 202),
           dd.t_normalish((1, 256, H // 8, H // 8), 203), dd.t_normalish((1, 256, H // 8, H // 8), 204)]
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}
    tru = oseg.hot_segment(P64, *[t.double() for t in ins], maxdisp, keep=True)
    att32, smp = tru["att_topk"].float(), tru["samples"].float()
    keep32, cap = {}, {}
    with torch.no_grad():
        p32 = oseg.matching_branch(P, ins[0], ins[1], att32, smp, keep32)
        hk = seg.classif.register_forward_hook(lambda m, a, o: cap.__setitem__("cost", o.detach()))
        ph = seg.matching_branch(dev(ins[0]), dev(ins[1]), dev(att32), dev(smp))
        hk.remove()
    cost64 = tru["cost"].squeeze(1)
    top3 = cost64.topk(3, dim=1).values
    ok = ((top3[:, 1] - top3[:, 2]) > 1e-4).unsqueeze(1)
    rms = lambda x: float(x.double().pow(2).mean().sqrt())                                   # noqa: E731
    c_hip, c_o32 = rms(cap["cost"].cpu().squeeze(1).double() - cost64), rms(keep32["cost"].squeeze(1).double() - cost64)
    e_hip = (ph.cpu().double() - tru["pred"]).abs()
    e_o32 = (p32.double() - tru["pred"]).abs()
    REPORT["segment_f64/cost_rms_err_hip"] = c_hip
    REPORT["segment_f64/cost_rms_err_oracle32"] = c_o32
    REPORT["segment_f64/epe_hip"] = float(e_hip.mean())
    REPORT["segment_f64/epe_oracle32"] = float(e_o32.mean())
    REPORT["segment_f64/epe_hip_gap_gt_1e-4"] = float(e_hip[ok].mean())
    REPORT["segment_f64/fraction_gap_gt_1e-4"] = float(ok.double().mean())
    assert c_hip <= 2.0 * c_o32 + 1e-7
    assert float(ok.double().mean()) > 0.5
    assert float(e_hip[ok].mean()) <= 1e-4 and float(e_hip[ok].max()) <= 1e-3


def test_reference_shaped_composition_on_gpu(sa, golden):
    """The line-by-line composition the reference's forward() performs (reference-named ops:
    build_gwc_volume_norm, disparity_regression, disparity_variance, SpatialTransformer_grid,
    regression_topk + module calls), which HotSegment takes when autograd is on, reaches the same
    disparities as the fixture and back-propagates through the HIP autograd.Functions."""
    if sa.modules.CONV_ENGINE == "bf16x3":
        pytest.skip("SS_CONV_ENGINE=bf16x3: the 1e-3 bound on every pixel is for the fp32-accurate engines (this one flips a top-2 pick here)")
    name = "s128"
    seg, P = _segment(sa, cases.SEGMENT[name][3])
    fl4, fr4, fl8, fr8, maxdisp = cases.segment_inputs(name)
    ins = [dev(t).requires_grad_(True) for t in (fl4, fr4, fl8, fr8)]
    before = dict(sa.modules.PATH_COUNTS)
    r = seg(*ins)                                   # eval(), autograd on -> unfused reference-shaped path
    # (until r04 the eval-mode BatchNorm layers under autograd were PyTorch's; r05: ss_batchnorm_eval_fwd / _bwd -- no PyTorch layer)
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"] and sa.modules.PATH_COUNTS.get("hip_train", 0) > before.get("hip_train", 0)
    g = golden["segment"]
    same = (r["samples"].detach().cpu().numpy().astype(np.int16) == g[f"{name}/samples"]).mean()
    assert same == 1.0
    check("segment_unfused/pred_att", r["pred_att"], g[f"{name}/pred_att"], 1e-3)
    check("segment_unfused/pred", r["pred"], g[f"{name}/pred"], 1e-3)
    (r["pred"].sum() + r["pred_att"].sum()).backward()
    assert all(t.grad is not None and torch.isfinite(t.grad).all() for t in ins)


# --------------------------------------------------------------------------------------
# behaviour at the edges of fp32 (the two documented differences of the fp16 form from an fp32 convolution)
# --------------------------------------------------------------------------------------

@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_conv3d_f16_form_nonfinite_inputs(sa, poison):
    """INTENDED BEHAVIOUR.  The reference's fp32 Conv3d confines a NaN / inf input voxel to its 3x3x3 receptive field.  The
    two-term fp16 form scales each staged chunk by the power of two of its maximum, so a non-finite voxel makes the scale of
    the WORKGROUP TILES that stage it non-finite: every output whose receptive field holds the voxel is non-finite (as in
    the reference), outputs of the same tiles may be too (a superset), and every output of a tile that never stages the
    voxel is bit-identical to the clean run.  The exact-fp32 engine (SS_CONV_ENGINE=f32) reproduces the reference's set."""
    import torch.nn.functional as F
    from oracle import detdata as dd
    Cin = Cout = 32
    D, H, W = 6, 24, 96
    x = F.relu(dd.t_normalish((1, Cin, D, H, W), 731))
    w = dd.t_uniform((Cout, Cin, 3, 3, 3), 732, -1, 1) * (3.0 / (Cin * 27)) ** 0.5
    one, zero = dev(torch.ones(Cout)), dev(torch.zeros(Cout))
    ws = sa.modules.pack_conv_weight_bf16s(dev(w), 19)
    clean = sa.modules.conv3d_bf16s_hip(dev(x), ws, Cout, one, zero, False, 19).cpu()
    pz, py, px = 3, 10, 40
    xp = x.clone()
    xp[0, 5, pz, py, px] = poison
    y = sa.modules.conv3d_bf16s_hip(dev(xp), ws, Cout, one, zero, False, 19).cpu()
    y32 = sa.modules.conv3d_hip(dev(xp), sa.modules.pack_conv_weight(dev(w)), one, zero, 3, 1, False).cpu()
    rf = torch.zeros(D, H, W, dtype=torch.bool)
    rf[pz - 1:pz + 2, py - 1:py + 2, px - 1:px + 2] = True
    bad = ~torch.isfinite(y[0])
    assert bool(bad[:, rf].all()), "an output whose receptive field holds the non-finite voxel is finite"
    bad32 = ~torch.isfinite(y32[0])
    assert bool(bad32[:, rf].all()) and not bool(bad32[:, ~rf].any()), "the exact-fp32 engine must confine it to the receptive field"
    # tiles are at most 2 x 8 x 32 outputs with a one-voxel halo: anything further than that from the voxel never staged it
    far = torch.ones(D, H, W, dtype=torch.bool)
    far[max(pz - 3, 0):pz + 4, max(py - 9, 0):py + 10, max(px - 33, 0):px + 34] = False
    assert torch.equal(y[0][:, far], clean[0][:, far]), "a tile that never stages the voxel changed"
    REPORT[f"conv3d_f16x3_nonfinite/{poison}/outputs_nonfinite_beyond_rf"] = int(bad[:, ~rf].sum())


def test_conv3d_f16_form_tiny_inputs_flush(sa):
    """INTENDED BEHAVIOUR.  The block-floating scale of a staged chunk is clamped at 2^-111 (split_f16.h: E_MIN), so a tile
    whose inputs are ALL below ~2^-111 = 3.9e-34 contributes zero where an fp32 convolution would return values of that
    size (|y| < 1e-32): an absolute difference below 1e-32, far under any tolerance of the path.  Inputs at 1e-30 and up keep
    full relative precision (test_conv3d_f16_form_block_floating_ranges)."""
    import torch.nn.functional as F
    from oracle import detdata as dd
    Cin = Cout = 32
    D, H, W = 3, 9, 40
    x = (F.relu(dd.t_normalish((1, Cin, D, H, W), 741)).double() * 2.0 ** -118).float()
    w = dd.t_uniform((Cout, Cin, 3, 3, 3), 742, -1, 1) * (3.0 / (Cin * 27)) ** 0.5
    shift = dd.t_uniform((Cout,), 743, -0.2, 0.2)
    ref = F.conv3d(x.double(), w.double(), None, 1, 1) + shift.double().reshape(1, -1, 1, 1, 1)
    y = sa.modules.conv3d_bf16s_hip(dev(x), sa.modules.pack_conv_weight_bf16s(dev(w), 19), Cout, dev(torch.ones(Cout)), dev(shift),
                                    False, 19).cpu()
    assert bool(torch.isfinite(y).all())
    assert float((y.double() - ref).abs().max()) <= 1e-32 + 1e-7 * 0.2           # the shift's own fp32 rounding
    REPORT["conv3d_f16x3_tiny/max_abs_diff"] = float((y.double() - ref).abs().max())


def test_cabi_is_reentrant_two_threads_two_streams(sa):
    """SURVEY.md section 8(b), threading: nn.DataParallel drives the ops from one Python thread per GPU, so the launchers
    must keep no global mutable state and honour the calling thread's current stream.  Two threads, each on its own HIP
    stream, run different entry points of the C ABI concurrently (ctypes releases the GIL during the calls) for many
    iterations; every result must be bit-identical to the single-threaded one."""
    import threading
    from oracle import detdata as dd
    a, b = dev(dd.t_normalish((2, 64, 24, 128), 751)), dev(dd.t_normalish((2, 64, 24, 128), 752))
    x = dev(torch.relu(dd.t_normalish((1, 32, 6, 24, 96), 753)))
    w = dd.t_uniform((32, 32, 3, 3, 3), 754, -1, 1) * (3.0 / (32 * 27)) ** 0.5
    ws = sa.modules.pack_conv_weight_bf16s(dev(w), 19)
    one, zero = dev(torch.ones(32)), dev(torch.zeros(32))
    cost = dev(dd.t_normalish((2, 24, 48, 64), 755))
    cand = dev(dd.distinct_sorted_candidates(2, 24, 48, 64, 32, 756))
    jobs = {
        "gwc": lambda: sa.ops.build_gwc_volume_norm(a, b, 8, 8),
        "conv": lambda: sa.modules.conv3d_bf16s_hip(x, ws, 32, one, zero, True, 19),
        "topk": lambda: sa.ops.regression_topk(cost, cand, 2),
        "concat": lambda: sa.ops.build_concat_volume(a, b, 6),
    }
    want = {k: f().clone() for k, f in jobs.items()}
    torch.cuda.synchronize()
    errors = []

    def worker(order):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                for it in range(40):
                    for k in order:
                        got = jobs[k]()
                        if it % 8 == 0:
                            st.synchronize()
                            if not torch.equal(got, want[k]):
                                errors.append(f"{k} differs in iteration {it} of thread {order[0]}")
            st.synchronize()
        except Exception as e:      # noqa: BLE001
            errors.append(repr(e))
    threads = [threading.Thread(target=worker, args=(o,)) for o in (("gwc", "conv", "topk", "concat"), ("conv", "concat", "gwc", "topk"))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


# --------------------------------------------------------------------------------------
# round 2: channelAtt.im_att as one kernel; trilinear up-sampling fused into softmax + regression + variance
# --------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(256, 128, 2, 9, 21), (128, 64, 1, 16, 40), (256, 128, 1, 128, 128), (128, 64, 1, 64, 64)])
@pytest.mark.parametrize("sigmoid", [False, True])
def test_channel_att_logits_kernel(sa, shape, sigmoid):
    """channelAtt.im_att (models/SemStereo.py:89-100): 1x1 conv -> BatchNorm(eval) -> ReLU -> 1x1 conv (+bias) [-> sigmoid]
    in one launch, for both gates of the model, positions not a multiple of the 64-position tile, against the same
    layers in float64 and against the module's own PyTorch layers on the GPU (what ran before)."""
    from oracle import detdata as dd
    cin, cmid, B, H, W = shape
    mod = sa.modules.channelAtt(32, cin)
    with torch.no_grad():
        for i, (name, t) in enumerate(sorted(list(mod.named_parameters()) + list(mod.named_buffers()))):
            if name.endswith("num_batches_tracked"):
                continue
            if name.endswith("running_var") or (name.endswith(".weight") and t.dim() == 1):
                t.copy_(dd.t_uniform(tuple(t.shape), 760 + i, 0.6, 1.4))
            elif t.dim() == 1:
                t.copy_(dd.t_uniform(tuple(t.shape), 760 + i, -0.3, 0.3))
            else:
                t.copy_(dd.t_uniform(tuple(t.shape), 760 + i, -1, 1) * (3.0 / t.shape[1]) ** 0.5)
    mod = mod.eval()
    im = dd.t_normalish((B, cin, H, W), 770)
    m64 = __import__("copy").deepcopy(mod).double()
    with torch.no_grad():
        ref = m64.im_att(im.double())
        ref = torch.sigmoid(ref) if sigmoid else ref
        mg = mod.cuda()
        before = dict(sa.modules.PATH_COUNTS)
        got = mg.logits(dev(im), sigmoid=sigmoid)
        assert sa.modules.PATH_COUNTS["hip"] == before["hip"] + 1, "the HIP kernel did not run"
        torch_path = mg.im_att(dev(im))
        torch_path = torch.sigmoid(torch_path) if sigmoid else torch_path
    e, e_t = float((got.double().cpu() - ref).abs().max()), float((torch_path.double().cpu() - ref).abs().max())
    REPORT[f"channel_att/{shape}/{sigmoid}"] = e
    assert got.shape == (B, 32, H, W)
    assert e <= 2.0 * e_t + 2e-6, (e, e_t)
    # and as the gate of a volume (the reference's forward line :276 / :320)
    if not sigmoid:
        cv = dd.t_normalish((B, 32, 3, H, W), 771)
        with torch.no_grad():
            y = mg(dev(cv), dev(im))
        want = torch.sigmoid(m64.im_att(im.double())).unsqueeze(2) * cv.double()
        assert float((y.double().cpu() - want).abs().max()) <= 5e-6


@pytest.mark.parametrize("shape", [(1, 32, 8, 12), (2, 48, 5, 9), (1, 8, 1, 3), (1, 32, 32, 32)])
def test_upsample_softmax_regression_kernel(sa, shape):
    """models/SemStereo.py:279-285 in one kernel: the up-sampled logits must equal F.interpolate(trilinear) (ATen's CPU
    result, what the reference computes) to a few ulp, and disp / var the oracle's softmax -> regression -> variance."""
    import torch.nn.functional as F
    from oracle import detdata as dd
    B, m, h8, w8 = shape                     # coarse [B,1,m,h8,w8] -> fine [B,1,2m,2*h8,2*w8]
    coarse = dd.t_normalish((B, 1, m, h8, w8), 780) * 3.0
    up_ref = F.interpolate(coarse, [2 * m, 2 * h8, 2 * w8], mode="trilinear")
    prob = F.softmax(up_ref.squeeze(1), dim=1)
    disp_ref = oops.disparity_regression(prob, m)
    var_ref = oops.disparity_variance(prob, m, disp_ref.unsqueeze(1))
    assert sa.ops.upsample_softmax_regression_applies(dev(coarse), m, 2 * h8, 2 * w8)
    up, disp, var = sa.ops.upsample_softmax_regression(dev(coarse), m, 2 * h8, 2 * w8)
    check(f"upsample_softmax/{shape}/up", up, up_ref, 2e-6)
    check(f"upsample_softmax/{shape}/disp", disp, disp_ref, 2e-5)
    check(f"upsample_softmax/{shape}/var", var, var_ref, 2e-4, 1e-5)
    # identical to the two-step form on the GPU
    d2, v2, _ = sa.ops.softmax_regression(up.squeeze(1), m)
    assert float((d2 - disp).abs().max()) <= 1e-6 and float((v2 - var).abs().max()) <= 1e-4


@pytest.mark.parametrize("shape", [
    # (B, C, H, W, m, G, gate)
    (1, 256, 16, 128, 16, 32, True),      # the live split (8 channels per group), one column tile
    (2, 64, 13, 256, 16, 8, True),        # two column tiles: the seam columns; H not a multiple of the 6-row tile
    (1, 64, 7, 260, 24, 8, True),         # maxdisp 192's range; a ragged third column tile
    (1, 32, 5, 64, 8, 8, False),          # narrower than a tile; 4 channels per group; no gate
    (1, 64, 1, 128, 16, 8, True),         # a single row
    (1, 64, 26, 384, 16, 8, True),        # three column tiles (the middle one has real halo columns on both sides), several interior row tiles
])
def test_gwc_patch_gate_fused_is_bit_identical_to_the_two_kernels(sa, shape):
    """models/SemStereo.py:273-276 in one kernel (ss_gwc_patch_gate_fwd) against build_gwc_volume_norm followed by the
    gated `patch` kernel: same arithmetic in the same order, so the same bits; and against the oracle's composition."""
    import torch.nn.functional as F
    from oracle import detdata as dd
    B, C, H, W, m, G, with_gate = shape
    a, b = dd.t_normalish((B, C, H, W), 790), dd.t_normalish((B, C, H, W), 791)
    wp = dd.t_uniform((G, 1, 1, 3, 3), 792, -1, 1)
    gate = dd.t_normalish((B, G, H, W), 793) if with_gate else None
    assert sa.ops.gwc_patch_gate_applies(a, m, G)
    fused = sa.ops.gwc_patch_gate(dev(a), dev(b), m, G, dev(wp), None if gate is None else dev(gate))
    patch = sa.modules.DepthwisePatch(G).cuda().eval()
    with torch.no_grad():
        patch.weight.copy_(wp)
        two = patch(sa.ops.build_gwc_volume_norm(dev(a), dev(b), m, G), None if gate is None else dev(gate))
    assert fused.shape == two.shape == (B, G, 2 * m, H, W)
    assert torch.equal(fused, two), f"max diff {float((fused - two).abs().max()):.3e}"
    ref = F.conv3d(oops.build_gwc_volume_norm(a, b, m, G), wp, None, 1, (0, 1, 1), 1, G)
    if gate is not None:
        ref = torch.sigmoid(gate).unsqueeze(2) * ref
    check(f"gwc_patch_gate/{shape}", fused, ref, 3e-6)
    # un-normalised form
    f2 = sa.ops.gwc_patch_gate(dev(a), dev(b), m, G, dev(wp), None, normalize=False)
    with torch.no_grad():
        t2 = patch(sa.ops.build_gwc_volume(dev(a), dev(b), m, G))
    assert torch.equal(f2, t2)


def test_backward_warp_and_topk_in_hip(sa):
    """VERDICT r1 missing #2: the backward of SpatialTransformer_grid (features AND the disparity candidates, the live use at
    models/SemStereo.py:291) and of regression_topk are HIP kernels (ss_warp_sampled_bwd, ss_regression_topk_bwd), against
    autograd through the oracle's restatement of the reference's composition (grid_sample / sort + gather + softmax)."""
    from oracle import detdata as dd
    for name in ("frac", "prop5", "int24"):
        x, y, d = cases.warp_inputs(name)
        if name != "int24":
            d = d * 0.4 + 0.3                    # keep the taps mostly inside the image and off the integer grid
        seeds = [dd.t_normalish((x.shape[0], x.shape[1], d.shape[1], x.shape[2], x.shape[3]), 811 + k) for k in range(2)]

        def both(fn, to):
            xs = [to(t).clone().requires_grad_(True) for t in (x, y, d)]
            yw, xw = fn(*xs)
            (yw * to(seeds[0])).sum().add((xw * to(seeds[1])).sum()).backward()
            return [t.grad for t in xs]
        gh = both(sa.ops.SpatialTransformer_grid, dev)
        go = both(oops.SpatialTransformer_grid, lambda t: t)
        check(f"bwd/warp/{name}/x", gh[0], go[0], 1e-5, 1e-6)
        check(f"bwd/warp/{name}/y", gh[1], go[1], 1e-5, 1e-6)          # atomics: summation order differs
        check(f"bwd/warp/{name}/disp", gh[2], go[2], 2e-5, 2e-5)
    for name in sorted(cases.TOPK):
        c, s, k = cases.topk_inputs(name)
        seed = dd.t_normalish((c.shape[0], 1, c.shape[2], c.shape[3]), 821)
        gh = _grads(lambda p, q: sa.ops.regression_topk(p, q, k), [dev(c), dev(s)], lambda yy: dev(seed))
        go = _grads(lambda p, q: oops.regression_topk(p, q, k), [c, s], lambda yy: seed)
        check(f"bwd/topk/{name}/cost", gh[0], go[0], 2e-6, 1e-6)
        check(f"bwd/topk/{name}/samples", gh[1], go[1], 2e-6, 1e-6)


@pytest.mark.parametrize("name", sorted(cases.WARP) + ["c12_w70_int", "c20_w200_frac"])
def test_backward_warp_onto_the_features_alone_row_by_row(sa, name):
    """The live backward of SpatialTransformer_grid at models/SemStereo.py:316: the candidates are INDICES (no gradient), so only the
    feature gradient is formed -- `warp_bwd_rows_kernel`: each wave sums two channel rows in LDS with tagged read-add-writes
    (ss::lds_owned_add2; lanes whose taps land on the same column take turns) and adds the row to memory once.  Against autograd
    through the oracle's restatement (F.grid_sample), on every warp case -- rows narrower than a wave, ragged widths, integer
    candidates that differ between neighbouring pixels (colliding lanes), fractional ones (two taps per row, south taps in the next
    row), and channel counts that leave the second channel of a wave, or whole waves, without work."""
    from oracle import detdata as dd
    if name in cases.WARP:
        x, y, d = cases.warp_inputs(name)
    else:
        C, W, kind = {"c12_w70_int": (12, 70, "int"), "c20_w200_frac": (20, 200, "frac")}[name]
        x, y = dd.t_normalish((2, C, 5, W), 871), dd.t_normalish((2, C, 5, W), 872)
        d = dd.distinct_sorted_candidates(2, 24, 5, W, 32, 873) if kind == "int" else dd.t_uniform((2, 6, 5, W), 873, -20.0, 20.0)
    seeds = [dd.t_normalish((x.shape[0], x.shape[1], d.shape[1], x.shape[2], x.shape[3]), 874 + k) for k in range(2)]

    def both(fn, to):
        xs = [to(x).clone().requires_grad_(True), to(y).clone().requires_grad_(True), to(d).clone()]
        yw, xw = fn(*xs)
        (yw * to(seeds[0])).sum().add((xw * to(seeds[1])).sum()).backward()
        return xs[0].grad, xs[1].grad
    gh = both(sa.ops.SpatialTransformer_grid, dev)
    go = both(oops.SpatialTransformer_grid, lambda t: t)
    check(f"bwd/warp_rows/{name}/x", gh[0], go[0], 1e-5, 1e-6)
    check(f"bwd/warp_rows/{name}/y", gh[1], go[1], 1e-5, 2e-6)              # sums in another order


@pytest.mark.parametrize("case", [
    # (B, C, H, W, nd, kind, margin)
    (1, 32, 6, 64, 24, "int", 16),          # the live form: 32 concat channels, 24 integer candidates
    (2, 12, 5, 128, 6, "int", 16),          # a wave with 4 of its 8 channels, batch 2
    (1, 40, 4, 64, 5, "frac", 64),          # two channel groups on the grid (grad_att through atomics), fractional candidates: four taps, two rows
    (1, 8, 7, 192, 24, "int", 2),           # candidates far outside the windows' margin: every tap the long way
    (1, 16, 1, 64, 3, "frac", 8),           # H == 1
])
def test_concat_volume_training_one_launch_each_way(sa, case):
    """models/SemStereo.py:316-318 under autograd (r06): `att_topk * cat(left broadcast, warp(right))` as ss_concat_sampled_fwd +
    ss_concat_sampled_bwd -- gradients to the left map (sum over the candidates), to the right map (the warp's bilinear scatter, summed
    in LDS windows of the two rows the taps reach) and to att (the ungated volume dotted with the gradient) -- against CPU autograd
    through the oracle's restatement of the reference's three statements."""
    from oracle import detdata as dd
    B, C, H, W, nd, kind, margin = case
    left, right = dd.t_normalish((B, C, H, W), 881), dd.t_normalish((B, C, H, W), 882)
    d = dd.distinct_sorted_candidates(B, nd, H, W, max(nd, 20), 883) if kind == "int" else dd.t_uniform((B, nd, H, W), 883, -20.0, 20.0)
    att = dd.t_uniform((B, 1, nd, H, W), 884, 0.0, 1.0)
    seed = dd.t_normalish((B, 2 * C, nd, H, W), 885)
    T = sa.train
    assert T.concat_volume_applies(dev(left), dev(right), dev(d), dev(att))
    xs = [dev(t).clone().requires_grad_(True) for t in (left, right, att)]
    vol = T.concat_volume_sampled(xs[0], xs[1], dev(d), xs[2], margin=margin)
    (vol * dev(seed)).sum().backward()
    # (fp32 on the CPU, as test_backward_warp_and_topk_in_hip: the coordinate round trip of grid_sample is part of the function --
    # in fp32 an integer candidate leaves ix = integer -+ ~1e-5 and so four live taps; float64 would not)
    rs = [t.clone().requires_grad_(True) for t in (left, right, att)]
    right_w, left_b = oops.SpatialTransformer_grid(rs[0], rs[1], d)
    ref = rs[2] * torch.cat((left_b, right_w), dim=1)
    (ref * seed).sum().backward()
    check(f"train/concat_volume/{case}/fwd", vol, ref, 2e-6, 2e-6)
    for name, a_, r_ in zip(("left", "right", "att"), xs, rs):
        check(f"train/concat_volume/{case}/grad_{name}", a_.grad, r_.grad, 1e-5, 3e-6)


CONV_TRAIN_CASES = [
    # (B, Cin, Cout, D, H, W, stride)
    (2, 32, 32, 4, 10, 36, 1),
    (1, 32, 64, 6, 8, 34, 2),           # stride 2 (even sizes: its data gradient is the k3-s2-p1-op1 transposed conv)
    (1, 64, 32, 3, 7, 33, 1),           # W odd, ragged tile
    (1, 40, 48, 2, 6, 20, 1),           # channels not multiples of 32
    (1, 64, 128, 4, 6, 16, 2),
    (1, 32, 32, 5, 21, 150, 1),         # r06: rows of several 32-position chunks, ragged last chunk (the bf16 weight-gradient kernel's K loop)
    (2, 32, 64, 6, 22, 138, 2),         # ... stride 2 (even / odd column rows), batch 2
    (1, 8, 1, 3, 9, 70, 1),             # ... a single output channel (the classifiers' heads run this kernel too)
    (1, 32, 32, 4, 64, 256, 1),         # the rows of the 1024^2 pair (W/4 = 256: eight chunks per row, columns cut into segments)
    (1, 64, 32, 3, 32, 512, 1),         # ... of the 2048^2 pair, two input-channel tiles
    (1, 32, 64, 4, 64, 256, 2),         # ... stride 2 on 256-wide rows
]


@pytest.mark.parametrize("case", CONV_TRAIN_CASES)
def test_conv3d_training_forward_dgrad_wgrad_in_hip(sa, case):
    """VERDICT r1 missing #2: Conv3d(k3,p1) through the HIP autograd function -- forward, data gradient (the same engine on
    flipped weights / the transposed-conv kernels) and weight gradient (conv3d_wgrad.hip) -- against autograd of
    F.conv3d in float64."""
    if sa.modules.CONV_ENGINE == "bf16x3":
        pytest.skip("SS_CONV_ENGINE=bf16x3: this bound is for the fp32-accurate engines")
    import torch.nn.functional as F
    from oracle import detdata as dd
    B, Cin, Cout, D, H, W, stride = case
    x = dd.t_normalish((B, Cin, D, H, W), 830)
    w = dd.t_uniform((Cout, Cin, 3, 3, 3), 831, -1, 1) * (3.0 / (Cin * 27)) ** 0.5
    conv = torch.nn.Conv3d(Cin, Cout, 3, stride, 1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(w)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y64 = F.conv3d(x64, w64, None, stride, 1)
    seed = dd.t_normalish(tuple(y64.shape), 832)
    y64.backward(seed.double())
    conv = conv.cuda()
    xg = dev(x).requires_grad_(True)
    before = sa.modules.PATH_COUNTS.get("hip_train", 0)
    y = sa.modules.conv3d_train(conv, xg)
    assert sa.modules.PATH_COUNTS.get("hip_train", 0) == before + 1, "the stock PyTorch layer ran"
    y.backward(dev(seed))
    scale = lambda t: float(t.detach().abs().max())                        # noqa: E731
    e_y = float((y.detach().double().cpu() - y64.detach()).abs().max()) / scale(y64)
    e_x = float((xg.grad.double().cpu() - x64.grad).abs().max()) / scale(x64.grad)
    e_w = float((conv.weight.grad.double().cpu() - w64.grad).abs().max()) / scale(w64.grad)
    REPORT[f"conv3d_train/{case}"] = (e_y, e_x, e_w)
    assert e_y <= 2e-6 and e_x <= 2e-6 and e_w <= 5e-6, (e_y, e_x, e_w)


@pytest.mark.parametrize("form", ["f32", "per_wave"])
def test_conv3d_weight_gradient_other_forms(sa, form, tuning_env, monkeypatch):
    """The weight-gradient kernels that are not the default: the exact-fp32 MFMA kernel of rounds 2-5 (SS_WGRAD_ENGINE=f32) and the
    per-wave form of the stride-1 bf16 kernel (SS_WGRAD_COOP=0) -- same bound as the default forms, on shapes with ragged chunks,
    a single output channel and channel counts that are not multiples of 32."""
    import torch.nn.functional as F
    from oracle import detdata as dd
    if form == "f32":
        monkeypatch.setattr(sa.train_layers, "WGRAD_ENGINE", "f32")
    else:
        tuning_env("SS_WGRAD_COOP", "0")
    for (B, Cin, Cout, D, H, W, stride) in [(1, 32, 32, 5, 21, 150, 1), (1, 40, 48, 2, 6, 20, 1), (1, 8, 1, 3, 9, 70, 1), (2, 32, 64, 6, 22, 138, 2)]:
        x = dd.t_normalish((B, Cin, D, H, W), 850)
        w64 = (dd.t_uniform((Cout, Cin, 3, 3, 3), 851, -1, 1) * (3.0 / (Cin * 27)) ** 0.5).double().requires_grad_(True)
        y64 = F.conv3d(x.double(), w64, None, stride, 1)
        seed = dd.t_normalish(tuple(y64.shape), 852)
        y64.backward(seed.double())
        gw = sa.train_layers.conv3d_wgrad_hip(dev(seed), dev(x), Cout, Cin, stride)
        e_w = float((gw.double().cpu() - w64.grad).abs().max()) / float(w64.grad.abs().max())
        REPORT[f"conv3d_wgrad/{form}/{(B, Cin, Cout, D, H, W, stride)}"] = e_w
        assert e_w <= 5e-6, (form, e_w)


@pytest.mark.parametrize("case", [(1, 64, 32, 3, 6, 18), (2, 128, 64, 2, 4, 8), (1, 48, 40, 2, 5, 33)])
def test_deconv3d_training_forward_dgrad_wgrad_in_hip(sa, case):
    """ConvTranspose3d(k3,s2,p1,op1) of the hourglasses (models/SemStereo.py:124-130) through the HIP autograd function."""
    if sa.modules.CONV_ENGINE == "bf16x3":
        pytest.skip("SS_CONV_ENGINE=bf16x3: this bound is for the fp32-accurate engines")
    import torch.nn.functional as F
    from oracle import detdata as dd
    B, Cin, Cout, D, H, W = case
    x = dd.t_normalish((B, Cin, D, H, W), 840)
    w = dd.t_uniform((Cin, Cout, 3, 3, 3), 841, -1, 1) * (3.0 / (Cin * 27 / 8)) ** 0.5
    dc = torch.nn.ConvTranspose3d(Cin, Cout, 3, padding=1, output_padding=1, stride=2, bias=False)
    with torch.no_grad():
        dc.weight.copy_(w)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y64 = F.conv_transpose3d(x64, w64, None, stride=2, padding=1, output_padding=1)
    seed = dd.t_normalish(tuple(y64.shape), 842)
    y64.backward(seed.double())
    dc = dc.cuda()
    xg = dev(x).requires_grad_(True)
    before = sa.modules.PATH_COUNTS.get("hip_train", 0)
    y = sa.modules.deconv3d_train(dc, xg)
    assert sa.modules.PATH_COUNTS.get("hip_train", 0) == before + 1
    y.backward(dev(seed))
    scale = lambda t: float(t.detach().abs().max())                        # noqa: E731
    e_y = float((y.detach().double().cpu() - y64.detach()).abs().max()) / scale(y64)
    e_x = float((xg.grad.double().cpu() - x64.grad).abs().max()) / scale(x64.grad)
    e_w = float((dc.weight.grad.double().cpu() - w64.grad).abs().max()) / scale(w64.grad)
    REPORT[f"deconv3d_train/{case}"] = (e_y, e_x, e_w)
    assert e_y <= 2e-6 and e_x <= 2e-6 and e_w <= 5e-6, (e_y, e_x, e_w)


@pytest.fixture
def counted_bf16s_deconv(sa, monkeypatch):
    """training's transposed conv (train_layers._deconv_k3_forward) takes the bf16s kernel at any size; -> the shapes it was given"""
    calls = []
    inner = sa.train_layers.deconv3d_bf16s_hip

    def counted(x, *a, **k):
        calls.append(tuple(x.shape))
        return inner(x, *a, **k)
    monkeypatch.setattr(sa.engine, "DECONV_MIN_WORKGROUPS", 0)
    monkeypatch.setattr(sa.engine, "DECONV_BF16S", True)
    monkeypatch.setattr(sa.train_layers, "deconv3d_bf16s_hip", counted)
    return calls


@pytest.mark.parametrize("groups", ["0", "1"])
def test_deconv3d_training_in_the_forms_of_large_layers(sa, groups, tuning_env, counted_bf16s_deconv):
    """test_deconv3d_training_forward_dgrad_wgrad_in_hip's first case with the forward on the forms a full-size layer gets
    (SS_DECONV_GROUPS=0: all 8 parity classes per workgroup; 1: two class groups), no skip tensor and a zero shift"""
    assert sa.engine._deconv_nterms() == 19, "the class groups are forms of the fp16 engine"
    tuning_env("SS_DECONV_GROUPS", groups)
    test_deconv3d_training_forward_dgrad_wgrad_in_hip(sa, (1, 64, 32, 3, 6, 18))
    assert counted_bf16s_deconv == [(1, 64, 3, 6, 18)]


@pytest.mark.parametrize("groups", ["0", "1"])
def test_conv3d_stride2_data_gradient_in_the_forms_of_large_layers(sa, groups, tuning_env, counted_bf16s_deconv):
    """the stride-2 case (1, 32, 64, 6, 8, 34, 2) of CONV_TRAIN_CASES: its data gradient is the transposed conv of the output
    gradient [1, 64, 3, 4, 17], run here on the forms a full-size layer gets"""
    assert sa.engine._deconv_nterms() == 19, "the class groups are forms of the fp16 engine"
    tuning_env("SS_DECONV_GROUPS", groups)
    test_conv3d_training_forward_dgrad_wgrad_in_hip(sa, (1, 32, 64, 6, 8, 34, 2))
    assert counted_bf16s_deconv == [(1, 64, 3, 4, 17)]


def _rel(a, ref):
    return float((a.double().cpu() - ref.double().cpu()).abs().max()) / (float(ref.double().abs().max()) + 1e-30)


def test_training_kernels_vs_float64_autograd(sa):
    """semstereo_amd/train.py: every HIP autograd function (forward AND backward kernels) against the float64 CPU autograd of
    the PyTorch op it replaces -- BatchNorm with batch statistics (+ ReLU, running statistics), 1x1(x1) convolutions with and
    without bias on 4-D and 5-D tensors, the 3x3 Conv2d, the depthwise `patch`, the channelAtt gate, the windowed attention
    block (both window shapes of the model)."""
    import torch.nn as nn
    import torch.nn.functional as F
    from oracle import detdata as dd
    T = sa.train
    before = dict(sa.modules.PATH_COUNTS)

    def run(fn_hip, fn_ref, inputs, tol, name):
        hip_in = [dev(t).clone().requires_grad_(True) for t in inputs]
        ref_in = [t.double().clone().requires_grad_(True) for t in inputs]
        y, yr = fn_hip(*hip_in), fn_ref(*ref_in)
        REPORT[f"train/{name}/fwd"] = _rel(y, yr)
        assert _rel(y, yr) <= tol, (name, "forward", _rel(y, yr))
        go = dd.t_normalish(tuple(yr.shape), 777)
        y.backward(dev(go)); yr.backward(go.double())
        for i, (a_, r_) in enumerate(zip(hip_in, ref_in)):
            e = _rel(a_.grad, r_.grad)
            REPORT[f"train/{name}/grad{i}"] = e
            assert e <= tol, (name, "grad of input", i, e)

    # BatchNorm3d / 2d, batch statistics, with and without ReLU
    for relu, shape in ((True, (2, 8, 3, 5, 7)), (False, (3, 4, 6, 9)), (True, (1, 32, 4, 16, 20))):
        C = shape[1]
        bn = (nn.BatchNorm3d if len(shape) == 5 else nn.BatchNorm2d)(C).cuda().train()
        bnr = (nn.BatchNorm3d if len(shape) == 5 else nn.BatchNorm2d)(C).double().train()

        def hip(x, w, b_):
            bn.weight, bn.bias = nn.Parameter(w.detach()), nn.Parameter(b_.detach())
            y_ = T._BatchNormTrain.apply(x, w, b_, bn.eps, relu, None, None)[0]
            return y_

        def ref(x, w, b_):
            y_ = F.batch_norm(x, None, None, w, b_, True, 0.0, bnr.eps)
            return F.relu(y_) if relu else y_
        run(hip, ref, [dd.t_normalish(shape, 701) * 2 + 0.3, dd.t_uniform((C,), 702, 0.5, 1.5), dd.t_uniform((C,), 703, -0.3, 0.3)], 2e-5, f"bn{shape}{relu}")
        x = dev(dd.t_normalish(shape, 704))
        y = T.batchnorm_train(bn, x, relu)                         # running statistics as F.batch_norm updates them
        bn2 = (nn.BatchNorm3d if len(shape) == 5 else nn.BatchNorm2d)(C).cuda().train()
        bn2(x)
        assert _rel(bn.running_mean, bn2.running_mean) <= 1e-5 and _rel(bn.running_var, bn2.running_var) <= 1e-5
        assert int(bn.num_batches_tracked) == 1
    # ... with the skip branch joining behind the normalisation and before the ReLU (r04: the `F.relu(conv5(..) + redir2(..))` of
    # hourglass.forward, models/SemStereo.py:141-142, inside the BatchNorm apply): forward, and gradients of x, weight, bias, residual
    for shape in ((2, 8, 3, 5, 7), (1, 32, 4, 16, 20)):
        C = shape[1]
        run(lambda x, w, b_, r_: T._BatchNormTrain.apply(x, w, b_, 1e-5, True, r_, None)[0],
            lambda x, w, b_, r_: F.relu(F.batch_norm(x, None, None, w, b_, True, 0.0, 1e-5) + r_),
            [dd.t_normalish(shape, 705) * 2 + 0.3, dd.t_uniform((C,), 706, 0.5, 1.5), dd.t_uniform((C,), 707, -0.3, 0.3),
             dd.t_normalish(shape, 708)], 2e-5, f"bn_res{shape}")
    # BatchNorm in eval() under autograd (r05: frozen running statistics, learnable affine, gradients to the input and the residual):
    # against F.batch_norm(training=False) in float64; and through batchnorm_train on a module in eval(), which must not move its
    # running statistics and must not take a PyTorch layer
    for relu, shape, with_res in ((True, (2, 8, 3, 5, 7), True), (False, (3, 4, 6, 9), False), (True, (1, 32, 4, 16, 20), False)):
        C = shape[1]
        rm, rv = dd.t_uniform((C,), 731, -0.4, 0.4), dd.t_uniform((C,), 732, 0.5, 2.0)

        def hip_e(x, w, b_, *r_):
            inv = torch.rsqrt(dev(rv) + 1e-5)
            return T._BatchNormEval.apply(x, w, b_, dev(rm), inv, relu, r_[0] if r_ else None)

        def ref_e(x, w, b_, *r_):
            y_ = F.batch_norm(x, rm.double(), rv.double(), w, b_, False, 0.0, 1e-5)
            if r_:
                y_ = y_ + r_[0]
            return F.relu(y_) if relu else y_
        ins = [dd.t_normalish(shape, 733) * 2 + 0.3, dd.t_uniform((C,), 734, 0.5, 1.5), dd.t_uniform((C,), 735, -0.3, 0.3)]
        if with_res:
            ins.append(dd.t_normalish(shape, 736))
        run(hip_e, ref_e, ins, 2e-5, f"bn_eval{shape}{relu}")
        bn = (nn.BatchNorm3d if len(shape) == 5 else nn.BatchNorm2d)(C).cuda().eval()
        with torch.no_grad():
            bn.running_mean.copy_(dev(rm)); bn.running_var.copy_(dev(rv))
        x = dev(dd.t_normalish(shape, 737)).requires_grad_(True)
        before = dict(sa.modules.PATH_COUNTS)
        y = T.batchnorm_train(bn, x, relu)
        assert sa.modules.PATH_COUNTS["torch"] == before["torch"] and sa.modules.PATH_COUNTS["hip_train"] > before.get("hip_train", 0)
        want = F.relu(bn(x)) if relu else bn(x)
        assert _rel(y, want) <= 1e-6 and torch.equal(bn.running_mean, dev(rm)) and int(bn.num_batches_tracked) == 0
        y.sum().backward()
        assert x.grad is not None and bn.weight.grad is not None and bn.bias.grad is not None
    # 1x1 convolutions: redir (32 -> 32, no bias, 5-D), qkv (128 -> 384, bias), im_att (256 -> 128 on a 2-D map, bias)
    for (cin, cout, shp, bias) in ((32, 32, (2, 3, 6, 9), False), (128, 384, (1, 4, 8, 8), True), (256, 128, (2, 12, 20), True), (64, 32, (1, 7, 5), True)):
        ins = [dd.t_normalish((shp[0], cin) + shp[1:], 711), dd.t_uniform((cout, cin) + (1,) * (len(shp) - 1), 712, -0.2, 0.2)]
        if bias:
            ins.append(dd.t_uniform((cout,), 713, -0.5, 0.5))
        conv = F.conv3d if len(shp) == 4 else F.conv2d
        run(lambda x, w, b_=None: T.conv_k1(x, w, b_), lambda x, w, b_=None: conv(x, w, b_), ins, 2e-5, f"k1_{cin}_{cout}_{len(shp)}")
    # 3x3 Conv2d (concat_feature)
    c2 = nn.Conv2d(16, 24, 3, 1, 1, bias=False).cuda()
    run(lambda x, w: T._Conv2dK3.apply(x, w), lambda x, w: F.conv2d(x, w, None, 1, 1), [dd.t_normalish((2, 16, 9, 37), 721), dd.t_uniform((24, 16, 3, 3), 722, -0.2, 0.2)],
        2e-5, "conv2d_k3")
    assert sa.modules._is_plain_3x3(c2)
    # depthwise patch
    run(lambda x, w: T._DepthwisePatch.apply(x, w), lambda x, w: F.conv3d(x, w, None, 1, (0, 1, 1), 1, 8),
        [dd.t_normalish((2, 8, 5, 9, 12), 731), dd.t_uniform((8, 1, 1, 3, 3), 732, -1, 1)], 2e-5, "patch")
    # channelAtt gate
    run(lambda a_, cv: T._ChannelGate.apply(a_, cv), lambda a_, cv: torch.sigmoid(a_).unsqueeze(2) * cv,
        [dd.t_normalish((2, 8, 6, 10), 741), dd.t_normalish((2, 8, 4, 6, 10), 742)], 2e-5, "gate")
    # attention block, both window shapes
    # (r04: also volumes whose H, W are not window multiples -- both padded (the -1000 mask), only W, only H (the reference's `-0:`
    # quirk: no mask) -- whose pad tokens carry the qkv bias and feed its gradient)
    for blk, shape in (((4, 4, 4), (1, 128, 8, 8, 12)), ((6, 4, 4), (2, 128, 6, 8, 8)), ((4, 4, 4), (1, 128, 8, 6, 10)),
                       ((6, 4, 4), (1, 128, 6, 8, 9)), ((4, 4, 4), (2, 128, 4, 7, 8))):
        ab = sa.modules.attention_block(128, 16, blk)
        with torch.no_grad():
            for i, p_ in enumerate(ab.parameters()):
                p_.copy_(dd.t_uniform(tuple(p_.shape), 750 + i, -0.1, 0.1))
        abr = __import__("copy").deepcopy(ab).double()
        ab = ab.cuda().train()
        x = dd.t_normalish(shape, 760)
        xh, xr = dev(x).requires_grad_(True), x.double().requires_grad_(True)
        assert T.window_attention_applies(xh, 16, blk)
        y, yr = ab(xh), abr._forward_torch(xr)
        assert _rel(y, yr) <= 2e-5, _rel(y, yr)
        go = dd.t_normalish(shape, 761)
        y.backward(dev(go)); yr.backward(go.double())
        assert _rel(xh.grad, xr.grad) <= 5e-5, _rel(xh.grad, xr.grad)
        for (n_, p_), (_, pr_) in zip(ab.named_parameters(), abr.named_parameters()):
            REPORT[f"train/attention{blk}/{n_}"] = _rel(p_.grad, pr_.grad)
            assert _rel(p_.grad, pr_.grad) <= 5e-5, (n_, _rel(p_.grad, pr_.grad))
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"], "a PyTorch layer ran inside the HIP training functions"


@pytest.mark.parametrize("m", [8, 12])
def test_attention_tail_training_functions_vs_float64_autograd(sa, m):
    """Round 4: the three fused attention-tail launches (models/SemStereo.py:279-285, :286-293, :295-310) as
    autograd functions -- HIP forward AND backward kernels (attention_tail_bwd.hip) -- against float64 CPU autograd of the
    reference's statement-by-statement composition (the oracle's ops)."""
    import torch.nn.functional as F
    from oracle import detdata as dd
    T = sa.train
    B, Hc, Wc, C, K = 2, 5, 7, 12, 6
    H, W, D = 2 * Hc, 2 * Wc, 2 * m
    rng = (-m, 2 * m)

    def grads_close(hip_in, ref_in, tol, name):
        for i, (a_, r_) in enumerate(zip(hip_in, ref_in)):
            if r_.grad is None:
                continue
            e = _rel(a_.grad, r_.grad)
            REPORT[f"train/tail_{name}/m{m}/grad{i}"] = e
            assert e <= tol, (name, "gradient of input", i, e)

    # ---- :279-285 ----
    coarse = dd.t_normalish((B, 1, m, Hc, Wc), 801) * 2
    ch, cr = dev(coarse).requires_grad_(True), coarse.double().requires_grad_(True)
    up, disp, var = T._UpsampleSoftmaxRegression.apply(ch, H, W, rng)
    upr = F.interpolate(cr, [D, H, W], mode="trilinear")
    pr = F.softmax(upr.squeeze(1), dim=1)
    dispr = oops.disparity_regression(pr, m)
    varr = oops.disparity_variance(pr, m, dispr.unsqueeze(1))
    assert _rel(up, upr) <= 2e-6 and _rel(disp, dispr) <= 2e-5 and _rel(var, varr) <= 2e-5
    g1, g2, g3 = dd.t_normalish(tuple(upr.shape), 802), dd.t_normalish(tuple(dispr.shape), 803), dd.t_normalish(tuple(varr.shape), 804)
    ((up * dev(g1)).sum() + (disp * dev(g2)).sum() + (var * dev(g3)).sum()).backward()
    ((upr * g1.double()).sum() + (dispr * g2.double()).sum() + (varr * g3.double()).sum()).backward()
    grads_close([ch], [cr], 2e-5, "upsoft")

    # ---- :286-293 (candidate disparities kept away from integers: the bilinear derivative jumps there) ----
    left, right = dd.stereo_features(B, C, H, W, 5, max_shift=3)
    frac = dd.t_uniform((B, H, W), 811, 0.2, 0.8)
    pred0 = torch.round(dd.t_uniform((B, H, W), 812, -5.0, 5.0)) + frac
    varin = dd.t_uniform((B, 1, H, W), 813, 0.0, 20.0)
    gamma, beta = torch.tensor([0.25]), torch.tensor([2.0])
    ins = [left, right, pred0, varin, gamma, beta]
    hin = [dev(t).clone().requires_grad_(True) for t in ins]
    rin = [t.double().clone().requires_grad_(True) for t in ins]
    st = T._SampleStrength.apply(*hin)
    v = torch.sigmoid(rin[5] + rin[4] * rin[3])
    rw, lb = oops.SpatialTransformer_grid(rin[0], rin[1], oops.propagation(rin[2].unsqueeze(1)))
    str_ = torch.softmax((lb * rw).mean(dim=1) * oops.propagation(v), dim=1)
    assert _rel(st, str_) <= 2e-5, _rel(st, str_)
    go = dd.t_normalish(tuple(str_.shape), 814)
    (st * dev(go)).sum().backward(); (str_ * go.double()).sum().backward()
    grads_close(hin, rin, 5e-5, "strength")

    # ---- :295-310 ----
    logits = dd.t_normalish((B, 1, D, H, W), 821) * 3.0
    strength = torch.softmax(dd.t_normalish((B, 5, H, W), 822), dim=1)
    lh, sh = dev(logits).requires_grad_(True), dev(strength).requires_grad_(True)
    lr, sr = logits.double().requires_grad_(True), strength.double().requires_grad_(True)
    att_topk, samples, pred_att = T._TopkCandidates.apply(lh, sh, K, rng)
    aw = (oops.propagation_prob(lr) * sr.unsqueeze(2)).sum(dim=1, keepdim=True)
    prob = F.softmax(aw, dim=2)
    _, ind = prob.sort(dim=2, descending=True, stable=True)
    ind_k = ind[:, :, :K].sort(2, False)[0]
    att_r = torch.gather(prob, 2, ind_k)
    smp_r = ind_k.squeeze(1).double() - m
    pred_r = (F.softmax(torch.gather(aw, 2, ind_k).squeeze(1), dim=1) * smp_r).sum(dim=1)
    assert torch.equal(samples.cpu().double(), smp_r), "candidate sets differ"
    assert _rel(att_topk, att_r) <= 2e-5 and _rel(pred_att, pred_r) <= 2e-5
    ga, gp = dd.t_normalish(tuple(att_r.shape), 823), dd.t_normalish(tuple(pred_r.shape), 824)
    ((att_topk * dev(ga)).sum() + (pred_att * dev(gp)).sum()).backward()
    ((att_r * ga.double()).sum() + (pred_r * gp.double()).sum()).backward()
    grads_close([lh, sh], [lr, sr], 5e-5, "topk")


@pytest.mark.parametrize("name", ["s128", "s96x160_b2", "t256_md64"])
def test_hot_segment_training_step_runs_on_the_hip_stack(sa, name):
    """A training-mode pass of the hot segment (BatchNorm with batch statistics, autograd on: main_us3d.py:186-222): every
    module of the 3-D stack runs HIP autograd functions (no PyTorch layer: PATH_COUNTS["torch"] does not move), every
    parameter receives a finite gradient, and the gradients agree with the ORACLE's -- the functional restatement of the
    graph (oracle/hot_segment.py) in training mode, float64, CPU autograd.  `s96x160_b2` (r04): batch 2, and neither H nor W
    of either hourglass's coarsest level is a window multiple (3 x 5 and 6 x 10 voxels for 4 x 4 windows): the windowed
    attention with pad tokens, forward and backward, on the HIP kernels."""
    if sa.modules.CONV_ENGINE == "bf16x3":
        pytest.skip("SS_CONV_ENGINE=bf16x3: this bound is for the fp32-accurate engines")
    fl4, fr4, fl8, fr8, maxdisp = cases.segment_inputs(name)
    seg, P = _segment(sa, maxdisp)
    seg.train()
    before = dict(sa.modules.PATH_COUNTS)
    r = seg(dev(fl4), dev(fr4), dev(fl8), dev(fr8))
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"], "a PyTorch layer ran in the training pass of the 3-D stack"
    assert sa.modules.PATH_COUNTS.get("hip_train", 0) - before.get("hip_train", 0) >= 60
    (r["pred"].mean() + r["pred_att"].mean()).backward()
    grads = {k: v.grad.detach().cpu() for k, v in seg.named_parameters() if v.grad is not None}
    assert len(grads) > 60 and all(bool(torch.isfinite(g_).all()) for g_ in grads.values())
    # the oracle: same parameters, float64, CPU autograd, BatchNorm on batch statistics
    P64 = {k: v.double().clone().requires_grad_(v.is_floating_point() and not k.endswith(("running_mean", "running_var"))) for k, v in P.items()}
    hip_smp = r["samples"].detach().cpu().double()
    with ostack.training_mode():
        # the oracle's own picks first: the HIP pass may pick otherwise ONLY where the oracle's 24th / 25th probabilities are within
        # DELTA24_REL of each other (r04: the fused selection kernel rounds the propagated logits in another order than the
        # statement-by-statement composition) ...
        keep = {}
        with torch.no_grad():
            _, smp0, _ = oseg.attention_branch({k: v.detach() for k, v in P64.items()}, fl8.double(), fr8.double(), fl4.double(), fr4.double(),
                                               maxdisp, keep)
        other = (hip_smp != smp0).any(dim=1)
        REPORT[f"segment_train/{name}/pixels_with_other_candidates"] = int(other.sum())
        assert int(other.sum()) <= 2 and bool((keep["gap24_rel"][other] < cases.DELTA24_REL).all()), (int(other.sum()), keep["gap24_rel"][other])
        # ... and the gradients are compared like for like: the oracle differentiated on the HIP pass's candidates
        att, smp, pred_att = oseg.attention_branch(P64, fl8.double(), fr8.double(), fl4.double(), fr4.double(), maxdisp, force_samples=hip_smp)
        pred = oseg.matching_branch(P64, fl4.double(), fr4.double(), att, smp)
    (pred.mean() + pred_att.mean()).backward()
    same = (hip_smp == smp).all(dim=1)
    REPORT["segment_train/pixels_with_the_oracles_candidates"] = float(same.double().mean())
    errs = {}
    for k, g_ in grads.items():
        ref = P64[k].grad
        assert ref is not None, k
        errs[k] = float((g_.double() - ref).abs().max()) / (float(ref.abs().max()) + 1e-12)
    # gamma / beta (models/SemStereo.py:204-205) are scalars whose gradient is a sum of signed per-pixel contributions through the
    # 5-candidate probe that nearly cancel: held to the scale of the other gradients instead of to their own magnitude
    gscale = max(float(P64[k].grad.abs().max()) for k in grads)
    for k in ("gamma", "beta"):
        REPORT[f"segment_train/{k}_grad"] = [float(grads[k].reshape(-1)[0]), float(P64[k].grad.reshape(-1)[0])]
        assert float((grads[k].double() - P64[k].grad).abs().max()) <= 1e-4 * gscale, (k, grads[k], P64[k].grad, gscale)
        errs.pop(k)
    worst = max(errs.values())
    med = sorted(errs.values())[len(errs) // 2]
    REPORT["segment_train/worst_relative_grad_diff_vs_oracle_f64"] = worst
    REPORT["segment_train/median_relative_grad_diff_vs_oracle_f64"] = med
    # batch statistics over 8 x 8 x 8 voxels at the coarsest level and the hard top-24 / top-2 picks amplify fp32 rounding:
    # typical 1e-6 ... 1e-5, worst parameter a few 1e-4 -- as long as every discontinuity of the graph falls on the oracle's side.
    # The picks are checked here; a ReLU is not: under SS_CONV_ENGINE=f32 one of the 786 432 pre-activations of classif.0 lies
    # within rounding of zero and lands on the other side, and every gradient upstream of it moves by 2-5e-3 of its scale while
    # every kernel call of the pass is within 2e-6 of float64 on its own inputs (tools/err_train_step.py).  The tight bound is
    # asserted for the engines that hit no such flip on this fixture, the loose one guards the others against a wrong kernel.
    same_picks = bool(same.all()) and float((r["pred"].detach().cpu().double() - pred.detach()).abs().max()) <= 1e-3      # (top-24 and top-2)
    REPORT["segment_train/same_picks_as_the_oracle"] = same_picks
    # (s96x160_b2 with the fused attention tail: the matching-branch gradients sit at 3e-3 of their scale with classif.2 at 1e-6 -- the
    # signature of ONE classif.0 pre-activation on the other side of zero (tools/err_train_step.py s96x160_b2 [notail]: with the
    # statement-by-statement tail the same pass is at 1e-5 ... 4e-4); the per-kernel tests above hold every function to 5e-5)
    # (r06, VERDICT r5 #5: `t256_md64` -- 256 x 256 at the reference's training default maxdisp 64, main_us3d.py:54 -- is held to the
    # TIGHT bound as well: its closed-form input was chosen so that no ReLU lands on the other side of zero)
    tight = (name == "s128" and sa.modules.CONV_ENGINE in ("f16x3", "bf16x6")) or (name == "t256_md64" and sa.modules.CONV_ENGINE == "f16x3")
    if same_picks and tight:
        assert med <= 1e-4 and worst <= 5e-3, (med, worst, max(errs, key=errs.get))
    else:
        assert med <= 5e-3 and worst <= 5e-2, (med, worst, max(errs, key=errs.get), float(same.double().mean()))


def test_hot_segment_training_step_full_size_smoke(sa):
    """one training step at the size the reference trains at (1024 x 1024 tiles, maxdisp 64: main_us3d.py:54, 74,
    186-222), batch 1: every parameter and every feature map receives a finite gradient, no PyTorch layer runs in the 3-D stack
    (PATH_COUNTS["torch"] does not move), and a second pass without a weight update reproduces the gradients to rounding (the
    scatter / statistics kernels sum through atomics, whose order differs between runs).  tools/bench_train.py times this step."""
    if sa.modules.CONV_ENGINE == "bf16x3":
        pytest.skip("SS_CONV_ENGINE=bf16x3")
    import torch.nn.functional as F
    from oracle import detdata as dd
    H = W = 1024
    maxdisp = 64
    seg, _ = _segment(sa, maxdisp)
    seg.train()
    fl8, fr8 = dd.stereo_features(1, 256, H // 8, W // 8, 870, max_shift=3)
    fl4, fr4 = dd.stereo_features(1, 128, H // 4, W // 4, 871, max_shift=6)
    feats = [dev(t).requires_grad_(True) for t in (fl4, fr4, fl8, fr8)]
    gt = dev(dd.t_uniform((1, H // 4, W // 4), 872, -15.0, 15.0))
    before = dict(sa.modules.PATH_COUNTS)
    torch.cuda.reset_peak_memory_stats()

    def grads_of_a_pass():
        for p_ in seg.parameters():
            p_.grad = None
        for t in feats:
            t.grad = None
        r = seg(*feats)
        (F.smooth_l1_loss(r["pred"].squeeze(1), gt) + F.smooth_l1_loss(r["pred_att"], gt)).backward()
        return {k: v.grad.detach().clone() for k, v in seg.named_parameters() if v.grad is not None}, [t.grad.detach().clone() for t in feats]
    g1, f1 = grads_of_a_pass()
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"], "a PyTorch layer ran in the training pass of the 3-D stack"
    assert sa.modules.PATH_COUNTS.get("hip_train", 0) - before.get("hip_train", 0) >= 60
    assert len(g1) > 60 and all(bool(torch.isfinite(g_).all()) for g_ in g1.values()) and all(bool(torch.isfinite(g_).all()) for g_ in f1)
    assert all(float(g_.abs().max()) > 0 for g_ in f1), "a feature map received no gradient"
    REPORT["segment_train/full_size_peak_allocated_gb"] = torch.cuda.max_memory_allocated() / 2 ** 30
    g2, f2 = grads_of_a_pass()
    worst = max(float((g2[k] - g1[k]).abs().max()) / (float(g1[k].abs().max()) + 1e-30) for k in g1 if k not in ("gamma", "beta"))
    worst_f = max(float((a - b).abs().max()) / (float(a.abs().max()) + 1e-30) for a, b in zip(f1, f2))
    REPORT["segment_train/full_size_rerun_rel_diff"] = [worst, worst_f]
    assert worst <= 1e-4 and worst_f <= 1e-4, (worst, worst_f)


# --------------------------------------------------------------------------------------
# the unsigned-range op set (models/submodule_.py) and the SemStereo_WHU graph (VERDICT r1 missing #3)
# --------------------------------------------------------------------------------------

def test_unsigned_op_set_vs_reference_fixture(sa, golden):
    from oracle import ops_unsigned as uops
    U = sa.ops_unsigned
    g = golden["ops_unsigned"]
    for n in sorted(cases.UGWC):
        a, b, m, G = cases.ugwc_inputs(n)
        ref = g[f"ugwc/{n}"] if f"ugwc/{n}" in g.files else uops.build_gwc_volume(a, b, m, G)
        refn = g[f"ugwc_norm/{n}"] if f"ugwc_norm/{n}" in g.files else uops.build_gwc_volume_norm(a, b, m, G)
        check(f"ugwc/{n}", U.build_gwc_volume(dev(a), dev(b), m, G), ref, 1e-6)
        check(f"ugwc_norm/{n}", U.build_gwc_volume_norm(dev(a), dev(b), m, G), refn, 2e-6)
    for n in sorted(cases.UCONCAT):
        a, b, m = cases.uconcat_inputs(n)
        ref = g[f"uconcat/{n}"] if f"uconcat/{n}" in g.files else uops.build_concat_volume(a, b, m)
        check(f"uconcat/{n}", U.build_concat_volume(dev(a), dev(b), m), ref, 0.0)
    for n in sorted(cases.UREGRESSION):
        p, m, d = cases.uregression_inputs(n)
        check(f"uregression/{n}", U.disparity_regression(dev(p), m), g[f"uregression/{n}"], 2e-6)
        check(f"uvariance/{n}", U.disparity_variance(dev(p), m, dev(d)), g[f"uvariance/{n}"], 2e-5, 1e-6)
    # backward of the unsigned volume builders against the oracle's autograd
    from oracle import detdata as dd
    a, b = dd.t_normalish((2, 16, 5, 12), 871), dd.t_normalish((2, 16, 5, 12), 872)
    seed = dd.t_normalish((2, 4, 8, 5, 12), 873)
    gh = _grads(lambda p, q: U.build_gwc_volume_norm(p, q, 8, 4), [dev(a), dev(b)], lambda y: dev(seed))
    go = _grads(lambda p, q: uops.build_gwc_volume_norm(p, q, 8, 4), [a, b], lambda y: seed)
    for i, (x, r) in enumerate(zip(gh, go)):
        check(f"bwd/ugwc_norm/{i}", x, r, 2e-5)
    seed = dd.t_normalish((2, 32, 8, 5, 12), 874)
    gh = _grads(lambda p, q: U.build_concat_volume(p, q, 8), [dev(a), dev(b)], lambda y: dev(seed))
    go = _grads(lambda p, q: uops.build_concat_volume(p, q, 8), [a, b], lambda y: seed)
    for i, (x, r) in enumerate(zip(gh, go)):
        check(f"bwd/uconcat/{i}", x, r, 1e-5)


def test_op_library_at_configs0_maxdisp48(sa):
    """BASELINE.json configs[0]: a 256 x 256 pair at maxdisp = 48 (m8 = 6, m4 = 12: disparity ranges that are NOT multiples
    of 4 / 8, so the volume kernels take their generic forms and the gwc -> patch -> gate fusion does not apply).  The
    whole graph needs maxdisp % 64 == 0, so this is the op library stand-alone against the oracle."""
    import torch.nn.functional as F
    from oracle import detdata as dd
    m8, m4, H8, H4 = 6, 12, 32, 64
    fl8, fr8 = dd.stereo_features(1, 256, H8, H8, 881, 3)
    assert not sa.ops.gwc_patch_gate_applies(fl8, m8, 32)
    check("md48/gwc_norm", sa.ops.build_gwc_volume_norm(dev(fl8), dev(fr8), m8, 32), oops.build_gwc_volume_norm(fl8, fr8, m8, 32), 2e-6)
    check("md48/gwc", sa.ops.build_gwc_volume(dev(fl8), dev(fr8), m8, 32), oops.build_gwc_volume(fl8, fr8, m8, 32), 1e-6, 1e-6)
    cl, cr = dd.stereo_features(1, 32, H4, H4, 882, 6)
    got = sa.ops.build_concat_volume(dev(cl), dev(cr), m4)
    assert torch.equal(got.cpu(), oops.build_concat_volume(cl, cr, m4))
    coarse = dd.t_normalish((1, 1, m4, H8, H8), 883) * 2.0
    up = F.interpolate(coarse, [2 * m4, H4, H4], mode="trilinear")
    prob = F.softmax(up.squeeze(1), dim=1)
    want0 = oops.disparity_regression(prob, m4)
    check("md48/regression", sa.ops.disparity_regression(dev(prob), m4), want0, 1e-5)
    check("md48/variance", sa.ops.disparity_variance(dev(prob), m4, dev(want0.unsqueeze(1))), oops.disparity_variance(prob, m4, want0.unsqueeze(1)), 1e-4)
    assert sa.ops.upsample_softmax_regression_applies(dev(coarse), m4, H4, H4)
    up_h, p0, var = sa.ops.upsample_softmax_regression(dev(coarse), m4, H4, H4)
    check("md48/upsample", up_h, up, 2e-6)
    check("md48/upsample_regression", p0, want0, 1e-5)
    check("md48/upsample_variance", var, oops.disparity_variance(prob, m4, want0.unsqueeze(1)), 1e-4)
    fl4, fr4 = dd.stereo_features(1, 128, H4, H4, 884, 6)
    g_, b_ = torch.full((1,), 0.25), torch.full((1,), 2.0)
    v_ = torch.sigmoid(b_ + g_ * oops.disparity_variance(prob, m4, want0.unsqueeze(1)))
    rw, lb = oops.SpatialTransformer_grid(fl4, fr4, oops.propagation(want0.unsqueeze(1)))
    st_want = torch.softmax((lb * rw).mean(dim=1) * oops.propagation(v_), dim=1)
    st = sa.ops.sample_strength(dev(fl4), dev(fr4), dev(want0), dev(oops.disparity_variance(prob, m4, want0.unsqueeze(1))), dev(g_), dev(b_))
    check("md48/strength", st, st_want, 2e-6)
    aw = (oops.propagation_prob(up) * st_want.unsqueeze(2)).sum(dim=1, keepdim=True)
    awp = F.softmax(aw, dim=2)
    ind_k = awp.sort(dim=2, descending=True, stable=True)[1][:, :, :6].sort(2, False)[0]
    att, smp, pa = sa.ops.topk_candidates(dev(up), dev(st_want), m4, 6)           # 6 of 24 planes (the 24-candidate kernels need D4 >= 24)
    assert torch.equal(smp.cpu(), ind_k.squeeze(1).float() - m4)
    check("md48/att_topk", att, torch.gather(awp, 2, ind_k), 1e-6)
    cost = dd.t_normalish((1, 6, H4, H4), 885)
    check("md48/regression_topk", sa.ops.regression_topk(dev(cost), smp, 2), oops.regression_topk(cost, smp.cpu(), 2), 1e-5)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", sorted(cases.SEGMENT_WHU))
def test_hot_segment_whu_vs_reference_fixture(sa, golden, name, fused, deferral_on):
    """HotSegment(unsigned=True) = models/SemStereo_WHU.py:273-323 on the unsigned op set (fixture: the reference's own
    SemStereo_WHU with models/submodule_.py's definitions bound in its globals), fused kernels and line-by-line form."""
    B, H, W, maxdisp = cases.segment_shape(name)
    seg = sa.HotSegment(maxdisp, unsigned=True)
    P = oseg.deterministic_params()
    seg.load_state_dict(P, strict=False)
    seg = seg.cuda().eval()
    seg.FUSED = fused
    fl4, fr4, fl8, fr8, _ = cases.segment_inputs(name)
    from semstereo_amd import deferred as dfr
    dfr.STATS["fused"].clear()
    with torch.no_grad():
        r = seg(dev(fl4), dev(fr4), dev(fl8), dev(fr8))
    if not fused:
        # the statement-by-statement form: the deferred handles recognise the WHU variant's text too (:279 maxdisp//4 planes,
        # :305 no offset -> candidates are the plane indices) and run the same fused kernels on the unsigned ranges
        assert set(dfr.STATS["fused"]) == ({"gwc_patch_gate", "upsample_softmax_regression", "sample_strength", "topk_candidates", "stem_by_halves"}
                                           | ({"concat_feature_pair"} if sa.engine._conv2d_hip_on() else set())), dfr.STATS
    g = golden["segment_whu"]
    assert float(r["samples"].min()) >= 0 and float(r["samples"].max()) < maxdisp // 4
    check(f"whu/{name}/{fused}/pred_att0", r["pred_att0"], g[f"{name}/pred_att0"], 1e-3)
    _explained_deviation_check(f"whu/{name}/{fused}", r, g, name)
