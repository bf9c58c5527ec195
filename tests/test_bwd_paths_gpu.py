"""Every shape-dependent path of the training backward kernels of the attention tail and the cost volume, at the smallest shapes that
reach it (tests/bwd_path_cases.py; the properties are checked on the CPU by tests/test_bwd_path_cases.py), against the float64
references of tests/train_calls.py under CPU autograd, to the bounds train_calls.BOUNDS holds the same seams to at full size:

  * the probe's backward in BOTH forms (train.SSB_TWO_LAUNCHES off: sample_strength_bwd_kernel; on: ssb_dcorr_kernel + ssb_scatter_kernel):
    the row buffers (W % 64 == 0) with the second row above / below, 64 lanes on one slot, taps beyond the +-64-column window, the image
    borders, an odd channel count, a partial last block, and each subset of requested gradients (NULL outputs);
  * ss_gwc_volume_bwd's thread-per-element kernel (Cg > 8, more than 64 KiB of LDS, more than 48 planes) and the row-staged kernel on
    mostly empty planes, and the two kernels against each other bit for bit;
  * ss_group_normalise_bwd on groups whose channels are all zero;
  * ss_topk_candidates_bwd at k == D, H = 2, W = 1, and with either incoming gradient NULL;
  * ss_upsample_softmax_regression_bwd on a coarse axis of length one, and with each incoming gradient NULL.

Error = max|hip - ref64| / max|ref64| per tensor.  The figures of a run go to train_calls.report_path() under "bwd_paths"."""
import pytest
import torch
import torch.nn.functional as F

import bwd_path_cases as BP
import train_calls as TC
from golden import cases
from oracle import ops as oops

pytestmark = pytest.mark.gpu

REPORT = {}
FORMS = pytest.mark.parametrize("two_launches", [False, True], ids=["one_launch", "two_launches"])
GRAD_NAMES = ("left", "right", "pred0", "var", "gamma", "beta")


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    return semstereo_amd


@pytest.fixture(autouse=True)
def _fp32_accurate_engines(sa):
    if sa.modules.CONV_ENGINE == "bf16x3":
        pytest.skip("SS_CONV_ENGINE=bf16x3: these bounds are for the fp32-accurate engines")


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    if REPORT:
        TC.write_report("bwd_paths", REPORT)


def _rel(a, ref):
    a, ref = a.detach(), ref.detach()
    return float((a.double().cpu() - ref.double().cpu()).abs().max()) / (float(ref.double().abs().max()) + 1e-30)


def _hold(key, a, ref, bound):
    """Record, print, then assert one tensor's error against its seam's bound."""
    assert a.shape == ref.shape, (key, tuple(a.shape), tuple(ref.shape))
    e = _rel(a, ref)
    REPORT[key] = e
    print(f"{key}: {e:.3e} (bound {bound:.1e}, max|ref| {float(ref.abs().max()):.3e})")
    assert bool(torch.isfinite(a).all()), key
    assert e <= bound, (key, e, bound)


# ---- the probe ------------------------------------------------------------------------------------------------------------------------

_STRENGTH_REF = {}


def _strength_ref(name):
    """(inputs, grad_strength, float64 strength, float64 gradients of the six inputs) -- computed once per case, shared, never modified."""
    if name not in _STRENGTH_REF:
        ins, go, _ = BP.strength_case(name)
        xs = [t.double().clone().requires_grad_(True) for t in ins]
        out = TC.strength_ref(*xs)
        grads = torch.autograd.grad(out, xs, go.double())
        _STRENGTH_REF[name] = (ins, go, out.detach(), tuple(g.detach() for g in grads))
    return _STRENGTH_REF[name]


def _strength_hip(sa, ins, go, wanted):
    hin = [t.cuda().requires_grad_(i in wanted) for i, t in enumerate(ins)]
    st = sa.train._SampleStrength.apply(*hin)
    grads = torch.autograd.grad(st, [hin[i] for i in wanted], go.cuda())
    torch.cuda.synchronize()
    return st.detach(), dict(zip(wanted, grads))


@FORMS
@pytest.mark.parametrize("name", sorted(BP.STRENGTH_CASES))
def test_sample_strength_backward_on_every_path(sa, monkeypatch, name, two_launches):
    """All six gradients of each case of bwd_path_cases.STRENGTH_CASES, in the one-launch and in the two-launch form; in rows_below and
    rows_above also the one row of grad_right that nothing but the second row's taps reaches, on its own scale (the second row buffer of
    ssb_scatter_kernel: beside the main taps its sums are ~1e-7 of the tensor, and dropping them all passed every other check)."""
    monkeypatch.setattr(sa.train, "SSB_TWO_LAUNCHES", two_launches)
    ins, go, out_ref, g_ref = _strength_ref(name)
    tag = f"strength/{name}/{'two' if two_launches else 'one'}"
    st, grads = _strength_hip(sa, ins, go, tuple(range(6)))
    bound = TC.BOUNDS["train._SampleStrength"]
    _hold(f"{tag}/fwd", st, out_ref, bound["fwd"])
    for i, n in enumerate(GRAD_NAMES):
        _hold(f"{tag}/grad_{n}", grads[i], g_ref[i], bound["bwd"])
    if name in BP.SECOND_ROW_ONLY:       # the row of grad_right that only the second-row taps (weights ~1e-7) reach, on its own scale
        r = BP.SECOND_ROW_ONLY[name]
        _hold(f"{tag}/grad_right/second_row_only", grads[1][:, :, r], g_ref[1][:, :, r], bound["bwd"])


@FORMS
@pytest.mark.parametrize("wanted", [(0,), (2, 3, 4, 5), (1,)], ids=["left", "pred0_var_gamma_beta", "right"])
def test_sample_strength_backward_on_subsets_of_the_gradients(sa, monkeypatch, wanted, two_launches):
    """rows_below with gradients requested for `left` alone, for everything but the features (grad_left and grad_right NULL: no row
    buffer), and for `right` alone: the requested ones hold the same bound; autograd.grad of an input that does not require one raises,
    so `None` is checked on the Function's own return."""
    monkeypatch.setattr(sa.train, "SSB_TWO_LAUNCHES", two_launches)
    ins, go, _, g_ref = _strength_ref("rows_below")
    returned = {}
    real = sa.train._SampleStrength.backward

    def backward(ctx, g):
        res = real(ctx, g)
        returned["grads"] = res
        return res
    monkeypatch.setattr(sa.train._SampleStrength, "backward", staticmethod(backward))
    _, grads = _strength_hip(sa, ins, go, wanted)
    tag = f"strength/subsets/{'+'.join(GRAD_NAMES[i] for i in wanted)}/{'two' if two_launches else 'one'}"
    for i in wanted:
        _hold(f"{tag}/grad_{GRAD_NAMES[i]}", grads[i], g_ref[i], TC.BOUNDS["train._SampleStrength"]["bwd"])
    if 1 in wanted:
        r = BP.SECOND_ROW_ONLY["rows_below"]
        _hold(f"{tag}/grad_right/second_row_only", grads[1][:, :, r], g_ref[1][:, :, r], TC.BOUNDS["train._SampleStrength"]["bwd"])
    assert len(returned["grads"]) == 6
    for i in range(6):
        assert (returned["grads"][i] is None) == (i not in wanted), (GRAD_NAMES[i], wanted)


# ---- the group-wise correlation volume -------------------------------------------------------------------------------------------------

def _gwc_fn(sa, signed, norm):
    lib = sa.ops if signed else sa.ops_unsigned
    return lib.build_gwc_volume_norm if norm else lib.build_gwc_volume


def _gwc_hip(sa, ref, tgt, G, maxdisp, signed, norm, go):
    r, t = ref.cuda().requires_grad_(True), tgt.cuda().requires_grad_(True)
    vol = _gwc_fn(sa, signed, norm)(r, t, maxdisp, G)
    gr, gt = torch.autograd.grad(vol, (r, t), go.cuda())
    torch.cuda.synchronize()
    return vol.detach(), gr, gt


def _gwc_ref64(ref, tgt, G, rng, norm, go):
    r, t = ref.double().requires_grad_(True), tgt.double().requires_grad_(True)
    vol = TC.gwc_ref(TC.group_normalise_ref(r, G), TC.group_normalise_ref(t, G), rng, G) if norm else TC.gwc_ref(r, t, rng, G)
    gr, gt = torch.autograd.grad(vol, (r, t), go.double())
    return vol.detach(), gr, gt


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("name", ["generic_cg12", "generic_lds", "generic_d50", "rows_wide_d"])
def test_gwc_volume_backward_on_both_kernels(sa, name, norm):
    """build_gwc_volume (and the normalised form: _GroupNormalise, then the same volume kernels) under autograd where ss_gwc_volume_bwd
    takes the thread-per-element kernel, and the row-staged kernel on planes with |d| >= W.  The normalised form is held to the looser of
    its two seams' forward bounds (_GroupNormalise's)."""
    ref, tgt, G, maxdisp, signed, go, p = BP.gwc_case(name)
    vol, gr, gt = _gwc_hip(sa, ref, tgt, G, maxdisp, signed, norm, go)
    vol64, gr64, gt64 = _gwc_ref64(ref, tgt, G, p["range"], norm, go)
    b = TC.BOUNDS["ops._GwcVolume"]
    fwd = max(b["fwd"], TC.BOUNDS["ops._GroupNormalise"]["fwd"]) if norm else b["fwd"]
    tag = f"gwc/{name}/{'norm' if norm else 'plain'}"
    _hold(f"{tag}/fwd", vol, vol64, fwd)
    _hold(f"{tag}/grad_ref", gr, gr64, b["bwd"])
    _hold(f"{tag}/grad_tgt", gt, gt64, b["bwd"])


def test_gwc_volume_backward_kernels_form_the_same_sums(sa):
    """One pair on the row-staged kernel (Cg = 8), then as part of wider calls that take the thread-per-element kernel: every group's
    channels repeated r times (Cg = 8 r) with the incoming gradient scaled by r is the same operation -- each copy's gradient is the
    narrow call's.  r = 3: 3a / 24 is not a / 8 bit for bit, so both are held to float64.  r = 2: the scaling is by a power of two, every
    product, every partial sum (d ascending in both kernels) and the quotient by 2 Cg are exactly those of the narrow call, so the two
    kernels must agree BIT FOR BIT -- the claim of gwc_volume.hip that both form the same sums in the same order."""
    ref, tgt, G, maxdisp, signed, go, p = BP.gwc_case("same_sums")
    b = TC.BOUNDS["ops._GwcVolume"]
    vol, gr, gt = _gwc_hip(sa, ref, tgt, G, maxdisp, signed, False, go)
    vol64, gr64, gt64 = _gwc_ref64(ref, tgt, G, p["range"], False, go)
    _hold("gwc/same_sums/rows/fwd", vol, vol64, b["fwd"])
    _hold("gwc/same_sums/rows/grad_ref", gr, gr64, b["bwd"])
    _hold("gwc/same_sums/rows/grad_tgt", gt, gt64, b["bwd"])
    assert float(gr64.abs().max()) > 0 and float(gt64.abs().max()) > 0
    for r in (3, 2):
        volw, grw, gtw = _gwc_hip(sa, BP.widen_groups(ref, G, r), BP.widen_groups(tgt, G, r), G, maxdisp, signed, False, go * float(r))
        _hold(f"gwc/same_sums/x{r}/fwd", volw, vol64, b["fwd"])
        for copy in range(r):
            a_ref, a_tgt = (BP.narrow_groups(t, G, r)[:, :, copy].reshape(ref.shape) for t in (grw, gtw))
            _hold(f"gwc/same_sums/x{r}/copy{copy}/grad_ref", a_ref, gr64, b["bwd"])
            _hold(f"gwc/same_sums/x{r}/copy{copy}/grad_tgt", a_tgt, gt64, b["bwd"])
            if r == 2:
                assert torch.equal(a_ref, gr) and torch.equal(a_tgt, gt), "the two backward kernels of the volume differ in their sums"


# ---- the group normalisation ------------------------------------------------------------------------------------------------------------

def test_group_normalise_on_all_zero_groups(sa):
    """Groups whose channels are all zero at a pixel (features behind a ReLU): y = 0 and grad_x = grad_y / eps there (the kernel's
    n == 0 branch; torch's norm backward gives 0 for the second term).  Those gradients are 1e5 times the others, so the rest of the
    tensor is held to the bound on its own scale too."""
    x, G, gy, zero = BP.group_normalise_case()
    xh = x.cuda().requires_grad_(True)
    y = sa.ops._group_normalise(xh, G)
    assert y.grad_fn is not None and type(y.grad_fn).__name__.startswith("_GroupNormalise")
    (gx,) = torch.autograd.grad(y, xh, gy.cuda())
    torch.cuda.synchronize()
    x64 = x.double().requires_grad_(True)
    y64 = TC.group_normalise_ref(x64, G)
    (gx64,) = torch.autograd.grad(y64, x64, gy.double())
    assert bool(torch.isfinite(y64).all()) and bool(torch.isfinite(gx64).all())
    b = TC.BOUNDS["ops._GroupNormalise"]
    _hold("group_normalise/fwd", y, y64.detach(), b["fwd"])
    _hold("group_normalise/grad_x", gx, gx64, b["bwd"])
    _hold("group_normalise/grad_x/zero_groups", gx.cpu()[zero], gx64[zero], b["bwd"])
    _hold("group_normalise/grad_x/other_groups", gx.cpu()[~zero], gx64[~zero], b["bwd"])
    assert bool((y.cpu()[zero] == 0).all())


# ---- the top-k candidates -----------------------------------------------------------------------------------------------------------------

def _topk_forward(sa, shape):
    logits, strength, k, rng, ga, gp, _ = BP.topk_case(shape)
    lh, sh = logits.cuda().requires_grad_(True), strength.cuda().requires_grad_(True)
    att, samples, pred = sa.train._TopkCandidates.apply(lh, sh, k, rng)
    return (logits, strength, k, rng, ga, gp), (lh, sh), (att, samples, pred)


@pytest.mark.parametrize("shape", BP.TOPK_CASES, ids=lambda s: "x".join(map(str, s)))
def test_topk_candidates_backward_at_wide_d_and_thin_maps(sa, shape):
    """D = 48 / k = 24 on two rows, k == D on one column, k == D at batch 2: forward and both gradients against topk_ref on the HIP
    picks; a pixel whose float64 picks differ is allowed only where the k-th and (k+1)-th probabilities are within cases.DELTA24_REL."""
    (logits, strength, k, rng, ga, gp), (lh, sh), (att, samples, pred) = _topk_forward(sa, shape)
    gl, gs = torch.autograd.grad([att, pred], [lh, sh], [ga.cuda(), gp.cuda()])
    torch.cuda.synchronize()
    lr, sr = logits.double().requires_grad_(True), strength.double().requires_grad_(True)
    att_r, pred_r, own, gap = TC.topk_ref(lr, sr, k, rng, samples.detach().cpu())
    other = (own != samples.detach().cpu().to(torch.int64)).any(dim=1)
    assert not bool((other & (gap >= cases.DELTA24_REL)).any()), int(other.sum())
    glr, gsr = torch.autograd.grad([att_r, pred_r], [lr, sr], [ga.double(), gp.double()])
    b = TC.BOUNDS["train._TopkCandidates"]
    tag = "topk/" + "x".join(map(str, shape))
    _hold(f"{tag}/att_topk", att, att_r.detach(), b["fwd"])
    _hold(f"{tag}/pred_att", pred, pred_r.detach(), b["fwd"])
    _hold(f"{tag}/grad_logits", gl, glr, b["bwd"])
    _hold(f"{tag}/grad_strength", gs, gsr, b["bwd"])


@pytest.mark.parametrize("null", ["grad_att_topk", "grad_pred_att"])
def test_topk_candidates_backward_with_a_null_gradient(sa, null):
    """ss_topk_candidates_bwd with one incoming gradient NULL against the same call on a tensor of zeros (the scattered grad_logits goes
    through atomics: 1e-6, not bit equality)."""
    call, ptr = sa._lib.call, sa._lib.ptr
    shape = BP.TOPK_CASES[2]
    (logits, strength, k, rng, ga, gp), (lh, sh), (_att, samples, _pred) = _topk_forward(sa, shape)
    B, D, H, W, _ = shape
    lg, st, smp, ga, gp = lh.detach(), sh.detach(), samples.detach(), ga.cuda(), gp.cuda()
    got = []
    for form in ("null", "zeros"):
        a = ga if null != "grad_att_topk" else (None if form == "null" else torch.zeros_like(ga))
        p = gp if null != "grad_pred_att" else (None if form == "null" else torch.zeros_like(gp))
        gl, gs = torch.full_like(lg, float("nan")), torch.full_like(st, float("nan"))
        call("ss_topk_candidates_bwd", ptr(lg), ptr(st), ptr(smp), ptr(a), ptr(p), ptr(gl), ptr(gs), B, rng[0], D, H, W, k)
        torch.cuda.synchronize()
        got.append((gl, gs))
    assert float(got[1][0].abs().max()) > 0 and float(got[1][1].abs().max()) > 0
    _hold(f"topk/null_{null}/grad_logits", got[0][0], got[1][0], 1e-6)
    _hold(f"topk/null_{null}/grad_strength", got[0][1], got[1][1], 1e-6)


# ---- the up-sampling soft-argmax ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", BP.UPSOFT_CASES, ids=lambda s: "x".join(map(str, s)))
def test_upsample_softmax_regression_backward_on_a_coarse_axis_of_one(sa, shape):
    """A coarse axis of length 1 (H, W, D in turn): both edge folds of the transposed up-sampling land on the same voxel."""
    coarse, H, W, rng, (g_up, g_disp, g_var) = BP.upsoft_case(shape)
    m = rng[1] // 2
    assert sa.ops.upsample_softmax_regression_applies(coarse.cuda(), m, H, W, _range=rng)
    ch = coarse.cuda().requires_grad_(True)
    up, disp, var = sa.train._UpsampleSoftmaxRegression.apply(ch, H, W, rng)
    (gc,) = torch.autograd.grad([up, disp, var], [ch], [g_up.cuda(), g_disp.cuda(), g_var.cuda()])
    torch.cuda.synchronize()
    cr = coarse.double().requires_grad_(True)
    upr = F.interpolate(cr, [rng[1], H, W], mode="trilinear")
    pr = F.softmax(upr.squeeze(1), dim=1)
    dispr = oops.disparity_regression(pr, m)
    varr = oops.disparity_variance(pr, m, dispr.unsqueeze(1))
    (gcr,) = torch.autograd.grad([upr, dispr, varr], [cr], [g_up.double(), g_disp.double(), g_var.double()])
    b = TC.BOUNDS["train._UpsampleSoftmaxRegression"]
    tag = "upsoft/" + "x".join(map(str, shape))
    _hold(f"{tag}/up", up, upr.detach(), b["fwd"])
    _hold(f"{tag}/disp", disp, dispr.detach(), b["fwd"])
    _hold(f"{tag}/var", var, varr.detach(), b["fwd"])
    _hold(f"{tag}/grad_coarse", gc, gcr, b["bwd"])


@pytest.mark.parametrize("null", [0, 1, 2], ids=["grad_up", "grad_disp", "grad_var"])
def test_upsample_softmax_regression_backward_with_a_null_gradient(sa, null):
    """ss_upsample_softmax_regression_bwd with one incoming gradient NULL is bit for bit the call on a tensor of zeros (no atomics in
    these two kernels)."""
    call, ptr = sa._lib.call, sa._lib.ptr
    coarse, H, W, rng, grads = BP.upsoft_case(BP.UPSOFT_CASES[0])
    B = coarse.shape[0]
    up, _, _ = sa.ops.upsample_softmax_regression(coarse.cuda(), rng[1] // 2, H, W, _range=rng)
    grads = [g.cuda() for g in grads]
    got = []
    for form in ("null", "zeros"):
        g = [(None if form == "null" else torch.zeros_like(t)) if i == null else t for i, t in enumerate(grads)]
        gc, work = torch.full_like(coarse.cuda(), float("nan")), torch.empty_like(up)
        call("ss_upsample_softmax_regression_bwd", ptr(up), ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(gc), ptr(work), B, rng[0], rng[1], H, W)
        torch.cuda.synchronize()
        got.append(gc)
    assert bool(torch.isfinite(got[1]).all()) and float(got[1].abs().max()) > 0
    assert torch.equal(got[0], got[1])
