"""Every path of the fp32 per-channel training kernels at the smallest shape that reaches it (tests/train_ops_cases.py; the properties of
the cases and the references are checked on the CPU by tests/test_train_ops_cases.py): the BatchNorm statistics, apply and backward
kernels of csrc/train_ops.hip in their scalar and 16-byte forms, ss_channel_sum_fwd, the depthwise `patch` weight gradient, the gate's
logits gradient, and conv_wgrad_k1 of csrc/conv3d_wgrad.hip.  The entry points are called through `_lib.call` with explicit pointers, so
that NULL arguments and the alignment of every tensor are the test's choice; which form a call reaches is asserted from the host rules
restated in train_ops_cases on the device pointers, never by looking at a kernel.

  a. paths: every case x relu x residual x weight x bias x batch / running statistics x y given / NULL x float gradients given / NULL,
     and the four older entry points, against float64 under CPU autograd (the ReLU mask decided like for like from the HIP forward's
     y > 0; a float64 pre-activation on the other side of zero is counted and allowed only within the seam's bound of zero) to
     train_calls.BOUNDS["train._BatchNormTrain"], error = max|hip - ref64| / max|ref64|;
  b. bit relations read from the code (torch.equal);
  c. the module bookkeeping of train.batchnorm_train (momentum=None, track_running_stats=False, affine=False) against nn.BatchNorm3d in
     float64 on the CPU;
  d. ranges: channels drawn as (normal + off) * scale, off up to 1000 standard deviations, scale 1e-3 .. 1e3, and a constant channel,
     against float64 with the same reference in float32 on the CPU as the yardstick;
  e. the neighbours, each against float64 to its own seam's bound.

Every figure is printed before anything is asserted; SS_TRAIN_OPS_ERR_OUT=<file> keeps the table (profiles/train_ops_paths_err.txt holds
a copy of one run)."""
import itertools
import os

import pytest
import torch
import torch.nn as nn

import train_calls as TC
import train_ops_cases as OC

pytestmark = pytest.mark.gpu

BOUND = TC.BOUNDS["train._BatchNormTrain"]
_TABLE = []


def _line(text):
    print(text)
    _TABLE.append(text)


@pytest.fixture(scope="module", autouse=True)
def _dump_table():
    yield
    path = os.environ.get("SS_TRAIN_OPS_ERR_OUT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(_TABLE) + "\n")


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    return semstereo_amd


def _rel(a, ref):
    return float((a.detach().double().cpu() - ref.detach().double().cpu()).abs().max()) / (float(ref.detach().double().abs().max()) + 1e-300)


class _Worst:
    """The worst error per kind of tensor over the configurations of one test: recorded per call, printed and asserted at the end."""

    def __init__(self, tag):
        self.tag, self.worst, self.bad = tag, {}, []

    def hold(self, kind, config, a, ref, bound):
        assert a.shape == ref.shape, (self.tag, kind, config, tuple(a.shape), tuple(ref.shape))
        e = _rel(a, ref) if bool(torch.isfinite(a).all()) else float("inf")
        if kind not in self.worst or e > self.worst[kind][0]:
            self.worst[kind] = (e, config, bound, float(ref.detach().abs().max()))
        if not e <= bound:
            self.bad.append((kind, config, e, bound))

    def finish(self):
        for kind, (e, config, bound, scale) in sorted(self.worst.items()):
            _line(f"{self.tag + '/' + kind:58s} worst {e:.3e} (bound {bound:.1e}, max|ref| {scale:.3e}) at {config}")
        assert not self.bad, self.bad[:8]


# ---- device tensors whose alignment is the test's choice -------------------------------------------------------------------------------

def _place(t, off=0):
    """`t` on the device as a contiguous view `off` floats into a fresh buffer (the allocator's blocks are 16-byte aligned)."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * off) % 16
    return v


def _blank(shape, off=0, dtype=torch.float32):
    """An output of `shape` filled with NaN, so that an element the kernel leaves out shows."""
    return _place(torch.full(tuple(shape), float("nan"), dtype=dtype), off)


def _dev(case_tensors, off, names):
    return {n: _place(case_tensors[n], off.get(n, 0)) for n in names}


def _ptr(t):
    return None if t is None else t.data_ptr()


def _dims(x):
    return x.shape[0], x.shape[1], x[0, 0].numel()


def _fwd(sa, entry, x, residual, weight, bias, relu, off_y=0, stats=None):
    """One forward entry point -> dict(y, mean, invstd, var_unbiased, work).  entry: "rs" (ss_batchnorm_train_fwd_rs, no running
    statistics), "fwd" / "res_fwd" (the older two), "eval" (ss_batchnorm_eval_fwd on `stats` = (mean, invstd))."""
    call = sa._lib.call
    B, C, N = _dims(x)
    y = _blank(x.shape, off_y)
    if entry == "eval":
        call("ss_batchnorm_eval_fwd", _ptr(x), _ptr(residual), _ptr(stats[0]), _ptr(stats[1]), _ptr(weight), _ptr(bias), _ptr(y), B, C, N, int(relu))
        torch.cuda.synchronize()
        return {"y": y, "mean": stats[0], "invstd": stats[1]}
    mean, invstd, var_u, work = _blank((C,)), _blank((C,)), _blank((C,)), _blank((2 * C,), dtype=torch.float64)
    if entry == "rs":
        call("ss_batchnorm_train_fwd_rs", _ptr(x), _ptr(residual), _ptr(weight), _ptr(bias), _ptr(y), _ptr(mean), _ptr(invstd), _ptr(var_u),
             _ptr(work), None, None, None, 0.0, B, C, N, OC.EPS, int(relu))
    elif entry == "fwd":
        assert residual is None
        call("ss_batchnorm_train_fwd", _ptr(x), _ptr(weight), _ptr(bias), _ptr(y), _ptr(mean), _ptr(invstd), _ptr(var_u), _ptr(work), B, C, N,
             OC.EPS, int(relu))
    else:
        call("ss_batchnorm_train_res_fwd", _ptr(x), _ptr(residual), _ptr(weight), _ptr(bias), _ptr(y), _ptr(mean), _ptr(invstd), _ptr(var_u),
             _ptr(work), B, C, N, OC.EPS, int(relu))
    torch.cuda.synchronize()
    return {"y": y, "mean": mean, "invstd": invstd, "var_unbiased": var_u, "work": work}


def _bwd(sa, entry, g, x, y, mean, invstd, weight, bias, relu, want_res, off_gx=0, off_gres=0, want_gw=True, want_gb=True, batch_statistics=True):
    """One backward entry point -> dict(grad_x, grad_residual, work, grad_weight, grad_bias).  entry: "pg" (ss_batchnorm_bwd_pg), "bwd" /
    "res_bwd" (the older two), "eval" (ss_batchnorm_eval_bwd)."""
    call = sa._lib.call
    B, C, N = _dims(x)
    gx = _blank(x.shape, off_gx)
    gres = _blank(x.shape, off_gres) if want_res else None
    work = _blank((2 * C,), dtype=torch.float64)
    gw = _blank((C,)) if (entry == "pg" and want_gw) else None
    gb = _blank((C,)) if (entry == "pg" and want_gb) else None
    if entry == "pg":
        call("ss_batchnorm_bwd_pg", _ptr(g), _ptr(x), _ptr(y), _ptr(mean), _ptr(invstd), _ptr(weight), _ptr(bias), _ptr(gx), _ptr(gres), _ptr(work),
             _ptr(gw), _ptr(gb), int(batch_statistics), B, C, N, int(relu))
    elif entry == "bwd":
        assert not want_res
        call("ss_batchnorm_train_bwd", _ptr(g), _ptr(x), _ptr(y), _ptr(mean), _ptr(invstd), _ptr(weight), _ptr(gx), _ptr(work), B, C, N, int(relu))
    elif entry == "res_bwd":
        call("ss_batchnorm_train_res_bwd", _ptr(g), _ptr(x), _ptr(y), _ptr(mean), _ptr(invstd), _ptr(weight), _ptr(gx), _ptr(gres), _ptr(work), B, C, N,
             int(relu))
    else:
        call("ss_batchnorm_eval_bwd", _ptr(g), _ptr(x), _ptr(y), _ptr(mean), _ptr(invstd), _ptr(weight), _ptr(gx), _ptr(gres), _ptr(work), B, C, N,
             int(relu))
    torch.cuda.synchronize()
    return {"grad_x": gx, "grad_residual": gres, "work": work, "grad_weight": gw, "grad_bias": gb}


def _forms_on_device(N, tensors):
    """The restated rules on the device pointers of {name: tensor or None}."""
    return OC.expected_forms(N, {t: (0 if tensors.get(t) is None else tensors[t].data_ptr()) for t in OC.ALL_TENSORS})


def _flips(z64, y_hip, bound):
    """(elements whose float64 pre-activation lies on the other side of zero from the HIP y > 0, those beyond `bound` of the tensor)."""
    flip = (z64 > 0) != (y_hip.cpu() > 0)
    return int(flip.sum()), int((flip & (z64.abs() > bound * float(z64.abs().max()))).sum())


def _hold_backward(W, config, got, ref, residual, count_scale=1.0):
    W.hold("grad_x", config, got["grad_x"], ref["grad_x"], BOUND["bwd"])
    if residual:
        W.hold("grad_residual", config, got["grad_residual"], ref["grad_residual"], BOUND["bwd"])
    # work[2c] = sum g', work[2c + 1] = sum g' xhat as doubles; their float copies where asked for
    W.hold("work/sum_g", config, got["work"][0::2], ref["grad_bias"], BOUND["bwd"])
    W.hold("work/sum_g_xhat", config, got["work"][1::2], ref["grad_weight"], BOUND["bwd"])
    if got["grad_bias"] is not None:
        W.hold("grad_bias", config, got["grad_bias"], ref["grad_bias"], BOUND["bwd"])
    if got["grad_weight"] is not None:
        W.hold("grad_weight", config, got["grad_weight"], ref["grad_weight"], BOUND["bwd"])


#: (float grad_weight, float grad_bias) given: both and neither everywhere, one of the two where both affine terms exist
def _float_gradient_choices(weight, bias):
    return [(True, True), (False, False)] + ([(True, False), (False, True)] if (weight and bias) else [])


# ---- a. paths ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(OC.BN_CASES))
def test_batchnorm_paths_against_float64(sa, name):
    """Every configuration of the case through ss_batchnorm_train_fwd_rs / ss_batchnorm_bwd_pg(batch_statistics = 1) and through
    ss_batchnorm_eval_fwd / ss_batchnorm_bwd_pg(0) / ss_batchnorm_eval_bwd.  Inputs of mean 0.3 / std 2.  Measured: see
    profiles/train_ops_paths_err.txt."""
    t = OC.bn_case(name)
    B, C, spatial, N = OC.bn_shape(name)
    W = _Worst(f"bn/{name}")
    flips, unexplained = 0, 0
    for relu, residual, weight, bias in itertools.product((True, False), repeat=4):
        config = f"relu{int(relu)} res{int(residual)} w{int(weight)} b{int(bias)}"
        off = OC.offsets(name, residual)
        d = _dev(t, off, ["x", "grad_y"] + (["residual"] if residual else []))
        w = _place(t["weight"]) if weight else None
        b = _place(t["bias"]) if bias else None
        res = d.get("residual")
        want_forms = OC.expected_forms(N, OC.addresses(off, {"residual": residual, "grad_residual": residual}))
        for batch_statistics in (True, False):
            stats = None
            if batch_statistics:
                f = _fwd(sa, "rs", d["x"], res, w, b, relu, off["y"])
            else:
                stats = (_place(t["run_mean"]), _place(torch.rsqrt(t["run_var"] + OC.EPS)))
                f = _fwd(sa, "eval", d["x"], res, w, b, relu, off["y"], stats)
            mask = (f["y"] > 0).cpu() if relu else None
            ref = OC.bn_reference(t, torch.float64, relu, residual, weight, bias, batch_statistics, mask,
                                  None if stats is None else (stats[0].cpu(), stats[1].cpu()))
            kind = "train" if batch_statistics else "eval"
            if relu:
                n_flip, n_bad = _flips(ref["z"], f["y"], BOUND["fwd"])
                flips, unexplained = flips + n_flip, unexplained + n_bad
            W.hold(f"{kind}/y", config, f["y"], ref["y"], BOUND["fwd"])
            if batch_statistics:
                W.hold("train/mean", config, f["mean"], ref["mean"], BOUND["fwd"])
                W.hold("train/var_unbiased", config, f["var_unbiased"], ref["var_unbiased"], BOUND["fwd"])
                var_b = ref["var_unbiased"] * (B * N - 1) / (B * N) if B * N > 1 else ref["var_unbiased"]
                W.hold("train/invstd", config, f["invstd"], 1.0 / torch.sqrt(var_b + OC.EPS), BOUND["fwd"])
                W.hold("train/work/sum_x", config, f["work"][0::2], ref["sum_x"], BOUND["fwd"])
                W.hold("train/work/sum_xx", config, f["work"][1::2], ref["sum_xx"], BOUND["fwd"])
            for y_given in (True, False):
                if not y_given and relu and residual:
                    continue                                    # (the mask cannot be recomputed from x behind a residual)
                y = f["y"] if y_given else None
                for want_gw, want_gb in _float_gradient_choices(weight, bias):
                    got = _bwd(sa, "pg", d["grad_y"], d["x"], y, f["mean"], f["invstd"], w, b, relu, residual, off["grad_x"], off["grad_residual"],
                               want_gw, want_gb, batch_statistics)
                    tensors = {"x": d["x"], "residual": res, "y": y, "grad_y": d["grad_y"], "grad_x": got["grad_x"], "grad_residual": got["grad_residual"]}
                    assert d["x"].data_ptr() % 16 == 4 * off["x"] and got["grad_x"].data_ptr() % 16 == 4 * off["grad_x"]
                    have = _forms_on_device(N, dict(tensors, y=f["y"]))[:2] + _forms_on_device(N, tensors)[2:]
                    assert have == want_forms, (name, config, have, want_forms)
                    _hold_backward(W, f"{config} {kind} y{int(y_given)} gw{int(want_gw)} gb{int(want_gb)}", got, ref, residual)
            if not batch_statistics:
                got = _bwd(sa, "eval", d["grad_y"], d["x"], f["y"], f["mean"], f["invstd"], w, None, relu, residual, off["grad_x"], off["grad_residual"])
                _hold_backward(W, f"{config} ss_batchnorm_eval_bwd", got, ref, residual)
    _line(f"bn/{name}: {flips} float64 pre-activations on the other side of zero, {unexplained} of them beyond {BOUND['fwd']:.0e} of the tensor")
    W.finish()
    assert unexplained == 0, unexplained


@pytest.mark.parametrize("name", ["scalar_105", "vector_1280"])
def test_older_batchnorm_entry_points(sa, name):
    """ss_batchnorm_train_fwd / _bwd and ss_batchnorm_train_res_fwd / _res_bwd, once each on a scalar and a vector case."""
    t = OC.bn_case(name)
    W = _Worst(f"bn_older/{name}")
    d = _dev(t, {}, ["x", "grad_y", "residual"])
    w, b = _place(t["weight"]), _place(t["bias"])
    for residual in (False, True):
        res = d["residual"] if residual else None
        f = _fwd(sa, "res_fwd" if residual else "fwd", d["x"], res, w, b, True)
        ref = OC.bn_reference(t, torch.float64, True, residual, True, True, True, (f["y"] > 0).cpu())
        assert _flips(ref["z"], f["y"], BOUND["fwd"])[1] == 0
        config = "res" if residual else "plain"
        for k in ("y", "mean", "var_unbiased"):
            W.hold(k, config, f[k], ref[k], BOUND["fwd"])
        got = _bwd(sa, "res_bwd" if residual else "bwd", d["grad_y"], d["x"], f["y"], f["mean"], f["invstd"], w, None, True, residual)
        _hold_backward(W, config, got, ref, residual)
    W.finish()


# ---- b. bit relations read from the code ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(OC.BN_CASES))
def test_batchnorm_bit_relations(sa, name):
    t = OC.bn_case(name)
    B, C, spatial, N = OC.bn_shape(name)
    off = OC.offsets(name)
    d = _dev(t, off, ["x", "grad_y", "residual"])
    w, b = _place(t["weight"]), _place(t["bias"])
    for relu, residual in itertools.product((True, False), repeat=2):
        res = d["residual"] if residual else None
        f = _fwd(sa, "rs", d["x"], res, w, b, relu, off["y"])
        # the eval forward on the training forward's own mean / invstd is the same apply kernel on the same numbers
        e = _fwd(sa, "eval", d["x"], res, w, b, relu, off["y"], (f["mean"], f["invstd"]))
        assert torch.equal(e["y"], f["y"]), (name, relu, residual)
        # ... and on an aligned and a misaligned copy of the same data (vector against scalar apply where N % 4 == 0)
        xa, xm = _place(t["x"], 0), _place(t["x"], 1)
        ra, rm_ = (_place(t["residual"], 0), _place(t["residual"], 1)) if residual else (None, None)
        ya = _fwd(sa, "eval", xa, ra, w, b, relu, 0, (f["mean"], f["invstd"]))["y"]
        ym = _fwd(sa, "eval", xm, rm_, w, b, relu, 1, (f["mean"], f["invstd"]))["y"]
        assert (N % 4 != 0) or (OC.vec4_ok(N, xa.data_ptr(), _ptr(ra), ya.data_ptr()) and not OC.vec4_ok(N, xm.data_ptr(), _ptr(rm_), ym.data_ptr()))
        assert torch.equal(ya, ym) and torch.equal(ya, f["y"]), (name, relu, residual)
        for batch_statistics in (True, False):
            got = _bwd(sa, "pg", d["grad_y"], d["x"], f["y"], f["mean"], f["invstd"], w, b, relu, residual, off["grad_x"], off["grad_residual"],
                       True, True, batch_statistics)
            if residual:
                keep = (f["y"] > 0).float() if relu else torch.ones_like(f["y"])
                assert torch.equal(got["grad_residual"], d["grad_y"] * keep), (name, relu, batch_statistics)
            assert torch.equal(got["grad_bias"], got["work"][0::2].float()) and torch.equal(got["grad_weight"], got["work"][1::2].float())
            if not residual and not batch_statistics:
                # running statistics: no sums in grad_x, so y given and the mask from x (the forward's own expression) agree bit for bit
                from_x = _bwd(sa, "pg", d["grad_y"], d["x"], None, f["mean"], f["invstd"], w, b, relu, False, off["grad_x"], 0, True, True, False)
                assert torch.equal(got["grad_x"], from_x["grad_x"]), (name, relu)
                if relu:
                    assert bool((from_x["grad_x"][f["y"] == 0] == 0).all()) and bool((got["grad_x"][f["y"] == 0] == 0).all())


@pytest.mark.parametrize("name", [n for n in sorted(OC.BN_CASES) if OC.BN_CASES[n][3] == 1])
def test_batch_statistics_backward_with_the_mask_from_x_bit_for_bit(sa, name):
    """B = 1 and one chunk: one workgroup per channel forms the sums, so no atomics reorder them, and the backward with y given and with
    the mask recomputed from x agree in grad_x, in the doubles of `work` and in the float gradients (the first batch element of the case)."""
    t = OC.bn_case(name)
    off = OC.offsets(name, residual=False)
    d = _dev(t, off, ["x", "grad_y"])
    x1, g1 = d["x"][:1], d["grad_y"][:1]
    assert x1.is_contiguous() and x1.data_ptr() == d["x"].data_ptr() and OC.reduce_grid(x1[0, 0].numel())[0] == 1
    for weight, bias in itertools.product((True, False), repeat=2):
        w, b = (_place(t["weight"]) if weight else None), (_place(t["bias"]) if bias else None)
        f = _fwd(sa, "rs", x1, None, w, b, True, off["y"])
        assert 0 < int((f["y"] > 0).sum()) < f["y"].numel()
        with_y = _bwd(sa, "pg", g1, x1, f["y"], f["mean"], f["invstd"], w, b, True, False, off["grad_x"])
        from_x = _bwd(sa, "pg", g1, x1, None, f["mean"], f["invstd"], w, b, True, False, off["grad_x"])
        for k in ("grad_x", "work", "grad_weight", "grad_bias"):
            assert torch.equal(with_y[k], from_x[k]), (name, weight, bias, k)


@pytest.mark.parametrize("name", ["scalar_105", "vector_1280", "misaligned_1280"])
def test_eval_backward_is_zero_where_the_pre_activation_is_exactly_zero(sa, name):
    """x = 0 on a channel with mean = 0 and bias = 0 (and on one with no bias at all): the pre-activation is exactly 0, y == 0, and
    grad_x is exactly 0 there with y given and with the mask from x; the elements around them keep their gradient."""
    t = OC.bn_case(name)
    B, C, spatial, N = OC.bn_shape(name)
    off = OC.offsets(name, residual=False)
    x = t["x"].clone()
    zero = torch.zeros_like(x, dtype=torch.bool)
    zero.reshape(B, C, N)[:, 0, ::3] = True
    x[zero] = 0.0
    mean, bias = t["run_mean"].clone(), t["bias"].clone()
    mean[0] = bias[0] = 0.0
    invstd = torch.rsqrt(t["run_var"] + OC.EPS)
    for with_bias in (True, False):
        if not with_bias and float(mean[0]) != 0.0:
            continue
        xd, gd = _place(x, off["x"]), _place(t["grad_y"], off["grad_y"])
        w, b = _place(t["weight"]), (_place(bias) if with_bias else None)
        stats = (_place(mean), _place(invstd))
        f = _fwd(sa, "eval", xd, None, w, b, True, off["y"], stats)
        assert bool((f["y"].cpu()[zero] == 0).all())
        for y in (f["y"], None):
            got = _bwd(sa, "pg", gd, xd, y, stats[0], stats[1], w, b, True, False, off["grad_x"], 0, True, True, False)
            gx = got["grad_x"].cpu()
            assert bool((gx[f["y"].cpu() == 0] == 0).all()) and bool(torch.isfinite(gx).all())
            live = f["y"].cpu() > 0
            assert int(live.sum()) > 0 and bool((gx[live] != 0).all())


# ---- c. module bookkeeping ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["momentum_none", "no_running_stats", "no_affine"])
@pytest.mark.parametrize("name", ["scalar_105", "vector_1280"])
def test_batchnorm_train_module_bookkeeping(sa, name, variant):
    """train.batchnorm_train on modules whose bookkeeping leaves the fused path's defaults, against a stock nn.BatchNorm3d in float64 on
    the CPU fed the same batches (two steps): outputs and gradients to the seam's bound, the running statistics and the batch counter as
    test_training_kernels_vs_float64_autograd compares them, and no PyTorch layer counted."""
    kw = {"momentum_none": {"momentum": None}, "no_running_stats": {"track_running_stats": False}, "no_affine": {"affine": False}}[variant]
    t = OC.bn_case(name)
    B, C, spatial, N = OC.bn_shape(name)
    bn, bnr = nn.BatchNorm3d(C, **kw).cuda().train(), nn.BatchNorm3d(C, **kw).double().train()
    if variant != "no_affine":
        with torch.no_grad():
            for m in (bn, bnr):
                m.weight.copy_(t["weight"])
                m.bias.copy_(t["bias"])
    W = _Worst(f"bn_module/{name}/{variant}")
    before = dict(sa.modules.PATH_COUNTS)
    for step, relu in enumerate((True, False)):
        x = t["x"] if step == 0 else t["residual"] * 3.0 - 0.7
        xh, xr = x.cuda().requires_grad_(True), x.double().requires_grad_(True)
        y = sa.train.batchnorm_train(bn, xh, relu)
        z = bnr(xr)
        yr = z * (y.detach().cpu() > 0).double() if relu else z                  # the ReLU decided like for like
        if relu:
            assert _flips(z.detach(), y.detach(), BOUND["fwd"])[1] == 0
        W.hold("y", f"step{step}", y, yr, BOUND["fwd"])
        for m in (bn, bnr):
            m.zero_grad()
        y.backward(t["grad_y"].cuda())
        yr.backward(t["grad_y"].double())
        W.hold("grad_x", f"step{step}", xh.grad, xr.grad, BOUND["bwd"])
        if variant != "no_affine":
            W.hold("grad_weight", f"step{step}", bn.weight.grad, bnr.weight.grad, BOUND["bwd"])
            W.hold("grad_bias", f"step{step}", bn.bias.grad, bnr.bias.grad, BOUND["bwd"])
        if variant == "no_running_stats":
            assert bn.running_mean is None and bn.running_var is None and bn.num_batches_tracked is None
        else:
            W.hold("running_mean", f"step{step}", bn.running_mean, bnr.running_mean, 1e-5)
            W.hold("running_var", f"step{step}", bn.running_var, bnr.running_var, 1e-5)
            assert int(bn.num_batches_tracked) == int(bnr.num_batches_tracked) == step + 1
    W.finish()
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"], "a PyTorch layer ran"
    assert sa.modules.PATH_COUNTS["hip_train"] == before.get("hip_train", 0) + 2


# ---- d. ranges --------------------------------------------------------------------------------------------------------------------------

def _per_channel(a, ref):
    """[C]: max|a - ref| / max|ref| per channel (axis 1) of [B,C,...] tensors, in float64."""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    dims = [0] + list(range(2, ref.dim()))
    return (a - ref).abs().amax(dims) / (ref.abs().amax(dims) + 1e-300)


def _mean_rounding_in_grad_x(t, r64, count):
    """[C]: what the fp32 `mean` of the ABI costs a channel of grad_x, relative to max|grad_x| of that channel.  The backward's closed
    form w invstd (g' - mean(g') - xhat mean(g' xhat)) takes xhat = (x - mean) invstd with the mean as the fp32 the forward stored:
    xhat moves by c = (mean32 - mean) invstd, |c| <= 2^-24 |mean| invstd, and grad_x by w invstd c (mean(g' xhat) + xhat mean(g')) to first
    order -- autograd in any precision differentiates its own rounded mean and has no such term.  Two roundings are allowed, as for the
    mean itself: 2^-23 |mean| invstd * w invstd (|mean(g' xhat)| + max|xhat| |mean(g')|), all from the float64 reference."""
    x = t["x"].double()
    dims = [0] + list(range(2, x.dim()))
    mean = r64["mean"]
    invstd = 1.0 / torch.sqrt(r64["var_unbiased"] * (count - 1) / count + OC.EPS)
    xhat_max = ((x - mean.reshape(TC._cshape(x))).abs().amax(dims)) * invstd
    c = 2.0 ** -23 * mean.abs() * invstd
    move = c * t["weight"].double().abs() * invstd * (r64["grad_weight"].abs() / count + xhat_max * r64["grad_bias"].abs() / count)
    return (move / (r64["grad_x"].abs().amax(dims) + 1e-300)).detach()


@pytest.mark.parametrize("relu", [True, False], ids=["relu_mask_from_x", "no_relu"])
@pytest.mark.parametrize("name", OC.RANGE_CASES)
def test_batchnorm_ranges_against_float32_on_the_cpu(sa, name, relu):
    """Channels drawn as (normal + off) * scale, off in {0, 10, 100, 1000}, scale in {1e-3, 1, 1e3}, one constant channel of 1000.1.
    Reference float64; yardstick the same reference in float32 on the CPU, same inputs and mask.
      y, grad_x, grad_weight, grad_bias over the tensor:  e <= 1.5 e32 + 1e-6,  e = max|hip - ref64| / max|ref64|
      y and grad_x also per channel, on the channel's own scale (grad_x grows with 1 / scale, so the channels of scale 1e-3 would hide the
      rest): the same rule; for grad_x plus what the ABI's fp32 mean moves it by (_mean_rounding_in_grad_x: below 1e-6 up to a mean of 10 std)
      var_unbiased per channel:  |v - v64| <= 1.5 |v32 - v64| + 1e-6 v64 + 1e-10 mean64^2   (exact sums pass, fp32 squares do not)
      mean per channel:          |m - m64| <= 1.5 |m32 - m64| + 2^-23 |m64|                  (two fp32 roundings of the double mean)
    Measured before and after the statistics kernel summed in double: profiles/train_ops_paths_err.txt."""
    t = OC.range_case(name)
    B, _, spatial, N = OC.bn_shape(name)
    off = OC.offsets(name, residual=False)
    chans = OC.range_channels()
    d = _dev(t, off, ["x", "grad_y"])
    w, b = _place(t["weight"]), _place(t["bias"])
    f = _fwd(sa, "rs", d["x"], None, w, b, relu, off["y"])
    got = _bwd(sa, "pg", d["grad_y"], d["x"], None, f["mean"], f["invstd"], w, b, relu, False, off["grad_x"], 0, True, True, True)
    mask = (f["y"] > 0).cpu() if relu else None
    r64 = OC.bn_reference(t, torch.float64, relu, False, True, True, True, mask)
    r32 = OC.bn_reference(t, torch.float32, relu, False, True, True, True, mask)
    tag = f"bn_range/{name}/{'relu' if relu else 'plain'}"
    bad = []
    names = [("const 1000.1" if oc is None else f"off {oc[0]:g} scale {oc[1]:g}") for oc in chans]
    for kind, hip in (("y", f["y"]), ("grad_x", got["grad_x"])):
        e, e32 = _per_channel(hip, r64[kind]), _per_channel(r32[kind], r64[kind])
        allow = _mean_rounding_in_grad_x(t, r64, B * N) if kind == "grad_x" else torch.zeros_like(e)
        for c, label in enumerate(names):
            ok = float(e[c]) <= 1.5 * float(e32[c]) + 1e-6 + float(allow[c])
            _line(f"{tag}/{kind:8s} ch{c:2d} {label:22s} e {float(e[c]):.3e}  e32 {float(e32[c]):.3e}  fp32 mean {float(allow[c]):.1e}"
                  f"  {'ok' if ok else 'ABOVE 1.5 e32 + 1e-6'}")
            if not ok:
                bad.append((kind, label, float(e[c]), float(e32[c])))
    for kind, hip in (("y", f["y"]), ("grad_x", got["grad_x"]), ("grad_weight", got["grad_weight"]), ("grad_bias", got["grad_bias"])):
        assert bool(torch.isfinite(hip).all()), (tag, kind)
        e, e32 = _rel(hip, r64[kind]), _rel(r32[kind], r64[kind])
        ok = e <= 1.5 * e32 + 1e-6
        _line(f"{tag}/{kind:8s} tensor {'':22s} e {e:.3e}  e32 {e32:.3e}  {'ok' if ok else 'ABOVE 1.5 e32 + 1e-6'}")
        if not ok:
            bad.append((kind, "tensor", e, e32))
    v, v64, v32 = f["var_unbiased"].double().cpu(), r64["var_unbiased"], r32["var_unbiased"].double()
    m, m64, m32 = f["mean"].double().cpu(), r64["mean"], r32["mean"].double()
    for c, label in enumerate(names):
        ev, bv = float((v[c] - v64[c]).abs()), float(1.5 * (v32[c] - v64[c]).abs() + 1e-6 * v64[c] + 1e-10 * m64[c] ** 2)
        em, bm = float((m[c] - m64[c]).abs()), float(1.5 * (m32[c] - m64[c]).abs() + 2.0 ** -23 * m64[c].abs())
        _line(f"{tag}/var      ch{c:2d} {label:22s} |v - v64| {ev:.3e} (bound {bv:.3e}, fp32 {float((v32[c] - v64[c]).abs()):.3e}, v64 {float(v64[c]):.3e})"
              f"  {'ok' if ev <= bv else 'ABOVE'}")
        _line(f"{tag}/mean     ch{c:2d} {label:22s} |m - m64| {em:.3e} (bound {bm:.3e}, fp32 {float((m32[c] - m64[c]).abs()):.3e})  {'ok' if em <= bm else 'ABOVE'}")
        if not ev <= bv:
            bad.append(("var_unbiased", label, ev, bv))
        if not em <= bm:
            bad.append(("mean", label, em, bm))
    assert not bad, bad


# ---- e. the neighbours --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", OC.CHANNEL_SUM_CASES)
def test_channel_sum_alone(sa, name):
    """ss_channel_sum_fwd (the bias gradient of _ConvK1) on one- and two-chunk, scalar, vector and misaligned rows: 2e-5 of the largest
    channel sum."""
    a = OC.channel_sum_case(name)
    B, C, N = a.shape
    misaligned = name.startswith("misaligned")
    ad = _place(a, int(misaligned))
    assert OC.reduce_is_vector(N, ad.data_ptr()) == (N % 4 == 0 and not misaligned)
    sums = _blank((C,), dtype=torch.float64)
    sa._lib.call("ss_channel_sum_fwd", _ptr(ad), _ptr(sums), B, C, N)
    torch.cuda.synchronize()
    W = _Worst(f"channel_sum/{name}")
    W.hold("sums", f"{OC.reduce_grid(N)[0]} chunks", sums, a.double().sum(dim=(0, 2)), TC.BOUNDS["train._ConvK1"]["bwd"])
    W.finish()


@pytest.mark.parametrize("name", sorted(OC.PATCH_CASES))
def test_depthwise_patch_weight_gradient_paths(sa, name):
    B, C, D, H, W_ = OC.PATCH_CASES[name]
    g, x = OC.patch_case(name)
    gd, xd, gw = _place(g), _place(x), _blank((C, 1, 1, 3, 3))        # (named: a temporary's block would be handed to the next tensor)
    sa._lib.call("ss_depthwise_patch_wgrad_fwd", _ptr(gd), _ptr(xd), _ptr(gw), B, C, D, H, W_)
    torch.cuda.synchronize()
    W = _Worst(f"patch_wgrad/{name}")
    W.hold("grad_w", f"rows_per_block {OC.depthwise_rows(D, H)[0]}", gw, OC.patch_wgrad_ref(g.double(), x.double()), TC.BOUNDS["train._DepthwisePatch"]["bwd"])
    W.finish()
    dead = OC.patch_dead_taps(H, W_)
    assert bool((gw.cpu()[:, 0, 0][:, dead] == 0).all()), "a tap that never sees the image is not exactly zero"


@pytest.mark.parametrize("name", sorted(OC.GATE_CASES))
def test_channel_gate_logits_gradient_paths(sa, name):
    B, C, D, H, W_ = OC.GATE_CASES[name]
    g, cv, a = OC.gate_case(name)
    gd, cd, ad, da = _place(g), _place(cv), _place(a), _blank((B, C, H, W_))
    sa._lib.call("ss_channel_gate_bwd_logits", _ptr(gd), _ptr(cd), _ptr(ad), _ptr(da), B, C, D, H, W_)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(da).all()), "NaN or Inf at a saturated sigmoid"
    W = _Worst(f"gate_logits/{name}")
    W.hold("grad_att", "logits +-30, +-100 among O(1)", da, OC.gate_logits_grad_ref(g.double(), cv.double(), a.double()), TC.BOUNDS["train._ChannelGate"]["bwd"])
    W.finish()


@pytest.mark.parametrize("name", sorted(OC.K1_POSITIONS))
@pytest.mark.parametrize("cin,cout", OC.K1_CHANNELS, ids=lambda v: str(v))
def test_conv_k1_weight_gradient_paths(sa, cin, cout, name):
    B, npos, misaligned = OC.K1_POSITIONS[name]
    g, x = OC.k1_case(cin, cout, name)
    gd, xd = _place(g), _place(x, int(misaligned == "in"))
    plan = OC.k1_wgrad_plan(B, cin, cout, npos, gd.data_ptr(), xd.data_ptr())
    assert plan["vec"] == [npos % 4 == 0 and not misaligned] * plan["gx"]
    gw = _blank((cout, cin))
    sa._lib.call("ss_conv_k1_wgrad_fwd", _ptr(gd), _ptr(xd), _ptr(gw), B, cin, cout, npos)
    torch.cuda.synchronize()
    W = _Worst(f"k1_wgrad/{cin}x{cout}/{name}")
    W.hold("grad_w", f"{plan['gx']} workgroups of {plan['positions']}", gw, OC.k1_wgrad_ref(g.double(), x.double()), TC.BOUNDS["train._ConvK1"]["bwd"])
    W.finish()
