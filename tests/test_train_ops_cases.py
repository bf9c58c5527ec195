"""CPU: every case of tests/train_ops_cases.py reaches the branch it is named for -- by the host rules of csrc/train_ops.hip and
csrc/conv3d_wgrad.hip restated there -- and the float64 references of tests/test_train_ops_paths_gpu.py agree with F.batch_norm,
F.conv2d / F.conv3d and autograd in float64."""
import pytest
import torch
import torch.nn.functional as F

import train_calls as TC
import train_ops_cases as OC


def _rel(a, ref):
    return float((a.double() - ref.double()).abs().max()) / (float(ref.double().abs().max()) + 1e-300)


# ---- the restated rules -----------------------------------------------------------------------------------------------------------------

def test_reduce_grid_chunks():
    assert OC.reduce_grid(4) == (1, 4) and OC.reduce_grid(105) == (1, 108) and OC.reduce_grid(1280) == (1, 1280)
    assert OC.reduce_grid(16384) == (1, 16384)
    assert OC.reduce_grid(16385) == (2, 8196) and OC.chunk_lengths(16385) == [8196, 8189]
    assert OC.reduce_grid(16388) == (2, 8196) and OC.chunk_lengths(16388) == [8196, 8192]
    assert OC.reduce_grid(16384 * 65535 + 1)[0] <= 65535           # (the cap on the grid's x)
    for N in (4, 105, 1280, 16385, 16388, 3 * 16384 + 2):
        gx, per_block = OC.reduce_grid(N)
        assert per_block % 4 == 0 and (gx - 1) * per_block < N <= gx * per_block and sum(OC.chunk_lengths(N)) == N


def test_alignment_rules():
    assert OC.vec4_ok(1280, 0, 0, 16, 32) and not OC.vec4_ok(1280, 0, 4) and not OC.vec4_ok(105, 0, 0)
    assert OC.vec4_ok(1280, None, 16)                              # (a NULL tensor has no bits)
    assert OC.reduce_is_vector(16388, 0) and not OC.reduce_is_vector(16385, 0) and not OC.reduce_is_vector(16388, 4)
    assert OC.reduce_is_vector(1280, 0, 0, None) and not OC.reduce_is_vector(1280, 0, 0, 4)
    assert OC.apply_grid(4) == 1 and OC.apply_grid(16388) == 5 and OC.apply_grid(65535 * 4096 + 1) == 65535


@pytest.mark.parametrize("name", sorted(OC.BN_CASES))
def test_batchnorm_cases_take_the_forms_they_are_named_for(name):
    (B, C, spatial), off_centre, forms, chunks = OC.BN_CASES[name]
    _, _, _, N = OC.bn_shape(name)
    assert OC.reduce_grid(N)[0] == chunks
    present = {t: True for t in OC.ALL_TENSORS}
    assert OC.expected_forms(N, OC.addresses(OC.offsets(name), present)) == forms
    assert name.startswith(forms[0]) or name.startswith(("misaligned", "mixed"))
    t = OC.bn_case(name)
    assert t["x"].shape == (B, C) + tuple(spatial) == t["residual"].shape == t["grad_y"].shape and t["x"].dtype == torch.float32
    spread = 8.0 / t["x"].numel() ** 0.5                          # (four standard errors of the mean of std-2 samples)
    assert abs(float(t["x"].mean()) - 0.3) < spread and abs(float(t["x"].std()) - 2.0) < spread
    if name == "scalar_105":
        assert N == 105 and (B * C * N) % 256 != 0                 # a partial last block of the scalar apply kernels
    if name == "vector_4":
        assert N == 4 and C % 2 == 1
    if name == "vector_two_chunks_16388":
        assert OC.chunk_lengths(N) == [8196, 8192] and 8196 % 1024 == 4      # the first chunk ends inside the 1024-element stride
    if name == "scalar_two_chunks_16385":
        assert OC.chunk_lengths(N) == [8196, 8189] and N % 4 == 1
    if name.startswith("misaligned"):
        assert N % 4 == 0 and set(off_centre) == set(OC.ALL_TENSORS)
    if name == "mixed_1280":
        # without a residual (and its gradient) the forward is all vector; the backward keeps grad_x off the boundary
        addr = OC.addresses(OC.offsets(name, residual=False), {"residual": False, "grad_residual": False})
        assert OC.expected_forms(N, addr) == ("vector", "vector", "vector", "scalar")
    # y == NULL (the mask from x): no bits in either backward rule
    addr = OC.addresses(OC.offsets(name), {"y": False})
    assert OC.expected_forms(N, addr)[2:] == forms[2:]


def test_range_and_sum_cases_exist():
    assert set(OC.RANGE_CASES) <= set(OC.BN_CASES) and set(OC.CHANNEL_SUM_CASES) <= set(OC.BN_CASES)
    assert [OC.bn_shape(n)[3] for n in OC.RANGE_CASES] == [105, 1280, 16388, 1280]
    assert sorted({OC.bn_shape(n)[3] for n in OC.CHANNEL_SUM_CASES}) == [105, 1280, 16385, 16388]


# ---- the references ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("relu,residual,weight,bias", [(True, True, True, True), (False, False, False, False), (True, False, True, False),
                                                        (False, True, False, True)])
@pytest.mark.parametrize("name", ["scalar_105", "vector_4"])
def test_batch_statistics_reference_is_f_batch_norm(name, relu, residual, weight, bias):
    t = OC.bn_case(name)
    got = OC.bn_reference(t, torch.float64, relu, residual, weight, bias, True)
    x = t["x"].double().requires_grad_(True)
    w = t["weight"].double().requires_grad_(True) if weight else None
    b = t["bias"].double().requires_grad_(True) if bias else None
    r = t["residual"].double().requires_grad_(True) if residual else None
    y = F.batch_norm(x, None, None, w, b, True, 0.0, OC.EPS)
    if residual:
        y = y + r
    y = F.relu(y) if relu else y
    leaves = [v for v in (x, w, b, r) if v is not None]
    grads = dict(zip([n for n, v in (("grad_x", x), ("grad_weight", w), ("grad_bias", b), ("grad_residual", r)) if v is not None],
                     torch.autograd.grad(y, leaves, t["grad_y"].double())))
    assert _rel(got["y"], y.detach()) <= 1e-13
    for k, g in grads.items():
        assert _rel(got[k], g) <= 1e-12, k
    dims = [0] + list(range(2, x.dim()))
    assert _rel(got["mean"], x.detach().mean(dims)) <= 1e-14 and _rel(got["var_unbiased"], x.detach().var(dims, unbiased=True)) <= 1e-13
    n = x.numel() // x.shape[1]
    assert _rel(got["sum_x"] / n, got["mean"]) <= 1e-14
    # the absent affine term's would-be gradient: the same sums as with the term present and equal to one / zero
    if not weight:
        ones = dict(t, weight=torch.ones_like(t["weight"]))
        assert _rel(got["grad_weight"], OC.bn_reference(ones, torch.float64, relu, residual, True, bias, True)["grad_weight"]) <= 1e-13


@pytest.mark.parametrize("relu,residual", [(True, True), (False, False), (True, False)])
def test_running_statistics_reference_is_f_batch_norm_in_eval(relu, residual):
    t = OC.bn_case("vector_4")
    invstd = torch.rsqrt(t["run_var"] + OC.EPS)                     # fp32, as the kernel receives it
    got = OC.bn_reference(t, torch.float64, relu, residual, True, True, False, stats=(t["run_mean"], invstd))
    x, w, b = (t[k].double().requires_grad_(True) for k in ("x", "weight", "bias"))
    var = 1.0 / invstd.double() ** 2 - OC.EPS
    y = F.batch_norm(x, t["run_mean"].double(), var, w, b, False, 0.0, OC.EPS)
    r = t["residual"].double().requires_grad_(True)
    if residual:
        y = y + r
    y = F.relu(y) if relu else y
    gx, gw, gb = torch.autograd.grad(y, [x, w, b], t["grad_y"].double())
    assert _rel(got["y"], y.detach()) <= 1e-12 and _rel(got["grad_x"], gx) <= 1e-12
    assert _rel(got["grad_weight"], gw) <= 1e-12 and _rel(got["grad_bias"], gb) <= 1e-12


def test_a_given_mask_replaces_the_sign_of_the_pre_activation():
    t = OC.bn_case("scalar_105")
    free = OC.bn_reference(t, torch.float64, True, False, True, True, True)
    same = OC.bn_reference(t, torch.float64, True, False, True, True, True, mask=free["y"] > 0)
    assert torch.equal(free["y"], same["y"]) and torch.equal(free["grad_x"], same["grad_x"])
    none = OC.bn_reference(t, torch.float64, True, False, True, True, True, mask=torch.zeros_like(free["y"]))
    assert float(none["y"].abs().max()) == 0.0 and float(none["grad_x"].abs().max()) == 0.0 and float(none["grad_bias"].abs().max()) == 0.0


def test_range_inputs():
    chans = OC.range_channels()
    assert len(chans) == 13 and chans[-1] is None and len(set(chans[:-1])) == 12
    assert {c[0] for c in chans[:-1]} == set(OC.RANGE_OFFSETS) and {c[1] for c in chans[:-1]} == set(OC.RANGE_SCALES)
    assert all(a[0] != b[0] and a[1] != b[1] for a, b in zip(chans[:-2], chans[1:-1]))         # neighbouring channels differ
    for name in OC.RANGE_CASES:
        t = OC.range_case(name)
        B, _, spatial, N = OC.bn_shape(name)
        assert t["x"].shape == (B, 13) + tuple(spatial)
        x = t["x"].double().transpose(0, 1).reshape(13, -1)
        assert bool((x[12] == float(torch.tensor(OC.CONSTANT_VALUE, dtype=torch.float32))).all())
        for c, (off, scale) in enumerate(chans[:-1]):
            assert abs(float(x[c].mean()) / scale - off) < 0.5 and 0.7 < float(x[c].std()) / scale < 1.3, (name, c)
        ref = OC.bn_reference(t, torch.float64, True, False, True, True, True)
        assert float(ref["var_unbiased"][12]) == 0.0 and all(bool(torch.isfinite(v).all()) for v in ref.values() if v is not None)


def test_channel_sum_inputs_do_not_cancel():
    for name in OC.CHANNEL_SUM_CASES:
        a = OC.channel_sum_case(name).double()
        s = a.sum(dim=(0, 2))
        assert float(s.abs().min()) > 0.25 * a.shape[0] * a.shape[2]


@pytest.mark.parametrize("name", sorted(OC.PATCH_CASES))
def test_patch_cases(name):
    B, C, D, H, W = OC.PATCH_CASES[name]
    rpb, blocks, last = OC.depthwise_rows(D, H)
    if name == "rows_65":
        assert (D * H, rpb, blocks, last) == (65, 2, 33, 1)
    if name == "wide_block":
        assert rpb * W > 256
    if name == "one":
        assert (rpb, blocks, last) == (1, 1, 1)
    g, x = OC.patch_case(name)
    gw = OC.patch_wgrad_ref(g.double(), x.double())
    w = torch.zeros((C, 1, 1, 3, 3), dtype=torch.float64, requires_grad=True)
    (want,) = torch.autograd.grad(F.conv3d(x.double(), w, None, 1, (0, 1, 1), 1, C), w, g.double())
    assert _rel(gw, want) <= 1e-13
    dead = OC.patch_dead_taps(H, W)
    assert int(dead.sum()) == {"w1": 6, "h1": 6, "one": 8}.get(name, 0)
    assert bool((gw[:, 0, 0][:, dead] == 0).all()) and bool((gw[:, 0, 0][:, ~dead] != 0).all())


@pytest.mark.parametrize("name", sorted(OC.GATE_CASES))
def test_gate_cases(name):
    B, C, D, H, W = OC.GATE_CASES[name]
    g, cv, a = OC.gate_case(name)
    if name == "d1_plane257":
        assert D == 1 and B * C * H * W == 257
    assert all(bool((a.reshape(B, C, -1)[:, :, i] == v).all()) for i, v in enumerate(OC.SATURATED_LOGITS))
    a64 = a.double().requires_grad_(True)
    (want,) = torch.autograd.grad(TC.gate_ref(a64, cv.double()), a64, g.double())
    got = OC.gate_logits_grad_ref(g.double(), cv.double(), a.double())
    assert _rel(got, want) <= 1e-12 and bool(torch.isfinite(got).all())
    assert float(got.reshape(B, C, -1)[:, :, :4].abs().max()) < 1e-10 * float(got.abs().max())       # the saturated elements: ~0


@pytest.mark.parametrize("name", sorted(OC.K1_POSITIONS))
@pytest.mark.parametrize("cin,cout", OC.K1_CHANNELS)
def test_k1_wgrad_cases(cin, cout, name):
    B, npos, misaligned = OC.K1_POSITIONS[name]
    plan = OC.k1_wgrad_plan(B, cin, cout, npos, 0, 4 if misaligned else 0)
    assert plan["pos_per_wg"] == 128 and plan["gx"] == -(-npos // 128) and plan["splits"] == 2048 // (plan["tiles"] * B)
    want = {"npos35": ([False], [35]), "npos132": ([True, True], [128, 4]), "npos260_b3": ([True] * 3, [128, 128, 4]),
            "npos132_misaligned": ([False, False], [128, 4])}[name]
    assert (plan["vec"], plan["positions"]) == want
    assert plan["tiles"] == {(33, 1): 2, (3, 5): 1, (40, 70): 6}[(cin, cout)]
    g, x = OC.k1_case(cin, cout, name)
    w = torch.zeros((cout, cin, 1), dtype=torch.float64, requires_grad=True)
    (gw,) = torch.autograd.grad(F.conv1d(x.double(), w), w, g.double())
    assert _rel(OC.k1_wgrad_ref(g.double(), x.double()), gw[:, :, 0]) <= 1e-13
    # ... which is also the weight gradient of the 1x1x1 Conv3d on the same positions
    w5 = torch.zeros((cout, cin, 1, 1, 1), dtype=torch.float64, requires_grad=True)
    (gw5,) = torch.autograd.grad(TC.k1_ref(x.double().reshape(B, cin, 1, 1, npos), w5, None), w5, g.double().reshape(B, cout, 1, 1, npos))
    assert _rel(OC.k1_wgrad_ref(g.double(), x.double()), gw5.reshape(cout, cin)) <= 1e-13


def test_large_k1_split_keeps_whole_words():
    """With more positions than 128 per workgroup the split stays a multiple of 128, so every workgroup starts on a 16-byte word."""
    plan = OC.k1_wgrad_plan(1, 32, 32, 1 << 20)
    assert plan["splits"] == 2048 and plan["pos_per_wg"] == 512 and all(plan["vec"])
