"""CPU: every input of tests/bwd_path_cases.py has the property it is named for -- the taps really reach the row, column, slot or
branch that tests/test_bwd_paths_gpu.py means to exercise -- and the float64 references stay finite on them."""
import pytest
import torch

import bwd_path_cases as BP
import train_calls as TC


@pytest.fixture(scope="module")
def strength():
    return {name: BP.strength_case(name) for name in BP.STRENGTH_CASES}


def test_row_coordinate_round_trip_by_height():
    """The fp32 round trip of the row coordinate: exact for H <= 5 and H = 12; rows just below (taps in y - 1, y) at H = 6, 8, 10; a row
    just above (taps in y, y + 1) at H = 7."""
    for H in (2, 3, 4, 5, 12):
        assert set(BP.row_kinds(H)) == {0}, (H, BP.row_kinds(H))
    for H in (6, 8, 10):
        assert -1 in BP.row_kinds(H) and 1 not in BP.row_kinds(H), (H, BP.row_kinds(H))
    assert 1 in BP.row_kinds(7)
    assert BP.row_kinds(10)[1] == BP.row_kinds(10)[2] == -1 and BP.row_kinds(7)[1] == 1


@pytest.mark.parametrize("name", sorted(BP.STRENGTH_CASES))
def test_strength_cases_keep_off_the_derivative_jumps_and_have_their_shape(strength, name):
    ins, go, p = strength[name]
    B, C, H, W = p["shape"]
    assert ins[0].shape == ins[1].shape == (B, C, H, W) and ins[2].shape == (B, H, W) and ins[3].shape == (B, 1, H, W)
    assert go.shape == (B, 5, H, W) and all(t.dtype == torch.float32 for t in ins + [go])
    assert p["min_frac"] >= 0.1, p["min_frac"]
    assert float(ins[3].min()) >= 0.0 and float(ins[3].max()) <= 20.0
    assert p["row_buffer"] == (name != "ragged")


def test_rows_exact(strength):
    p = strength["rows_exact"][2]
    assert p["row_same"] > 0 and p["row_above"] == 0 and p["row_below"] == 0 and set(p["row_kinds"]) == {0}
    B, C, H, W = p["shape"]
    assert W == 64 and p["blocks"] == B * H                   # one block per row
    assert 16 < C < 32 and (C - 16 + 1) // 2 == 2             # the second channel block of the two-launch form: two live waves of eight


def test_rows_below(strength):
    p = strength["rows_below"][2]
    assert p["row_above"] > 0 and p["row_same"] > 0 and p["row_below"] == 0
    assert p["row_kinds"][1] == p["row_kinds"][2] == -1


def test_rows_above(strength):
    p = strength["rows_above"][2]
    assert p["row_below"] > 0 and p["row_same"] > 0 and p["row_kinds"][1] == 1
    assert p["shape"][3] == 128 and p["blocks"] == 2 * p["shape"][2]          # two blocks per row


@pytest.mark.parametrize("name", sorted(BP.SECOND_ROW_ONLY))
def test_one_row_of_grad_right_holds_second_row_taps_alone(strength, name):
    """`left` is zero on the row whose main taps land in row r: in float64, row r of grad_right is not zero, and ~1e-7 of the rest."""
    ins, go, p = strength[name]
    r = p["second_row_only"]
    assert r == BP.SECOND_ROW_ONLY[name] and p["row_kinds"][r] == 0 and not bool(ins[0][:, :, r].any())
    assert p["row_kinds"][r + 1] == -1 if name == "rows_below" else p["row_kinds"][r - 1] == 1
    right = ins[1].double().requires_grad_(True)
    out = TC.strength_ref(ins[0].double(), right, *[t.double() for t in ins[2:]])
    (g,) = torch.autograd.grad(out, right, go.double())
    row, rest = float(g[:, :, r].abs().max()), float(g.abs().max())
    assert 0.0 < row < 1e-5 * rest, (row, rest)
    assert int((g[:, :, r] != 0).sum()) > 16 * p["shape"][1]


def test_collide(strength):
    p = strength["collide"][2]
    assert p["max_lanes_one_slot"] == 64
    assert p["outside_window"] == 0 and p["leave_image"] == 0                  # every add goes through the row buffer
    assert p["shape"][1] == 7                                                  # an odd last pair, four of eight waves without a channel
    assert strength["rows_exact"][2]["max_lanes_one_slot"] < 16                # (the random cases do not reach this)


def test_beyond_margin(strength):
    p = strength["beyond_margin"][2]
    assert p["beyond_margin"] > 0 and p["outside_window"] > 0 and p["leave_image"] > 0
    assert float(strength["beyond_margin"][0][2].abs().min()) >= 70.0 and float(strength["beyond_margin"][0][2].abs().max()) <= 120.0
    assert bool((strength["beyond_margin"][0][2] > 0).any()) and bool((strength["beyond_margin"][0][2] < 0).any())


def test_borders(strength):
    ins, _, p = strength["borders"]
    assert p["shape"][2] == 2 and p["col_minus1"] > 0 and p["col_W"] > 0 and p["leave_image"] > 0
    assert float(ins[2].abs().max()) <= 1.8
    assert p["outside_window"] == 0


def test_ragged(strength):
    p = strength["ragged"][2]
    B, C, H, W = p["shape"]
    assert W % 64 != 0 and B == 2 and p["blocks"] == 11 and p["lanes_in_last_block"] == 60
    assert C % 2 == 1


@pytest.mark.parametrize("name", ["rows_exact", "rows_below", "rows_above", "ragged"])
def test_no_case_but_beyond_margin_leaves_the_window(strength, name):
    assert strength[name][2]["beyond_margin"] == 0


@pytest.mark.parametrize("name", sorted(BP.GWC_CASES))
def test_gwc_cases_take_the_kernel_they_are_named_for(name):
    ref, tgt, G, maxdisp, signed, go, p = BP.gwc_case(name)
    assert p["rows_kernel"] == name.startswith(("rows", "same"))
    if name == "generic_cg12":
        assert p["cg"] == 12
    if name == "generic_lds":
        assert p["cg"] == 8 and p["range"][1] == 48 and ref.shape[3] == 512 and p["lds_bytes"] == 128 * 1024
    if name == "generic_d50":
        assert p["range"] == (0, 50) and p["empty_planes"] == 10
    if name == "rows_wide_d":
        assert p["empty_planes"] > p["range"][1] // 2
    if name == "same_sums":
        B, C, H, W = ref.shape
        assert not BP.gwc_rows_kernel_applies(3 * C, W, p["range"][1], G) and not BP.gwc_rows_kernel_applies(2 * C, W, p["range"][1], G)
        wide = BP.widen_groups(ref, G, 3)
        assert wide.shape == (B, 3 * C, H, W)
        assert all(torch.equal(BP.narrow_groups(wide, G, 3)[:, :, r].reshape(ref.shape), ref) for r in range(3))
        # the wider call is the same operation: the mean over three copies of a group's products is the mean over the group
        w64 = TC.gwc_ref(wide.double(), BP.widen_groups(tgt, G, 3).double(), p["range"], G)
        assert float((w64 - TC.gwc_ref(ref.double(), tgt.double(), p["range"], G)).abs().max()) <= 1e-14


def test_group_normalise_case_and_its_reference_at_zero_groups():
    """torch's norm backward gives 0 for the second term where the norm is 0: the float64 reference is finite there, and the gradient
    is grad_y / eps."""
    x, G, gy, zero = BP.group_normalise_case()
    cg = x.shape[1] // G
    v = x.reshape(x.shape[0], G, cg, *x.shape[2:])
    assert int((v.abs().amax(dim=2) == 0).sum()) == len(BP.ZERO_GROUPS) == 3 and int(zero.sum()) == 3 * cg
    b, g, y, xx = BP.ONE_CHANNEL_GROUP
    assert int((v[b, g, :, y, xx] != 0).sum()) == 1
    x64 = x.double().requires_grad_(True)
    out = TC.group_normalise_ref(x64, G)
    (gx,) = torch.autograd.grad(out, x64, gy.double())
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gx).all())
    assert bool((out.detach()[zero] == 0).all())
    assert torch.allclose(gx[zero], gy.double()[zero] / 1e-05, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("shape", BP.TOPK_CASES)
def test_topk_cases(shape):
    logits, strength, k, rng, ga, gp, p = BP.topk_case(shape)
    B, D, H, W, _ = shape
    assert k in (6, 24, 32) and k <= D <= 192 and p["lds_bytes"] <= 48 * 1024 and rng == (-(D // 2), D)
    assert logits.shape == (B, 1, D, H, W) and strength.shape == (B, 5, H, W) and ga.shape == (B, 1, k, H, W) and gp.shape == (B, H, W)
    if W == 1:
        assert p["border_taps"] == p["off_centre_taps"]          # every replicate-padded tap but the centre is a border tap
    if H == 2:
        assert p["border_taps"] >= p["off_centre_taps"] // 2     # every pixel is a border pixel: two of its four diagonal taps at least
    assert p["border_taps"] > 0


@pytest.mark.parametrize("shape", BP.UPSOFT_CASES)
def test_upsoft_cases_have_a_coarse_axis_of_length_one(shape):
    coarse, H, W, rng, grads = BP.upsoft_case(shape)
    assert 1 in shape[2:] and coarse.shape == shape and rng[1] == 2 * shape[2] and (H, W) == (2 * shape[3], 2 * shape[4])
    assert grads[0].shape == (shape[0], 1, rng[1], H, W)
    up, disp, var = TC.upsoft_ref(coarse.double(), H, W, rng)
    assert bool(torch.isfinite(up).all()) and bool(torch.isfinite(var).all())
