"""CPU: right_view and lr_consistency (semstereo_amd/data.py; the kernels are csrc/right_view.hip) -- the PyTorch composition against the
sequential restatement of tests/right_view_cases.py on every case and closed form, the key rules of prepare_sample, the ABI of the two
entry points and their refusals, and the properties that tie the consistency check to the right view.  Every comparison is
torch.equal: the outputs are selections, one subtraction or one comparison, so no tolerance appears (no GPU needed)."""
import ctypes
import os
import re

import pytest
import torch

import right_view_cases as rc
from abi import ROOT, declared, library

NAMES = ("ss_right_view_fwd", "ss_lr_consistency_fwd")
INF = float("inf")


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    return semstereo_amd


def moved(sa, before, key):
    return sa.modules.PATH_COUNTS.get(key, 0) - before.get(key, 0)


def same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        assert torch.equal(got[k], want[k]), f"{what} {k}: {(got[k] != want[k]).sum().item()} of {want[k].numel()} values differ"


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.CASES))
def test_composition_equals_the_restatement(sa, name):
    d, y, lo, hi, want = rc.case(name)
    before = dict(sa.modules.PATH_COUNTS)
    got = sa.right_view(d, y, maxdisp=rc.CASES[name][3])
    assert moved(sa, before, "data_torch") == 1 and moved(sa, before, "data_hip") == 0
    assert tuple(got) == sa.RIGHT_VIEW_KEYS and got["left_visible"].dtype == torch.bool
    same(got, want, name)
    same(sa.right_view(d, y, disp_range=(lo, hi)), want, name + " by range")
    share = want["left_visible"].float().mean().item()
    print(f"{name}: visible share {share:.2f}")
    assert 0.0 < share < 1.0                                            # the case has both kinds of pixel
    # the planted values
    W = d.shape[-1]
    assert want["left_visible"][0, 0, 1] and not want["left_visible"][0, 0, 0] and want["right_disparity"][0, 0, 0] == 1.5
    assert bool(want["left_visible"][0, 0, W - 1]) == (W % 2 == 1)      # W - 0.5 rounds to W for an even W
    assert not want["left_visible"][-1, -1].any()                       # the all-invalid row
    assert (want["right_disparity"][-1, -1] == rc.FILL_DISPARITY).all() and (want["right_label"][-1, -1] == rc.FILL_LABEL).all()


def test_the_unsigned_range_and_other_fills(sa):
    d, y, _, _ = rc.make_case("batch_w37")
    want = rc.restate(d, y, 0.0, 8.0, fill_disparity=0.0, fill_label=255.0)
    same(sa.right_view(d, y, disp_range=(0, 8), fill_disparity=0.0, fill_label=255.0), want, "unsigned")
    assert not want["left_visible"][d < 0].any()


@pytest.mark.parametrize("form", rc.closed_forms(), ids=lambda f: f[0])
def test_closed_forms(sa, form):
    what, d, y, maxdisp, rd, rl, vis = form
    want = {"right_disparity": rd, "right_label": rl, "left_visible": vis}
    same(rc.restate(d, y, -maxdisp, maxdisp), want, what + " (restatement)")
    same(sa.right_view(d, y, maxdisp=maxdisp), want, what)
    same(sa.right_view(d[0], y[0], maxdisp=maxdisp), {k: v[0] for k, v in want.items()}, what + " [H,W]")


@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8, torch.float32])
def test_label_dtypes_and_a_column_slice(sa, dtype):
    d, y, lo, hi, want = rc.case("batch_w37")
    wide = torch.cat([y + 1, y, y + 2], dim=2).to(dtype)
    crop = wide[:, :, 37:74]                                            # row stride 111, first pixel at an odd offset
    assert crop.stride(1) == 111 and not crop.is_contiguous()
    same(sa.right_view(d, crop, maxdisp=8), want, f"{dtype} slice")
    same(sa.right_view(d, y.to(dtype), maxdisp=8, want=("right_label",)), {"right_label": want["right_label"]}, f"{dtype}")


def test_other_inputs_and_the_arguments(sa):
    d, y, lo, hi, want = rc.case("quads_w7")
    same(sa.right_view(d.double(), y, maxdisp=4), want, "float64")      # converted first: the definitions are fp32
    got = sa.right_view(d, maxdisp=4, want=("left_visible", "right_disparity"))
    assert tuple(got) == ("left_visible", "right_disparity")            # no label needed, the caller's order
    for bad in (dict(), dict(maxdisp=4, disp_range=(-4, 4)), dict(disp_range=(4, 4)), dict(disp_range=(float("nan"), 4))):
        with pytest.raises(AssertionError):
            sa.right_view(d, y, **bad)
    with pytest.raises(AssertionError):
        sa.right_view(d, None, maxdisp=4)                               # right_label is asked for by default
    with pytest.raises(AssertionError):
        sa.right_view(d, y, maxdisp=4, want=("right_lable",))
    with pytest.raises(AssertionError):
        sa.lr_consistency(d, d, threshold=-1.0, maxdisp=4)
    assert not sa.right_view(d.requires_grad_(False), y, maxdisp=4)["right_disparity"].requires_grad


# 2 ------------------------------------------------------------------------------------------------------------------------------
def _raw(B=2, H=16, W=32, whu=False):
    g = torch.Generator().manual_seed(9300)
    raw = {"left_u8": torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8),
           "right_u8": torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)}
    if whu:
        raw["disparity"] = torch.randint(0, 12 * 256, (B, H, W), generator=g, dtype=torch.int32)
    else:
        raw["disparity"] = torch.round(16 * torch.rand(B, H, W, generator=g) - 8)
        raw["label"] = torch.randint(0, 6, (B, H, W), generator=g, dtype=torch.uint8)
    return raw


def test_prepare_sample_key_rules(sa):
    raw = _raw()
    for training, n in ((True, 11), (False, 8)):                        # the default dictionaries are today's, with or without a range
        a, b = sa.prepare_sample(raw, training), sa.prepare_sample(raw, training, maxdisp=8)
        assert list(a) == list(b) and len(a) == n and not set(a) & set(sa.RIGHT_VIEW_KEYS)
        assert tuple(a) == tuple(k for k in sa.data.KEYS[("us3d", training)] if k in a)
    want = rc.restate(raw["disparity"], raw["label"], -8.0, 8.0)
    before = dict(sa.modules.PATH_COUNTS)
    s = sa.prepare_sample(raw, True, keys=("left_visible", "right_label"), maxdisp=8)
    assert moved(sa, before, "data_torch") == 1                         # only what is named: one right_view call, no views, no pyramid
    assert tuple(s) == ("right_label", "left_visible")
    same(s, {k: want[k] for k in s}, "subset")
    before = dict(sa.modules.PATH_COUNTS)
    s = sa.prepare_sample(raw, True, keys=("left", "disparity", "label") + sa.RIGHT_VIEW_KEYS, disp_range=(-8, 8))
    assert moved(sa, before, "data_torch") == 3                         # the view, the pyramid call, the right view
    assert tuple(s) == ("left", "disparity", "label") + sa.RIGHT_VIEW_KEYS
    same({k: s[k] for k in sa.RIGHT_VIEW_KEYS}, want, "with the reference's keys")
    same(sa.prepare_sample(raw, False, keys=sa.RIGHT_VIEW_KEYS, maxdisp=8), want, "test branch")
    for bad in (dict(), dict(maxdisp=8, disp_range=(-8, 8))):           # a right-view key without a range, or with two
        with pytest.raises(AssertionError):
            sa.prepare_sample(raw, True, keys=("left", "left_visible"), **bad)
    with pytest.raises(AssertionError):
        sa.prepare_sample(raw, True, keys=("left", "lable"), maxdisp=8)
    assert tuple(sa.prepare_sample(raw, True, keys=("left",))) == ("left",)             # no range needed where none is used


def test_whu_warps_the_scaled_map(sa):
    raw = _raw(whu=True)
    scaled = raw["disparity"].float() / 256
    want = rc.restate(scaled, None, 0.0, 12.0)
    for keys in (("right_disparity", "left_visible"), ("disparity", "right_label", "right_disparity", "left_visible")):
        s = sa.prepare_sample(raw, True, keys=keys, disp_range=(0, 12))
        assert "right_label" not in s                                   # (no label: as a name of the other branch)
        same({k: s[k] for k in want}, want, "whu")
    loader = sa.DeviceLoader([raw], device="cpu", keys=("disparity", "left_visible"), training=True, disp_range=(0, 12))
    (s,) = list(loader)
    assert tuple(s) == ("disparity", "left_visible") and torch.equal(s["left_visible"], want["left_visible"])
    with pytest.raises(AssertionError):
        list(sa.DeviceLoader([raw], device="cpu", keys=("left_visible",), training=True))


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    _l, lib = library()
    decl = declared()
    for name in NAMES:
        assert name in decl and name in _l._SIGNATURES and name in _l.EXPORTS, name
        assert len(_l._SIGNATURES[name]) == len(decl[name][1]), name
        assert hasattr(lib, name) and decl[name][1][-1] == "ss_stream_t", name
    assert len(decl["ss_right_view_fwd"][1]) == 16 and len(decl["ss_lr_consistency_fwd"][1]) == 11
    assert _l.ABI_VERSION == 20 and lib.ss_abi_version() == 20          # symbols were added, nothing changed
    srcs = re.search(r"^SRCS_HIP\s*:=(.*)$", open(os.path.join(ROOT, "semstereo_amd", "csrc", "Makefile")).read(), flags=re.M).group(1)
    assert "right_view.hip" in srcs.split()
    import semstereo_amd as sa
    assert sa.right_view is sa.data.right_view and sa.lr_consistency is sa.data.lr_consistency
    assert sa.RIGHT_VIEW_KEYS == ("right_label", "right_disparity", "left_visible")


def test_the_source_only_launches():
    text = open(os.path.join(ROOT, "semstereo_amd", "csrc", "right_view.hip")).read()
    for word in ("hipMemcpy", "hipMemset", "Synchronize", "hipMalloc", "hipFree", "hipEvent", "atomicAdd", "printf", "assert(", "asm"):
        assert word not in text, word


def test_bad_arguments_are_refused_before_any_device_call():
    _l, lib = library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                               # pointers that are never followed
    nan = float("nan")

    def view(d=p, y=p, yd=1, row=16, img=256, B=1, H=16, W=16, lo=-8.0, hi=8.0, outs=(p, p, p)):
        return lib.ss_right_view_fwd(d, y, yd, row, img, B, H, W, lo, hi, -999.0, 5.0, *outs, None)

    def lr(dl=p, dr=p, B=1, H=16, W=16, lo=-8.0, hi=8.0, thr=1.0, ok=p, diff=p):
        return lib.ss_lr_consistency_fwd(dl, dr, B, H, W, lo, hi, thr, ok, diff, None)
    assert view(d=None) == -1 and view(B=0) == -1 and view(H=0) == -1 and view(W=-1) == -1
    assert view(y=None, outs=(None, None, None)) == -1                   # nothing asked for
    assert view(y=None) == -1 and view(outs=(p, None, p)) == -1          # the label and right_label come together
    assert view(yd=3) == -1 and view(yd=-1) == -1
    assert view(row=15) == -1 and view(img=255) == -1                    # label strides that would leave the tensor
    assert view(lo=8.0, hi=8.0) == -1 and view(lo=9.0) == -1 and view(lo=nan) == -1 and view(hi=nan) == -1
    assert view(W=8193, row=8193, img=16 * 8193) == -2                   # 32 KB of owners
    assert view(B=1 << 11, H=1 << 10, W=1 << 10, row=1 << 10, img=1 << 20) == -2         # 2^31 elements
    assert view(B=1 << 16, H=1 << 15, W=1, row=1, img=1 << 15) == -2     # 2^31 rows
    assert view(W=8193, row=8193, img=16 * 8193, lo=nan) == -1           # -1 comes first
    assert lr(dl=None) == -1 and lr(dr=None) == -1 and lr(B=0) == -1 and lr(H=-3) == -1 and lr(W=0) == -1
    assert lr(ok=None, diff=None) == -1
    assert lr(thr=-0.5) == -1 and lr(thr=nan) == -1
    assert lr(lo=8.0) == -1 and lr(lo=nan) == -1 and lr(hi=nan) == -1
    assert lr(B=1 << 11, H=1 << 10, W=1 << 10) == -2


# 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.CASES))
def test_consistency_equals_the_restatement(sa, name):
    d, _, lo, hi, _ = rc.case(name)
    dr = rc.right_estimate(name)
    before = dict(sa.modules.PATH_COUNTS)
    for thr in (0.0, 0.25, 1.0):
        ok, diff = sa.lr_consistency(d, dr, threshold=thr, disp_range=(lo, hi), return_diff=True)
        want_ok, want_diff = rc.restate_lr(d, dr, lo, hi, thr)
        assert ok.dtype == torch.bool and diff.dtype == torch.float32
        assert torch.equal(ok, want_ok) and torch.equal(diff, want_diff), (name, thr)
        assert torch.equal(sa.lr_consistency(d, dr, threshold=thr, maxdisp=rc.CASES[name][3]), want_ok)
    assert moved(sa, before, "data_torch") == 6 and moved(sa, before, "data_hip") == 0
    assert 0 < int(want_ok.sum()) < want_ok.numel() and bool(torch.isinf(want_diff).any()) and bool((want_diff == 0.25).any())


@pytest.mark.parametrize("name", list(rc.CASES))
def test_consistency_against_the_own_right_view(sa, name):
    """With dR = the right view of dL: a visible pixel reads its own disparity back (diff 0); a landing pixel that lost its column
    reads the owner's; diff is +inf exactly where the pixel does not land (an owned column always holds a valid value)."""
    d, _, lo, hi, want = rc.case(name)
    ok, diff = sa.lr_consistency(d, want["right_disparity"], threshold=0.0, disp_range=(lo, hi), return_diff=True)
    vis = want["left_visible"]
    assert bool(ok[vis].all()) and bool((diff[vis] == 0).all())
    W = d.shape[-1]
    x = torch.arange(W).view(1, 1, W)
    t = torch.round(x.float() - d)
    lands = (d >= lo) & (d < hi) & (t >= 0) & (t < W)
    assert torch.equal(torch.isinf(diff), ~lands)
    hidden = lands & ~vis
    assert bool(hidden.any())
    tt = torch.where(lands, t, torch.zeros_like(t)).long()
    owner_d = want["right_disparity"].gather(2, tt)                     # d[owner] of the column x aims at
    assert torch.equal(diff[hidden], (d - owner_d).abs()[hidden])
    assert torch.equal(ok, lands & (diff <= 0))
