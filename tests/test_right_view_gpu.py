"""right_view and lr_consistency on the HIP kernels (csrc/right_view.hip): every case of tests/right_view_cases.py against the sequential
restatement and against the PyTorch composition on the same device, every element written, each output alone, repeatability, no host
wait, routing, one full-size batch and DeviceLoader.  Run on the MI355X box: pytest -m gpu.

Every comparison is torch.equal: the outputs are selections, one fp32 subtraction or one comparison, and the owners are an integer
maximum, so the kernels, the composition and the restatement agree bit for bit and no tolerance appears.

No host wait: the calls run under torch.cuda.set_sync_debug_mode("error"), which raises on a synchronising call of torch; the library's
own launches are outside its view, and csrc/right_view.hip holds no synchronising or copying call (tests/test_right_view.py reads it)."""
import math
import os

import pytest
import torch

import right_view_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return semstereo_amd


class counted:
    """The calls inside make `hip` calls on the kernels and `torch_` on the composition."""

    def __init__(self, sa, hip, torch_=0):
        self.sa, self.hip, self.torch = sa, hip, torch_

    def __enter__(self):
        self.before = dict(self.sa.modules.PATH_COUNTS)

    def __exit__(self, *exc):
        if exc[0] is None:
            torch.cuda.synchronize()
            pc = self.sa.modules.PATH_COUNTS
            assert pc.get("data_hip", 0) == self.before.get("data_hip", 0) + self.hip, "data_hip"
            assert pc.get("data_torch", 0) == self.before.get("data_torch", 0) + self.torch, "data_torch"
            assert pc["hip"] == self.before["hip"] and pc["torch"] == self.before["torch"]


class composition:
    """engine.DATA_HIP off inside: what SS_DATA_HIP=0 sets."""

    def __init__(self, sa):
        self.sa = sa

    def __enter__(self):
        self.was, self.sa.engine.DATA_HIP = self.sa.engine.DATA_HIP, False

    def __exit__(self, *exc):
        self.sa.engine.DATA_HIP = self.was


def same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert got[k].is_cuda and got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        g, w = got[k].cpu(), want[k].cpu()
        assert torch.equal(g, w), f"{what} {k}: {(g != w).sum().item()} of {w.numel()} values differ"


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.CASES))
def test_cases_equal_the_restatement_and_the_composition(sa, name):
    d, y, lo, hi, want = rc.case(name)
    maxdisp = rc.CASES[name][3]
    dc, yc = d.cuda(), y.cuda()
    kernel = name in rc.KERNEL_CASES                                    # W = 8200 takes the composition, silently
    with counted(sa, 1 if kernel else 0, 0 if kernel else 1):
        got = sa.right_view(dc, yc, maxdisp=maxdisp)
    assert tuple(got) == sa.RIGHT_VIEW_KEYS and got["left_visible"].dtype == torch.bool
    same(got, want, name)
    with composition(sa), counted(sa, 0, 1):
        comp = sa.right_view(dc, yc, maxdisp=maxdisp)
    same(got, comp, name + " against the composition")
    same(comp, want, name + ", the composition on the device")


@pytest.mark.parametrize("form", rc.closed_forms(), ids=lambda f: f[0])
def test_closed_forms(sa, form):
    what, d, y, maxdisp, rd, rl, vis = form
    with counted(sa, 1):
        got = sa.right_view(d.cuda(), y.cuda(), maxdisp=maxdisp)
    same(got, {"right_disparity": rd, "right_label": rl, "left_visible": vis}, what)


@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8, torch.float32])
def test_label_dtypes_and_a_column_slice(sa, dtype):
    d, y, lo, hi, want = rc.case("batch_w37")
    wide = torch.cat([y + 1, y, y + 2], dim=2).to(dtype).cuda()
    crop = wide[:, :, 37:74]                                            # row stride 111, first pixel at an odd offset: read in place
    with counted(sa, 2):
        a = sa.right_view(d.cuda(), crop, maxdisp=8)
        b = sa.right_view(d.cuda(), y.to(dtype).cuda(), disp_range=(lo, hi), want=("right_label",))
    same(a, want, f"{dtype} slice")
    same(b, {"right_label": want["right_label"]}, f"{dtype}")
    with counted(sa, 0, 2):                                             # what the kernel does not take: the composition, silently
        c = sa.right_view(d.cuda().double(), crop, maxdisp=8)
        e = sa.right_view(d.cuda(), wide[:, :, 1::3], maxdisp=8)        # a label whose rows are not contiguous
    same(c, want, "float64")
    same(e, rc.restate(d, wide[:, :, 1::3].cpu(), lo, hi), "strided label")


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.KERNEL_CASES)
def test_every_element_is_written_and_each_output_alone(sa, name, monkeypatch):
    """torch.empty is made to hand out memory pre-filled with NaN / 0xFF, and each output is asked for alone (the others NULL)."""
    d, y, lo, hi, want = rc.case(name)
    dc, yc = d.cuda(), y.cuda()
    empty = torch.empty

    def poisoned(*args, **kwargs):
        t = empty(*args, **kwargs)
        return t.fill_(True) if t.dtype == torch.bool else t.fill_(float("nan")) if t.is_floating_point() else t
    monkeypatch.setattr(torch, "empty", poisoned)
    probe = torch.empty((2, 3), dtype=torch.float32, device="cuda")
    assert bool(torch.isnan(probe).all())
    with counted(sa, 4):
        whole = sa.right_view(dc, yc, maxdisp=rc.CASES[name][3])
        alone = {k: sa.right_view(dc, yc if k == "right_label" else None, maxdisp=rc.CASES[name][3], want=(k,)) for k in sa.RIGHT_VIEW_KEYS}
    monkeypatch.undo()
    same(whole, want, name)
    assert not bool(torch.isnan(whole["right_disparity"]).any()) and not bool(torch.isnan(whole["right_label"]).any())
    for k, got in alone.items():
        same(got, {k: want[k]}, f"{name}, {k} alone")


def test_two_calls_give_the_same_bits_and_nothing_waits(sa):
    d, y, lo, hi, want = rc.case("trips_w1030")
    dc, yc, dr = d.cuda(), y.cuda(), rc.right_estimate("trips_w1030").cuda()
    sa.right_view(dc, yc, maxdisp=48)                                   # (library load)
    torch.cuda.synchronize()
    with counted(sa, 4):
        torch.cuda.set_sync_debug_mode("error")
        try:
            a, b = sa.right_view(dc, yc, maxdisp=48), sa.right_view(dc, yc, maxdisp=48)
            p, q = (sa.lr_consistency(dc, dr, 0.25, maxdisp=48, return_diff=True) for _ in range(2))
        finally:
            torch.cuda.set_sync_debug_mode("default")
    for k in a:
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
    assert torch.equal(p[0], q[0]) and torch.equal(p[1].view(torch.int32), q[1].view(torch.int32))
    with composition(sa), counted(sa, 0, 2):
        torch.cuda.set_sync_debug_mode("error")
        try:
            c = sa.right_view(dc, yc, maxdisp=48)
            r = sa.lr_consistency(dc, dr, 0.25, maxdisp=48, return_diff=True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    same(a, c, "against the composition")
    assert torch.equal(p[0], r[0]) and torch.equal(p[1], r[1])


# 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full():
    """4 x 1024 x 1024 on the device: a smooth field plus steps, on the half-pixel grid so that collisions and exact halves are
    frequent, with no-data columns; and a label map."""
    g = torch.Generator().manual_seed(9400)
    yy, xx = torch.meshgrid(torch.arange(1024.0), torch.arange(1024.0), indexing="ij")
    maps = []
    for b in range(4):
        smooth = 20 * torch.sin(xx / (37.0 + 9 * b)) * torch.cos(yy / 61.0) + 0.01 * (b + 1) * xx
        steps = 14.0 * ((xx // (96 + 32 * b)) % 3) - 14.0
        maps.append(torch.round(2 * (smooth + steps)) / 2)
    d = torch.stack(maps)
    d[:, :, 10::11] = -999.0
    d[:, 5::97] += 0.25                                                 # some rows off the half-pixel grid
    label = torch.randint(0, 6, (4, 1024, 1024), generator=g, dtype=torch.uint8)
    return d.cuda(), label.cuda()


def test_full_size_equals_the_composition(sa, full):
    d, y = full
    with counted(sa, 1):
        got = sa.right_view(d, y, maxdisp=48)
    with composition(sa), counted(sa, 0, 1):
        want = sa.right_view(d, y, maxdisp=48)
    same(got, want, "4x1024x1024")
    share = got["left_visible"].float().mean().item()
    print(f"4x1024x1024: visible share {share:.3f}, holes {(got['right_disparity'] == -999).float().mean().item():.3f}")
    assert 0.0 < share < 1.0
    # every third column of the right map half a pixel off; the wider range keeps a moved value valid, so a visible pixel reads its own
    # disparity back to within the threshold
    dr = got["right_disparity"] + 0.5 * (torch.arange(1024, device="cuda") % 3 == 0)
    with counted(sa, 1):
        ok, diff = sa.lr_consistency(d, dr, threshold=0.5, maxdisp=64, return_diff=True)
    with composition(sa), counted(sa, 0, 1):
        want_ok, want_diff = sa.lr_consistency(d, dr, threshold=0.5, maxdisp=64, return_diff=True)
    assert torch.equal(ok, want_ok) and torch.equal(diff, want_diff)
    assert bool(ok[got["left_visible"]].all()) and 0 < int(ok.sum()) < ok.numel()


# 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.CASES))
def test_consistency_equals_the_restatement_and_the_composition(sa, name):
    d, _, lo, hi, _ = rc.case(name)
    dr = rc.right_estimate(name)
    dc, drc = d.cuda(), dr.cuda()
    for thr in (0.0, 0.25):
        want_ok, want_diff = rc.restate_lr(d, dr, lo, hi, thr)
        with counted(sa, 3):                                            # (no width limit here: W = 8200 runs the kernel too)
            ok, diff = sa.lr_consistency(dc, drc, threshold=thr, disp_range=(lo, hi), return_diff=True)
            only = sa.lr_consistency(dc, drc, threshold=thr, maxdisp=rc.CASES[name][3])             # diff NULL
            one = sa.lr_consistency(dc[0], drc[0], threshold=thr, disp_range=(lo, hi))
        assert ok.is_cuda and ok.dtype == torch.bool and diff.dtype == torch.float32
        assert torch.equal(ok.cpu(), want_ok) and torch.equal(diff.cpu(), want_diff), (name, thr)
        assert torch.equal(only, ok) and torch.equal(one, ok[0])
        with composition(sa), counted(sa, 0, 1):
            c_ok, c_diff = sa.lr_consistency(dc, drc, threshold=thr, disp_range=(lo, hi), return_diff=True)
        assert torch.equal(ok, c_ok) and torch.equal(diff, c_diff), (name, thr)


def test_consistency_writes_every_element(sa, monkeypatch):
    d, _, lo, hi, _ = rc.case("trips_w1030")
    dr = rc.right_estimate("trips_w1030")
    want_ok, want_diff = rc.restate_lr(d, dr, lo, hi, 0.25)
    empty = torch.empty

    def poisoned(*args, **kwargs):
        t = empty(*args, **kwargs)
        return t.fill_(True) if t.dtype == torch.bool else t.fill_(float("nan")) if t.is_floating_point() else t
    monkeypatch.setattr(torch, "empty", poisoned)
    with counted(sa, 1):
        ok, diff = sa.lr_consistency(d.cuda(), dr.cuda(), threshold=0.25, disp_range=(lo, hi), return_diff=True)
    monkeypatch.undo()
    assert torch.equal(ok.cpu(), want_ok) and torch.equal(diff.cpu(), want_diff) and not bool(torch.isnan(diff).any())
    assert math.isinf(float(diff.max()))


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_device_loader_delivers_the_new_keys(sa):
    batches = []
    for i in range(3):
        g = torch.Generator().manual_seed(9500 + i)
        raw = {"left_u8": torch.randint(0, 256, (2, 32, 48, 3), generator=g, dtype=torch.uint8),
               "right_u8": torch.randint(0, 256, (2, 32, 48, 3), generator=g, dtype=torch.uint8),
               "disparity": torch.round(2 * (24 * torch.rand(2, 32, 48, generator=g) - 12)) / 2,
               "label": torch.randint(0, 6, (2, 32, 48), generator=g, dtype=torch.uint8)}
        batches.append({k: v.pin_memory() for k, v in raw.items()})
    keys = ("left", "right", "disparity", "disparity_4", "label") + sa.RIGHT_VIEW_KEYS
    with counted(sa, 3 * 3):                                            # views, pyramid and right view per batch
        got = [{k: v.clone() for k, v in s.items()} for s in sa.DeviceLoader(batches, keys=keys, training=True, maxdisp=8)]
    assert len(got) == 3
    for s, raw in zip(got, batches):
        assert tuple(s) == keys and all(v.is_cuda for v in s.values())
        want = rc.restate(raw["disparity"], raw["label"], -8.0, 8.0)
        same({k: s[k] for k in sa.RIGHT_VIEW_KEYS}, want, "DeviceLoader")
        assert s["left_visible"].dtype == torch.bool
    noc = sa.disparity_metrics([got[0]["disparity"] + 0.5], got[0]["disparity"], maxdisp=8, mask_img=got[0]["left_visible"])
    assert float(noc[0, 0]) == 0.5                                      # the mask is accepted as it comes: EPE over the visible pixels
