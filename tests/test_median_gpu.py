"""median_disparity on the HIP kernel (csrc/disparity_median.hip): every case of tests/median_cases.py at both radii against the
sequential restatement and against the PyTorch composition on the same device, every element written, each output alone,
repeatability, no host wait, routing, the label dtypes, iterations, one full-size batch after the row fill and
SceneStereo(refine=dict(median=)).  Run on the MI355X box: pytest -m gpu.

Every comparison is torch.equal on the bits: the outputs are selections of the inputs' bit patterns, so the kernel, the composition
and the restatement agree bit for bit and no tolerance appears.

No host wait: the calls run under torch.cuda.set_sync_debug_mode("error"), which raises on a synchronising call of torch; the library's
own launches are outside its view, and csrc/disparity_median.hip holds no synchronising or copying call (tests/test_median.py reads it)."""
import os

import pytest
import torch

import median_cases as mc
import refine_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return semstereo_amd


class counted:
    """The calls inside make `hip` median calls on the kernel and `torch_` on the composition, and no refine call."""

    def __init__(self, sa, hip, torch_=0):
        self.sa, self.hip, self.torch = sa, hip, torch_

    def __enter__(self):
        self.before = dict(self.sa.modules.PATH_COUNTS)

    def __exit__(self, *exc):
        if exc[0] is None:
            torch.cuda.synchronize()
            pc = self.sa.modules.PATH_COUNTS
            assert pc.get("median_hip", 0) == self.before.get("median_hip", 0) + self.hip, "median_hip"
            assert pc.get("median_torch", 0) == self.before.get("median_torch", 0) + self.torch, "median_torch"
            assert pc.get("refine_hip", 0) == self.before.get("refine_hip", 0) and pc.get("refine_torch", 0) == self.before.get("refine_torch", 0)
            assert pc["hip"] == self.before["hip"] and pc["torch"] == self.before["torch"]


class composition:
    """engine.REFINE_HIP off inside: what SS_REFINE_HIP=0 sets."""

    def __init__(self, sa):
        self.sa = sa

    def __enter__(self):
        self.was, self.sa.engine.REFINE_HIP = self.sa.engine.REFINE_HIP, False

    def __exit__(self, *exc):
        self.sa.engine.REFINE_HIP = self.was


class no_host_wait:
    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")


def same(got, want, what):
    assert all(v.is_cuda for v in got.values()), what
    mc.same({k: v.cpu() for k, v in got.items()}, {k: v.cpu() for k, v in want.items()}, what)


def cuda(t):
    return t.cuda()


def on_device(c):
    return {k: v.cuda() for k, v in c.items()}


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", mc.RADII)
@pytest.mark.parametrize("name", list(mc.CASES))
def test_cases_equal_the_restatement_and_the_composition(sa, name, radius):
    c = mc.case(name)
    dev = on_device(c)
    mc.call(sa, dev, mc.GPU_VARIANTS[0], radius)                         # (library load)
    for variant in mc.GPU_VARIANTS:
        with counted(sa, 1), no_host_wait():
            got = mc.call(sa, dev, variant, radius)
        assert tuple(got) == sa.MEDIAN_KEYS
        same(got, mc.expected(c, variant, radius), f"{name} r={radius} {variant}")
        with composition(sa), counted(sa, 0, 1), no_host_wait():
            comp = mc.call(sa, dev, variant, radius)
        same(got, comp, f"{name} r={radius} {variant} against the composition")


@pytest.mark.parametrize("form", mc.closed_forms(), ids=lambda f: f[0])
def test_closed_forms(sa, form):
    what, d, y, kw, out, count = form
    with counted(sa, 1):
        got = sa.median_disparity(d.cuda(), None if y is None else y.cuda(), maxdisp=4, radius=1, want=sa.MEDIAN_KEYS, **kw)
    same(got, {"disparity": out, "count": count}, what)


@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8, torch.float32])
def test_label_dtypes_and_a_column_slice(sa, dtype):
    c = mc.case("batch_minus_one")
    d, where = c["d"], c["where"]
    W = d.shape[-1]
    y = c["y"].clamp(0, 255)                                            # (what every dtype can hold: -1 becomes class 0, 200 stays none)
    kw = dict(radius=2, same_class=True, fill_holes=True, min_count=2)
    want = mc.restate(d, label=y, where=where, **kw)
    args = dict(disp_range=(mc.LO, mc.HI), where=where.cuda(), want=sa.MEDIAN_KEYS, **kw)
    wide = torch.cat([y + 1, y, y + 2], dim=2).to(dtype).cuda()
    crop = wide[:, :, W:2 * W]                                          # row stride 3 W, first pixel at an odd offset: read in place
    assert crop.stride(1) == 3 * W and not crop.is_contiguous()
    with counted(sa, 3):
        a = sa.median_disparity(d.cuda(), crop, **args)
        b = sa.median_disparity(d.cuda(), y.to(dtype).cuda(), **args)
        u = sa.median_disparity(d.cuda(), y.to(dtype).cuda(), **dict(args, where=where.to(torch.uint8).cuda()))
    same(a, want, f"{dtype} slice")
    same(b, want, f"{dtype}")
    same(u, want, f"{dtype}, a uint8 mask")
    with counted(sa, 0, 3):                                             # what the kernel does not take: the composition, silently
        e = sa.median_disparity(d.cuda().double(), crop, **args)
        s = sa.median_disparity(d.cuda(), wide[:, :, 1::3], **args)     # a label whose rows are not contiguous
        r3 = sa.median_disparity(d.cuda(), crop, **dict(args, radius=3))
    same(e, want, "float64")
    same(s, mc.restate(d, label=wide[:, :, 1::3].cpu(), where=where, **kw), "strided label")
    same(r3, mc.restate(d, label=y, where=where, **dict(kw, radius=3)), "radius 3")


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", mc.RADII)
@pytest.mark.parametrize("name", list(mc.CASES))
def test_every_element_is_written_and_each_output_alone(sa, name, radius, monkeypatch):
    """torch.empty is made to hand out memory pre-filled with NaN / 0xFF, and each output is asked for alone (count: NULL or not)."""
    c = mc.case(name)
    variant = mc.GPU_VARIANTS[0]
    want = mc.expected(c, variant, radius)
    dev = on_device(c)
    empty = torch.empty

    def poisoned(*args, **kwargs):
        t = empty(*args, **kwargs)
        return t.fill_(float("nan")) if t.is_floating_point() else t.fill_(255)
    monkeypatch.setattr(torch, "empty", poisoned)
    probe = torch.empty((2, 3), dtype=torch.float32, device="cuda")
    assert bool(torch.isnan(probe).all())
    with counted(sa, 3):
        whole = mc.call(sa, dev, variant, radius)
        alone = {k: mc.call(sa, dev, variant, radius, want=(k,)) for k in sa.MEDIAN_KEYS}
    monkeypatch.undo()
    same(whole, want, f"{name} r={radius}")
    assert int(whole["count"].max()) <= (2 * radius + 1) ** 2
    assert torch.equal(torch.isnan(whole["disparity"]).cpu(), torch.isnan(want["disparity"]))
    for k, got in alone.items():
        assert tuple(got) == (k,)
        same(got, {k: want[k]}, f"{name} r={radius}, {k} alone")


def test_two_calls_give_the_same_bits_and_the_input_stays(sa):
    name, variant = mc.TWICE
    c = mc.case(name)
    dev = on_device(c)
    before = dev["d"].clone()
    for radius in mc.RADII:
        with counted(sa, 3), no_host_wait():
            a, b = mc.call(sa, dev, variant, radius), mc.call(sa, dev, variant, radius)
            three = mc.call(sa, dev, variant, radius, iterations=3)      # three launches between two buffers, one count
        for k in a:
            assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
        assert torch.equal(dev["d"].view(torch.int32), before.view(torch.int32))           # the caller's tensor is never written
        assert three["disparity"].data_ptr() != dev["d"].data_ptr()
        same(three, mc.expected(c, variant, radius, iterations=3), f"{name} r={radius} three iterations")
        with counted(sa, 1):
            two = mc.call(sa, dev, variant, radius, iterations=2)
        same(two, mc.expected(c, variant, radius, iterations=2), f"{name} r={radius} two iterations")


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_full_size_after_the_row_fill_equals_the_composition(sa):
    d, label = (t.cuda() for t in mc.full_batch())
    fill =sa.fill_disparity(d, label, maxdisp=64, max_gap=256)
    where = fill["kind"] != 0
    args = dict(label=label, where=where, maxdisp=64, fill_holes=True, want=sa.MEDIAN_KEYS)
    for radius in mc.RADII:
        with counted(sa, 1), no_host_wait():
            got = sa.median_disparity(fill["disparity"], radius=radius, **args)
        with composition(sa), counted(sa, 0, 1):
            want = sa.median_disparity(fill["disparity"], radius=radius, **args)
        same(got, want, f"2x1024x1024 r={radius}")
        kept = ~where
        assert torch.equal(got["disparity"].view(torch.int32)[kept], fill["disparity"].view(torch.int32)[kept])       # kind == 0: unchanged
        assert not bool(got["count"][kept].any())
        changed = float((got["disparity"].view(torch.int32) != fill["disparity"].view(torch.int32)).float().mean())
        unfilled = float(((fill["kind"] == 3) & (got["count"] > 0)).float().mean())
        print(f"2x1024x1024 r={radius}: {changed:.4f} of the pixels moved, {unfilled:.4f} were unfilled by the row fill and are filled now")
        assert changed > 0 and unfilled > 0                             # (a condition on the fixture: rows without a source exist)


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_scene_stereo_with_median(sa):
    left, right = (t.cuda() for t in fc.scene_pair(96, 160, seed=11))
    args = dict(tile=(64, 64), overlap=(32, 32), batch=2)
    stereo = sa.SceneStereo(fc.per_pixel_model, refine=dict(fc.REFINE, median=mc.MEDIAN), **args)
    before = dict(sa.modules.PATH_COUNTS)
    got = mc.check_scene(sa, stereo, left, right)
    assert all(v.is_cuda for v in got.values())
    pc = sa.modules.PATH_COUNTS
    assert pc.get("median_torch", 0) == before.get("median_torch", 0) and pc.get("refine_torch", 0) == before.get("refine_torch", 0)
    assert pc["median_hip"] == before.get("median_hip", 0) + 3           # check_scene: two scene calls and its own
    assert pc["refine_hip"] == before.get("refine_hip", 0) + 2
    with no_host_wait():                                                 # nothing waits on the host
        again = stereo(left, right, want=("disparity_median", "kind"))
    for k in again:
        assert torch.equal(again[k], got[k]), k
