"""fill_disparity and refine_disparity on the HIP kernel (csrc/disparity_refine.hip): every case of tests/refine_cases.py against the
sequential restatement and against the PyTorch composition on the same device, every element written, each output alone, repeatability,
no host wait, routing, the label dtypes, one full-size batch and SceneStereo(refine=).  Run on the MI355X box: pytest -m gpu.

Every comparison is torch.equal (the disparities by their bits): the outputs are selections, one fp32 subtraction or one comparison, and
the scans are integer maxima and minima, so the kernel, the composition and the restatement agree bit for bit and no tolerance appears.

No host wait: the calls run under torch.cuda.set_sync_debug_mode("error"), which raises on a synchronising call of torch; the library's
own launches are outside its view, and csrc/disparity_refine.hip holds no synchronising or copying call (tests/test_refine.py reads it)."""
import os

import pytest
import torch

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
    """The calls inside make `hip` calls on the kernel and `torch_` on the composition."""

    def __init__(self, sa, hip, torch_=0):
        self.sa, self.hip, self.torch = sa, hip, torch_

    def __enter__(self):
        self.before = dict(self.sa.modules.PATH_COUNTS)

    def __exit__(self, *exc):
        if exc[0] is None:
            torch.cuda.synchronize()
            pc = self.sa.modules.PATH_COUNTS
            assert pc.get("refine_hip", 0) == self.before.get("refine_hip", 0) + self.hip, "refine_hip"
            assert pc.get("refine_torch", 0) == self.before.get("refine_torch", 0) + self.torch, "refine_torch"
            assert pc["hip"] == self.before["hip"] and pc["torch"] == self.before["torch"]


class composition:
    """engine.REFINE_HIP off inside: what SS_REFINE_HIP=0 sets."""

    def __init__(self, sa):
        self.sa = sa

    def __enter__(self):
        self.was, self.sa.engine.REFINE_HIP = self.sa.engine.REFINE_HIP, False

    def __exit__(self, *exc):
        self.sa.engine.REFINE_HIP = self.was


def same(got, want, what):
    assert all(v.is_cuda for v in got.values()), what
    fc.same({k: v.cpu() for k, v in got.items()}, {k: v.cpu() for k, v in want.items()}, what)


def cuda(t):
    return t.cuda()


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.CASES))
def test_cases_equal_the_restatement_and_the_composition(sa, name):
    c = fc.case(name)
    kernel = name in fc.KERNEL_CASES                                    # W = 8200 takes the composition, silently
    for variant in fc.GPU_VARIANTS:
        with counted(sa, 1 if kernel else 0, 0 if kernel else 1):
            got = fc.call(sa, c, variant, move=cuda)
        assert tuple(got) == (sa.REFINE_KEYS if variant[0][0] else sa.REFINE_KEYS[:3])
        same(got, fc.expected(c, variant), f"{name} {variant}")
        with composition(sa), counted(sa, 0, 1):
            comp = fc.call(sa, c, variant, move=cuda)
        same(got, comp, f"{name} {variant} against the composition")


@pytest.mark.parametrize("form", fc.closed_forms(), ids=lambda f: f[0])
def test_closed_forms(sa, form):
    what, d, y, kw, out, kind, src = form
    with counted(sa, 1):
        got = sa.fill_disparity(d.cuda(), None if y is None else y.cuda(), maxdisp=4, want=sa.REFINE_KEYS[:3], **kw)
    same(got, {"disparity": out, "kind": kind, "source": src}, what)


@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8, torch.float32])
def test_label_dtypes_and_a_column_slice(sa, dtype):
    c = fc.case("batch_w37")
    y = c["y"].clamp(0, 255)                                            # (what every dtype can hold: -1 becomes class 0, 200 stays none)
    variant = ((True, True, None), "background", True, None)
    (d, dr), kw = fc.arguments(c, variant)
    kw.update(label=y, keep=c["keep"])
    want = fc.restate(d, dr, lo=c["lo"], hi=c["hi"], **kw)
    args = dict(threshold=fc.THRESHOLD, maxdisp=c["maxdisp"], keep=c["keep"].cuda(), want=sa.REFINE_KEYS)
    wide = torch.cat([y + 1, y, y + 2], dim=2).to(dtype).cuda()
    crop = wide[:, :, 37:74]                                            # row stride 111, first pixel at an odd offset: read in place
    assert crop.stride(1) == 111 and not crop.is_contiguous()
    with counted(sa, 3):
        a = sa.refine_disparity(d.cuda(), dr.cuda(), crop, **args)
        b = sa.refine_disparity(d.cuda(), dr.cuda(), y.to(dtype).cuda(), **args)
        u = sa.refine_disparity(d.cuda(), dr.cuda(), y.to(dtype).cuda(), **dict(args, keep=c["keep"].to(torch.uint8).cuda()))
    same(a, want, f"{dtype} slice")
    same(b, want, f"{dtype}")
    same(u, want, f"{dtype}, a uint8 mask")
    with counted(sa, 0, 2):                                             # what the kernel does not take: the composition, silently
        e = sa.refine_disparity(d.cuda().double(), dr.cuda(), crop, **args)
        s = sa.refine_disparity(d.cuda(), dr.cuda(), wide[:, :, 1::3], **args)          # a label whose rows are not contiguous
    same(e, want, "float64")
    same(s, fc.restate(d, dr, lo=c["lo"], hi=c["hi"], **dict(kw, label=wide[:, :, 1::3].cpu())), "strided label")


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.KERNEL_CASES)
def test_every_element_is_written_and_each_output_alone(sa, name, monkeypatch):
    """torch.empty is made to hand out memory pre-filled with NaN / 0xFF / -7, and each output is asked for alone (the others NULL)."""
    c = fc.case(name)
    variant = fc.GPU_VARIANTS[0]
    want = fc.expected(c, variant)
    dev = {k: v.cuda() if isinstance(v, torch.Tensor) else v for k, v in c.items()}
    empty = torch.empty

    def poisoned(*args, **kwargs):
        t = empty(*args, **kwargs)
        return t.fill_(True) if t.dtype == torch.bool else t.fill_(float("nan")) if t.is_floating_point() else t.fill_(-7 if t.dtype == torch.int32 else 255)
    monkeypatch.setattr(torch, "empty", poisoned)
    probe = torch.empty((2, 3), dtype=torch.float32, device="cuda")
    assert bool(torch.isnan(probe).all())
    with counted(sa, 5):
        whole = fc.call(sa, dev, variant)
        alone = {k: fc.call(sa, dev, variant, want=(k,)) for k in sa.REFINE_KEYS}
    monkeypatch.undo()
    same(whole, want, name)
    assert not bool(torch.isnan(whole["disparity"]).any()) and int(whole["kind"].max()) <= 3 and int(whole["source"].min()) >= -1
    for k, got in alone.items():
        same(got, {k: want[k]}, f"{name}, {k} alone")


def test_two_calls_give_the_same_bits_and_nothing_waits(sa):
    c = fc.case("trips_w1030")
    dev = {k: v.cuda() if isinstance(v, torch.Tensor) else v for k, v in c.items()}
    variant = fc.GPU_VARIANTS[0]
    fc.call(sa, dev, variant)                                           # (library load)
    torch.cuda.synchronize()
    with counted(sa, 4):
        torch.cuda.set_sync_debug_mode("error")
        try:
            a, b = fc.call(sa, dev, variant), fc.call(sa, dev, variant)
            p, q = fc.call(sa, dev, fc.GPU_VARIANTS[1]), fc.call(sa, dev, fc.GPU_VARIANTS[1])
        finally:
            torch.cuda.set_sync_debug_mode("default")
    for x, y in ((a, b), (p, q)):
        for k in x:
            assert torch.equal(x[k].view(torch.uint8), y[k].view(torch.uint8)), k
    with composition(sa), counted(sa, 0, 1):
        torch.cuda.set_sync_debug_mode("error")
        try:
            comp = fc.call(sa, dev, variant)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    same(a, comp, "against the composition")


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_full_size_equals_the_composition(sa):
    d, label = (t.cuda() for t in fc.full_batch())
    dr = sa.right_view(d, maxdisp=48, want=("right_disparity",))["right_disparity"] + 0.5 * (torch.arange(1024, device="cuda") % 3 == 0)
    args = dict(threshold=0.25, maxdisp=64, max_gap=256, want=sa.REFINE_KEYS)
    with counted(sa, 1):
        got = sa.refine_disparity(d, dr, label, **args)
    with composition(sa), counted(sa, 0, 1):
        want = sa.refine_disparity(d, dr, label, **args)
    same(got, want, "4x1024x1024")
    shares = [float((got["kind"] == k).float().mean()) for k in range(4)]
    print("4x1024x1024: kept %.3f, same class %.3f, any class %.3f, unfilled %.3f" % tuple(shares))
    assert all(s > 0 for s in shares)                                   # (a condition on the fixture: checked with the composition on the CPU)
    with counted(sa, 1):
        fill = sa.fill_disparity(d, label, keep=got["consistent"], maxdisp=64, max_gap=256, want=sa.REFINE_KEYS[:3])
    same(fill, {k: want[k] for k in fill}, "the check's own mask as keep")


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_scene_stereo_with_refine(sa):
    left, right = (t.cuda() for t in fc.scene_pair(96, 160, seed=11))
    args = dict(tile=(64, 64), overlap=(32, 32), batch=2)
    without = sa.SceneStereo(fc.per_pixel_model, **args)
    stereo = sa.SceneStereo(fc.per_pixel_model, refine=fc.REFINE, **args)
    before = dict(sa.modules.PATH_COUNTS)
    got = fc.check_scene(sa, stereo, without, left, right)
    assert stereo.plan.origin_y == (0, 32) and stereo.plan.origin_x == (0, 32, 64, 96)
    assert all(v.is_cuda for v in got.values())
    assert sa.modules.PATH_COUNTS.get("refine_torch", 0) == before.get("refine_torch", 0)
    assert sa.modules.PATH_COUNTS.get("scene_torch", 0) == before.get("scene_torch", 0)
    assert sa.modules.PATH_COUNTS["refine_hip"] == before.get("refine_hip", 0) + 3      # check_scene: its own call, the full and the `kind` one
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                             # nothing waits on the host
    try:
        again = stereo(left, right, want=("disparity_refined", "kind", "consistent", "disparity_right"))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for k in again:
        assert torch.equal(again[k], got[k]), k
