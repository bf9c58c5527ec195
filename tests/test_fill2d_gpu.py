"""fill_disparity / refine_disparity with axes="both" on the HIP kernels (csrc/disparity_fill2d.hip): every case of tests/fill2d_cases.py
against the sequential restatement and against the PyTorch composition on the same device, the closed forms, the label dtypes, every
element written, each output alone, repeatability, no host wait, routing, one full-size batch and SceneStereo(refine=dict(axes="both")).
Run on the MI355X box: pytest -m gpu.

Every comparison is torch.equal (the disparities by their bits): the outputs are selections or comparisons and the scans are integer
selections, so the kernels, the composition and the restatement agree bit for bit and no tolerance appears.

No host wait: the calls run under torch.cuda.set_sync_debug_mode("error"), which raises on a synchronising call of torch; the library's
own launches are outside its view, and csrc/disparity_fill2d.hip holds no synchronising or copying call (tests/test_fill2d.py reads it)."""
import os

import pytest
import torch

import fill2d_cases as f2
import refine_cases as fc

pytestmark = pytest.mark.gpu

COUNTERS = ("fill2d_hip", "fill2d_torch", "refine_hip", "refine_torch", "hip", "torch")


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return semstereo_amd


class counted:
    """The calls inside make `hip` axes="both" calls on the kernels and `torch_` on the composition; no other counter moves, but
    refine_hip / refine_torch by `rows` = (hip, torch)."""

    def __init__(self, sa, hip, torch_=0, rows=(0, 0)):
        self.sa, self.moves = sa, dict(zip(COUNTERS, (hip, torch_) + tuple(rows) + (0, 0)))

    def __enter__(self):
        self.before = dict(self.sa.modules.PATH_COUNTS)

    def __exit__(self, *exc):
        if exc[0] is None:
            torch.cuda.synchronize()
            pc = self.sa.modules.PATH_COUNTS
            for k, n in self.moves.items():
                assert pc.get(k, 0) == self.before.get(k, 0) + n, k


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
    f2.same({k: v.cpu() for k, v in got.items()}, {k: v.cpu() for k, v in want.items()}, what)


def cuda(t):
    return t.cuda()


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(f2.CASES))
def test_cases_equal_the_restatement_and_the_composition(sa, name):
    c = f2.case(name)
    kernel = name in f2.KERNEL_CASES                                    # H = 8193 and W = 8200 take the composition, silently
    for variant in (f2.GPU_VARIANTS[:1] if name in f2.LONG_CASES else f2.GPU_VARIANTS):
        with counted(sa, 1 if kernel else 0, 0 if kernel else 1):
            got = f2.call(sa, c, variant, move=cuda)
        assert tuple(got) == f2.keys(sa, variant)
        same(got, f2.expected(c, variant), f"{name} {variant}")
        with composition(sa), counted(sa, 0, 1):
            comp = f2.call(sa, c, variant, move=cuda)
        same(got, comp, f"{name} {variant} against the composition")


def test_one_row_equals_the_rows_call(sa):
    c = f2.case("one_row")
    for variant in f2.GPU_VARIANTS:
        with counted(sa, 1, 0, rows=(1, 0)):
            both = f2.call(sa, c, variant, move=cuda)
            rows = f2.call(sa, c, variant, want=("disparity", "kind", "source"), move=cuda, axes="rows")
        same({k: both[k] for k in rows}, rows, str(variant))


@pytest.mark.parametrize("form", f2.closed_forms(), ids=lambda f: f[0])
def test_closed_forms(sa, form):
    what, d, y, kw, out, kind, sx, sy = form
    want = {"disparity": out, "kind": kind, "source": sx, "source_row": sy}
    with counted(sa, 1):
        got = sa.fill_disparity(d.cuda(), None if y is None else y.cuda(), maxdisp=4, want=tuple(want), axes="both", **kw)
    same(got, want, what)


@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8, torch.float32])
def test_label_dtypes_and_a_column_slice(sa, dtype):
    c = f2.case("batch_37x37")
    y = c["y"].clamp(0, 255)                                            # (what every dtype can hold: -1 becomes class 0, 200 stays none)
    variant = ((True, True, None), "background", True, (5, 4))
    (d, dr), kw = fc.arguments(c, variant)
    kw.update(label=y, keep=c["keep"])
    want = f2.restate(d, dr, lo=c["lo"], hi=c["hi"], **kw)
    args = dict(threshold=f2.THRESHOLD, maxdisp=c["maxdisp"], keep=c["keep"].cuda(), max_gap=(5, 4), want=sa.REFINE_KEYS_2D, axes="both")
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
    with counted(sa, 0, 2):                                             # what the kernels do not take: the composition, silently
        e = sa.refine_disparity(d.cuda().double(), dr.cuda(), crop, **args)
        s = sa.refine_disparity(d.cuda(), dr.cuda(), wide[:, :, 1::3], **args)          # a label whose rows are not contiguous
    same(e, want, "float64")
    same(s, f2.restate(d, dr, lo=c["lo"], hi=c["hi"], **dict(kw, label=wide[:, :, 1::3].cpu())), "strided label")


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", f2.KERNEL_CASES)
def test_every_element_is_written_and_each_output_alone(sa, name, monkeypatch):
    """torch.empty is made to hand out memory pre-filled with NaN / 0xFF / -7 -- the outputs and the scratch, which is a uint8 tensor
    -- and each output is asked for alone (the others NULL)."""
    c = f2.case(name)
    variant = f2.GPU_VARIANTS[0]
    want = f2.expected(c, variant)
    dev = {k: v.cuda() if isinstance(v, torch.Tensor) else v for k, v in c.items()}
    empty = torch.empty

    def poisoned(*args, **kwargs):
        t = empty(*args, **kwargs)
        return t.fill_(True) if t.dtype == torch.bool else t.fill_(float("nan")) if t.is_floating_point() else t.fill_(-7 if t.dtype == torch.int32 else 255)
    monkeypatch.setattr(torch, "empty", poisoned)
    probe = torch.empty((2, 3), dtype=torch.float32, device="cuda")
    assert bool(torch.isnan(probe).all())
    with counted(sa, 6):
        whole = f2.call(sa, dev, variant)
        alone = {k: f2.call(sa, dev, variant, want=(k,)) for k in sa.REFINE_KEYS_2D}
    monkeypatch.undo()
    same(whole, want, name)
    assert not bool(torch.isnan(whole["disparity"]).any()) and int(whole["kind"].max()) <= 3
    assert int(whole["source"].min()) >= -1 and int(whole["source_row"].min()) >= -1
    for k, got in alone.items():
        same(got, {k: want[k]}, f"{name}, {k} alone")


def test_two_calls_give_the_same_bits_and_nothing_waits(sa):
    c = f2.case("carry_197x260")
    dev = {k: v.cuda() if isinstance(v, torch.Tensor) else v for k, v in c.items()}
    variant = f2.GPU_VARIANTS[0]
    f2.call(sa, dev, variant)                                           # (library load, the scratch query)
    torch.cuda.synchronize()
    with counted(sa, 4):
        torch.cuda.set_sync_debug_mode("error")
        try:
            a, b = f2.call(sa, dev, variant), f2.call(sa, dev, variant)
            p, q = f2.call(sa, dev, f2.GPU_VARIANTS[4]), f2.call(sa, dev, f2.GPU_VARIANTS[4])
        finally:
            torch.cuda.set_sync_debug_mode("default")
    for x, y in ((a, b), (p, q)):
        for k in x:
            assert torch.equal(x[k].view(torch.uint8), y[k].view(torch.uint8)), k
    with composition(sa), counted(sa, 0, 1):
        torch.cuda.set_sync_debug_mode("error")
        try:
            comp = f2.call(sa, dev, variant)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    same(a, comp, "against the composition")


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_full_size_equals_the_composition(sa):
    d, label = (t.cuda() for t in f2.blob_batch())
    dr = sa.right_view(d, maxdisp=48, want=("right_disparity",))["right_disparity"] + 0.5 * (torch.arange(1024, device="cuda") % 3 == 0)
    args = dict(threshold=0.25, maxdisp=64, max_gap=(256, 256), want=sa.REFINE_KEYS_2D, axes="both")
    with counted(sa, 1):
        got = sa.refine_disparity(d, dr, label, **args)
    with composition(sa), counted(sa, 0, 1):
        want = sa.refine_disparity(d, dr, label, **args)
    same(got, want, "4x1024x1024")
    with counted(sa, 0, 0, rows=(1, 0)):
        rows = sa.refine_disparity(d, dr, label, threshold=0.25, maxdisp=64, max_gap=256, want=("kind",))
    shares = f2.blob_conditions(got, rows)                              # (conditions on the fixture: checked with the composition on the CPU)
    print("4x1024x1024: kept %.3f, same class %.3f, any class %.3f, unfilled %.3f" % tuple(shares))
    with counted(sa, 1):
        fill = sa.fill_disparity(d, label, keep=got["consistent"], maxdisp=64, max_gap=(256, 256), axes="both",
                                 want=("disparity", "kind", "source", "source_row"))
    same(fill, {k: want[k] for k in fill}, "the check's own mask as keep")


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_scene_stereo_with_both_axes(sa):
    left, right = (t.cuda() for t in fc.scene_pair(96, 160, seed=11))
    args = dict(tile=(64, 64), overlap=(32, 32), batch=2)
    without = sa.SceneStereo(fc.per_pixel_model, **args)
    stereo = sa.SceneStereo(fc.per_pixel_model, refine=f2.REFINE, **args)
    before = dict(sa.modules.PATH_COUNTS)
    got = f2.check_scene(sa, stereo, without, left, right)
    assert all(v.is_cuda for v in got.values())
    pc = sa.modules.PATH_COUNTS
    assert not any(pc.get(k, 0) != before.get(k, 0) for k in pc if k.endswith("_torch")), "a composition ran"
    assert pc["fill2d_hip"] == before.get("fill2d_hip", 0) + 2 and pc["refine_hip"] == before.get("refine_hip", 0) + 1     # check_scene's calls and the scene's
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                             # nothing waits on the host
    try:
        again = stereo(left, right, want=("disparity_refined", "kind", "consistent", "disparity_right"))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for k in again:
        assert torch.equal(again[k], got[k]), k
