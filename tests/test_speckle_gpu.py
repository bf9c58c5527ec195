"""filter_speckles on the HIP kernels (csrc/disparity_speckle.hip): every case of tests/speckle_cases.py against the sequential flood
fill and against the PyTorch composition on the same device, every element written, each output alone, repeatability, no host wait,
routing, `where`, the label dtypes and layouts, in place at the C boundary and SceneStereo(refine=dict(speckle=)).  Run on the
MI355X box: pytest -m gpu.

Every comparison is torch.equal: components and sizes are integers fixed by the definitions whatever order the unions ran in, so the
kernel, the composition and the restatement agree exactly and no tolerance appears.

No host wait: the kernel calls run under torch.cuda.set_sync_debug_mode("error"), which raises on a synchronising call of torch; the
library's own launches are outside its view, and csrc/disparity_speckle.hip holds no synchronising or copying call
(tests/test_speckle.py reads it).  The composition is NOT run under it: it asks the host once per round."""
import os

import pytest
import torch

import refine_cases as fc
import speckle_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return semstereo_amd


def moved(sa, before, key):
    return sa.modules.PATH_COUNTS.get(key, 0) - before.get(key, 0)


class counted:
    """The calls inside make `hip` speckle calls on the kernel and `torch_` on the composition, and no other counted call."""

    def __init__(self, sa, hip, torch_=0):
        self.sa, self.hip, self.torch = sa, hip, torch_

    def __enter__(self):
        self.before = dict(self.sa.modules.PATH_COUNTS)

    def __exit__(self, *exc):
        if exc[0] is None:
            torch.cuda.synchronize()
            assert moved(self.sa, self.before, "speckle_hip") == self.hip, "speckle_hip"
            assert moved(self.sa, self.before, "speckle_torch") == self.torch, "speckle_torch"
            assert all(moved(self.sa, self.before, k) == 0 for k in self.sa.modules.PATH_COUNTS if not k.startswith("speckle"))


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
    sc.same({k: v.cpu() for k, v in got.items()}, {k: v.cpu() for k, v in want.items()}, what)


def on_device(c):
    return {k: v.cuda() if isinstance(v, torch.Tensor) else v for k, v in c.items()}


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.CASES)
def test_cases_equal_the_restatement_and_the_composition(sa, name):
    c = sc.case(name)
    variants = sc.variants(c)
    dev = on_device(c)
    sc.call(sa, dev, variants[0])                                        # (library load)
    for variant in variants:
        with counted(sa, 1), no_host_wait():
            got = sc.call(sa, dev, variant)
        assert tuple(got) == sa.SPECKLE_KEYS
        same(got, sc.expected(c, variant), f"{name} {variant}")
    for variant in (variants[0], variants[-1]):                          # (the composition does not depend on max_size before its last step)
        with counted(sa, 1):
            got = sc.call(sa, dev, variant)
        with composition(sa), counted(sa, 0, 1):
            comp = sc.call(sa, dev, variant)
        same(got, comp, f"{name} {variant} against the composition")
    with counted(sa, 1):
        free = sc.call(sa, dev, variants[0], where=None)
    sc.closed_forms({k: v.cpu() for k, v in free.items()}, name)


def test_what_max_size_removes(sa):
    dev = on_device(sc.case("checkerboard"))
    with counted(sa, 2):
        assert bool(sc.call(sa, dev, (True, 1))["speckle"].all()) and not bool(sc.call(sa, dev, (True, 0))["speckle"].any())
    c = sc.case("constant_4x4_tiles")
    dev, n = on_device(c), c["d"].numel()
    with counted(sa, 2):
        everything, nothing = sc.call(sa, dev, (True, n)), sc.call(sa, dev, (True, n - 1))
    assert bool(everything["speckle"].all()) and bool((everything["disparity"] == sc.FILL).all())
    assert bool((everything["size"] == n).all()) and bool((everything["component"] == 0).all())
    assert not bool(nothing["speckle"].any()) and torch.equal(nothing["disparity"].view(torch.int32).cpu(), c["d"].view(torch.int32))


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random_one_tile", sc.RAGGED, "thin_row", "thin_column", "one_pixel"])
def test_every_element_is_written_and_each_output_alone(sa, name, monkeypatch):
    """torch.empty is made to hand out memory pre-filled with NaN / 0xFF -- the outputs AND the scratch -- and each output is asked
    for alone: an output that is not wanted is not allocated."""
    c = sc.case(name)
    variant = sc.variants(c)[-2]
    want = sc.expected(c, variant)
    empty = torch.empty
    made = []

    def poisoned(*args, **kwargs):
        t = empty(*args, **kwargs)
        made.append((tuple(t.shape), t.dtype))
        return t.fill_(float("nan")) if t.is_floating_point() else t.fill_(255)
    dev = on_device(c)
    monkeypatch.setattr(torch, "empty", poisoned)
    with counted(sa, 1 + len(sa.SPECKLE_KEYS)):
        whole = sc.call(sa, dev, variant)
        del made[:]
        alone = {}
        for k in sa.SPECKLE_KEYS:
            alone[k] = sc.call(sa, dev, variant, want=(k,))
            assert len(made) == 2 and made[0][1] == torch.uint8 and len(made[0][0]) == 1, (k, made)       # the scratch and ONE output
            assert made[1] == (tuple(c["d"].shape), sa.refine._SPECKLE_DTYPES[k]), (k, made)
            del made[:]
    monkeypatch.undo()
    same(whole, want, name)
    for k, got in alone.items():
        assert tuple(got) == (k,)
        same(got, {k: want[k]}, f"{name}, {k} alone")


def test_two_calls_give_the_same_bits_and_the_input_stays(sa):
    c = sc.case(sc.RAGGED)
    dev = on_device(c)
    before = dev["d"].clone()
    for variant in ((True, 40), (False, 40)):
        with counted(sa, 2), no_host_wait():
            a, b = sc.call(sa, dev, variant), sc.call(sa, dev, variant)
        for k in a:
            assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
            assert a[k].data_ptr() != dev["d"].data_ptr()
        assert torch.equal(dev["d"].view(torch.int32), before.view(torch.int32))           # the caller's tensor is never written
        same(a, sc.expected(c, variant), f"{sc.RAGGED} {variant}")


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64, torch.float32])
def test_where_label_dtypes_and_layouts(sa, dtype):
    c = sc.case(sc.RAGGED)
    d, where, y = c["d"], c["where"], c["y"]
    W = d.shape[-1]
    kw = dict(max_diff=1.0, max_size=40, same_class=True)
    want = sc.restate(d, label=y, where=where, **kw)
    args = dict(disp_range=(sc.LO, sc.HI), want=sa.SPECKLE_KEYS, **kw)
    wide = torch.cat([y + 1, y, y + 2], dim=2).to(dtype).cuda()
    crop = wide[:, :, W:2 * W]                                          # row stride 3 W, first pixel at an odd offset: read in place
    assert crop.stride(1) == 3 * W and not crop.is_contiguous()
    dd, dy, dw, du = d.cuda(), y.to(dtype).cuda(), where.cuda(), where.to(torch.uint8).cuda()
    with counted(sa, 4), no_host_wait():
        a = sa.filter_speckles(dd, crop, dw, **args)
        b = sa.filter_speckles(dd, dy, dw, **args)
        u = sa.filter_speckles(dd, dy, du, **args)
        two = sa.filter_speckles(dd[1], dy[1], dw[1], **args)
    same(a, want, f"{dtype} crop")
    same(b, want, f"{dtype}")
    same(u, want, f"{dtype}, a uint8 mask")
    assert all(v.dim() == 2 for v in two.values())
    same(two, {k: v[1] for k, v in want.items()}, f"{dtype} [H,W]")
    with counted(sa, 0, 3):                                             # what the kernel does not take: the composition, silently
        e = sa.filter_speckles(d.cuda().double(), crop, where.cuda(), **args)
        s = sa.filter_speckles(d.cuda(), wide[:, :, 1::3], where.cuda(), **args)          # a label whose rows are not contiguous
        m = sa.filter_speckles(d.cuda(), crop, where.to(torch.int64).cuda(), **args)
    same(e, want, "float64")
    same(s, sc.restate(d, label=wide[:, :, 1::3].cpu(), where=where, **kw), "strided label")
    same(m, want, "an int64 mask")


def test_in_place_at_the_c_boundary(sa):
    """out_disparity == disparity is allowed (the header says so): the last pass reads nothing of the map but d[p] for p."""
    from semstereo_amd._lib import call, ptr, query_bytes
    c = sc.case(sc.RAGGED)
    variant = (True, 40)
    want = sc.expected(c, variant)
    d, y, where = c["d"].cuda(), c["y"].cuda(), c["where"].cuda().view(torch.uint8)
    B, H, W = d.shape
    nbytes = query_bytes("ss_disparity_speckle_scratch", B, H, W)
    scratch = torch.full((nbytes,), 255, dtype=torch.uint8, device="cuda")
    size = torch.full((B, H, W), -7, dtype=torch.int32, device="cuda")
    call("ss_disparity_speckle_fwd", ptr(d), ptr(y), 0, W, H * W, ptr(where), B, H, W, sc.LO, sc.HI, 1.0, 40, 1, sc.FILL, ptr(scratch), nbytes,
         ptr(d), None, ptr(size), None)
    torch.cuda.synchronize()
    same({"disparity": d, "size": size}, {k: want[k] for k in ("disparity", "size")}, "in place")


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_scene_stereo_with_speckle(sa):
    left, right = (t.cuda() for t in sc.blob_scene())
    before = dict(sa.modules.PATH_COUNTS)
    got = sc.check_scene(sa, fc, left, right, lambda b, k: moved(sa, b, k))
    assert all(v.is_cuda for v in got.values())
    assert moved(sa, before, "speckle_hip") == 3 and moved(sa, before, "speckle_torch") == 0          # two scene calls and check_scene's own
    assert moved(sa, before, "refine_torch") == 0 and moved(sa, before, "scene_torch") == 0
    stereo = sa.SceneStereo(fc.per_pixel_model, refine=dict(fc.REFINE, speckle=sc.SPECKLE), **sc.SCENE_ARGS)
    stereo(left, right, want=("speckle", "kind"))
    with no_host_wait():                                                 # nothing waits on the host
        again = stereo(left, right, want=("speckle", "kind", "disparity_refined"))
    for k in again:
        assert torch.equal(again[k], got[k]), k
