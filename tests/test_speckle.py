"""CPU: filter_speckles (semstereo_amd/refine.py; the kernel is csrc/disparity_speckle.hip) -- the PyTorch composition against the
sequential flood fill of tests/speckle_cases.py on every case and variant, the closed forms of the cases, `where`, label dtypes and
layouts, `want`, the argument errors, the ABI of the two entry points with their refusals, and SceneStereo(refine=dict(speckle=))
around a per-pixel stand-in callable.  Every comparison is torch.equal: components and sizes are integers fixed by the definitions,
so no tolerance appears (no GPU needed)."""
import ctypes
import os
import re

import pytest
import torch

import refine_cases as fc
import speckle_cases as sc
from abi import ROOT, declared, library

NAMES = ("ss_disparity_speckle_scratch", "ss_disparity_speckle_fwd")


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    return semstereo_amd


def moved(sa, before, key):
    return sa.modules.PATH_COUNTS.get(key, 0) - before.get(key, 0)


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.CASES)
def test_composition_equals_the_restatement(sa, name):
    c = sc.case(name)
    before = dict(sa.modules.PATH_COUNTS)
    for variant in sc.variants(c):
        got = sc.call(sa, c, variant)
        assert tuple(got) == sa.SPECKLE_KEYS
        sc.same(got, sc.expected(c, variant), f"{name} {variant}")
    assert moved(sa, before, "speckle_torch") == len(sc.variants(c)) and moved(sa, before, "speckle_hip") == 0
    assert all(moved(sa, before, k) == 0 for k in sa.modules.PATH_COUNTS if not k.startswith("speckle"))
    free = sc.variants(c)[0]
    sc.closed_forms(sc.expected(c, free, where=None), name)
    sc.closed_forms(sc.call(sa, c, free, where=None), name)


def test_what_max_size_removes(sa):
    c = sc.case("checkerboard")
    assert bool(sc.call(sa, c, (True, 1))["speckle"].all()) and not bool(sc.call(sa, c, (True, 0))["speckle"].any())
    c = sc.case("constant_4x4_tiles")
    n = c["d"].numel()
    everything, nothing = sc.call(sa, c, (True, n)), sc.call(sa, c, (True, n - 1))
    assert bool(everything["speckle"].all()) and bool((everything["disparity"] == sc.FILL).all())
    assert not bool(nothing["speckle"].any()) and torch.equal(nothing["disparity"].view(torch.int32), c["d"].view(torch.int32))     # -0.0 stays -0.0
    c = sc.case(sc.RAGGED)
    out = sc.call(sa, c, (True, 7))
    d, kept = c["d"], ~out["speckle"]
    assert torch.equal(out["disparity"].view(torch.int32)[kept], d.view(torch.int32)[kept])                 # a NaN, a -999 pass through
    assert bool(torch.isnan(out["disparity"][0, 0, 0])) and out["size"][0, 0, 0] == 0 and out["component"][0, 0, 0] == -1
    assert out["component"][0, 0, 3:6].tolist() == [3, 3, 3] and int(out["size"][0, 0, 3]) >= 3             # -0.0, 0.0, -0.0: one run
    assert out["size"][0, 0, 7] == 0 and out["size"][0, 0, 8] >= 2                                          # hi is not valid, lo is
    assert torch.equal(out["speckle"], c["where"] & (out["size"] > 0) & (out["size"] <= 7))
    agnostic = sc.call(sa, c, (False, 7))
    assert bool((agnostic["size"] >= out["size"]).all()) and bool((agnostic["size"] > out["size"]).any())   # a class boundary cuts a component
    assert bool((agnostic["component"] <= out["component"]).all())


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64, torch.float32])
def test_where_label_dtypes_layouts_and_want(sa, dtype):
    c = sc.case(sc.RAGGED)
    d, where = c["d"], c["where"]
    W = d.shape[-1]
    y = c["y"]                                                          # 0 .. 8 and 255: what every dtype can hold
    kw = dict(max_diff=1.0, max_size=40, same_class=True)
    want = sc.restate(d, label=y, where=where, **kw)
    args = dict(disp_range=(sc.LO, sc.HI), want=sa.SPECKLE_KEYS, **kw)
    held = d.clone()
    sc.same(sa.filter_speckles(d, y.to(dtype), where, **args), want, f"{dtype}")
    sc.same(sa.filter_speckles(d, y.to(dtype), where.to(torch.uint8), **args), want, f"{dtype}, a uint8 mask")
    wide = torch.cat([y + 1, y, y + 2], dim=2).to(dtype)
    crop = wide[:, :, W:2 * W]                                          # a strided crop of a larger tensor
    assert not crop.is_contiguous()
    sc.same(sa.filter_speckles(d, crop, where, **args), want, f"{dtype} crop")
    sc.same(sa.filter_speckles(d.double(), y.to(dtype), where, **args), want, f"{dtype}, float64 disparities")
    assert torch.equal(d.view(torch.int32), held.view(torch.int32))     # the caller's tensor is never written
    for keys in (("size",), ("component", "disparity"), ("speckle",), ("disparity",)):
        got = sa.filter_speckles(d, y.to(dtype), where, **dict(args, want=keys))
        assert tuple(got) == keys
        sc.same(got, {k: want[k] for k in keys}, f"{dtype} {keys}")
    two = sa.filter_speckles(d[1], y[1].to(dtype), where[1], **args)    # [H,W] in, [H,W] out
    assert all(v.shape == d.shape[1:] for v in two.values())
    sc.same(two, {k: v[1] for k, v in want.items()}, f"{dtype} [H,W]")
    assert tuple(sa.filter_speckles(d, maxdisp=8)) == ("disparity", "speckle")
    assert not sa.filter_speckles(d.clone().requires_grad_(True), maxdisp=8)["disparity"].requires_grad


def test_arguments(sa):
    c = sc.case("random_one_tile")
    d, y, where = c["d"], c["y"], c["where"]
    nan = float("nan")
    before = dict(sa.modules.PATH_COUNTS)
    for bad in (dict(), dict(maxdisp=8, disp_range=(-8, 8)), dict(disp_range=(8, 8)), dict(disp_range=(9, 8)), dict(disp_range=(nan, 8)),
                dict(maxdisp=8, want=()), dict(maxdisp=8, want=("disparity", "kind")), dict(maxdisp=8, want=("sizes",)),
                dict(maxdisp=8, max_size=-1), dict(maxdisp=8, max_size=1.5), dict(maxdisp=8, max_size=True), dict(maxdisp=8, max_size=2 ** 31),
                dict(maxdisp=8, max_size=None), dict(maxdisp=8, max_diff=-0.5), dict(maxdisp=8, max_diff=nan), dict(maxdisp=8, max_diff=None),
                dict(maxdisp=8, max_diff=True), dict(maxdisp=8, label=y[:, :, :36]), dict(maxdisp=8, where=where[0]), dict(maxdisp=8, label=y[0])):
        with pytest.raises(ValueError):
            sa.filter_speckles(d, **bad)
    with pytest.raises(ValueError):
        sa.filter_speckles(d[0, 0], maxdisp=8)
    with pytest.raises(ValueError):
        sa.filter_speckles(d.numpy(), maxdisp=8)
    assert all(moved(sa, before, k) == 0 for k in sa.modules.PATH_COUNTS)                  # before any launch, before any work
    sc.same(sa.filter_speckles(d, y, maxdisp=8, max_size=0, max_diff=0, want=("size",)), {"size": sc.restate(d, y, max_diff=0.0)["size"]}, "max_diff 0")


# 2 ------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported(sa):
    _l, lib = library()
    decl = declared()
    for name in NAMES:
        assert name in decl and name in _l._SIGNATURES and name in _l.EXPORTS and hasattr(lib, name), name
        assert len(_l._SIGNATURES[name]) == len(decl[name][1]), name
    assert decl[NAMES[0]] == ("int", ["int", "int", "int", "long long*"])
    assert decl[NAMES[1]] == ("int", ["const float*", "const void*", "int", "long long", "long long", "const unsigned char*", "int", "int", "int",
                                      "float", "float", "float", "int", "int", "float", "void*", "long long", "float*", "unsigned char*", "int*",
                                      "int*", "ss_stream_t"])
    assert len(_l._SIGNATURES[NAMES[1]]) == 22
    assert _l.ABI_VERSION == 20 and lib.ss_abi_version() == 20          # symbols were added, nothing changed
    srcs = re.search(r"^SRCS_HIP\s*:=(.*)$", open(os.path.join(ROOT, "semstereo_amd", "csrc", "Makefile")).read(), flags=re.M).group(1)
    assert "disparity_speckle.hip" in srcs.split()
    assert sa.filter_speckles is sa.refine.filter_speckles
    assert sa.SPECKLE_KEYS == sa.refine.SPECKLE_KEYS == ("disparity", "speckle", "size", "component")
    assert sa.refine.SPECKLE_TILE in ((32, 64), (64, 64))
    assert "speckle" in sa.scene.REFINED_OUTPUTS


def test_the_source_only_launches_and_waits_for_nobody():
    text = open(os.path.join(ROOT, "semstereo_amd", "csrc", "disparity_speckle.hip")).read()
    code = re.sub(r"//[^\n]*", "", text).replace("static_assert(", "")
    for word in ("hipMemcpy", "hipMemset", "Synchronize", "hipMalloc", "hipFree", "hipEvent", "printf", "assert(", "asm", "Cooperative",
                 "grid_group", "atomicCAS", "atomicExch", "__threadfence", "volatile"):
        assert word not in code, word
    assert "float" not in " ".join(line for line in code.splitlines() if "atomic" in line)          # integer atomics only


def test_bad_arguments_are_refused_before_any_device_call():
    _l, lib = library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                               # pointers that are never followed (16-byte aligned or not: checked below)
    base = ctypes.addressof(buf)
    aligned = ctypes.c_void_p(base + (-base) % 16)
    odd = ctypes.c_void_p(aligned.value + 4)
    nan = float("nan")
    n = ctypes.c_longlong(0)
    assert lib.ss_disparity_speckle_scratch(4, 16, 16, None) == -1
    for B, H, W in ((0, 1, 1), (1, 0, 1), (1, 1, -3)):
        assert lib.ss_disparity_speckle_scratch(B, H, W, ctypes.byref(n)) == -1
    assert lib.ss_disparity_speckle_scratch(1 << 11, 1 << 10, 1 << 10, ctypes.byref(n)) == -2
    assert lib.ss_disparity_speckle_scratch(1, 16, 16, ctypes.byref(n)) == 0 and n.value >= 2 * 4 * 256 and n.value % 16 == 0
    need = n.value
    assert lib.ss_disparity_speckle_scratch(1, 3, 5, ctypes.byref(n)) == 0 and n.value >= 2 * 4 * 15 and n.value % 16 == 0
    from semstereo_amd import _lib
    assert _lib.query_bytes("ss_disparity_speckle_scratch", 1, 16, 16) == need

    def speckle(d=p, y=p, yd=1, row=16, img=256, where=p, B=1, H=16, W=16, lo=-8.0, hi=8.0, diff=1.0, size=10, same=1, ws=aligned, ws_bytes=need,
                out=p, mask=p, sizes=p, comp=p):
        return lib.ss_disparity_speckle_fwd(d, y, yd, row, img, where, B, H, W, lo, hi, diff, size, same, -999.0, ws, ws_bytes, out, mask, sizes,
                                            comp, None)
    assert speckle(d=None) == -1 and speckle(ws=None) == -1
    assert speckle(out=None, mask=None, sizes=None, comp=None) == -1     # not all of them
    assert speckle(B=0) == -1 and speckle(H=0) == -1 and speckle(W=-1) == -1
    assert speckle(yd=3) == -1 and speckle(yd=-1) == -1
    assert speckle(row=15) == -1 and speckle(img=255) == -1              # label strides that would leave the tensor
    assert speckle(lo=8.0) == -1 and speckle(lo=9.0) == -1 and speckle(lo=nan) == -1 and speckle(hi=nan) == -1
    assert speckle(diff=-1.0) == -1 and speckle(diff=nan) == -1 and speckle(size=-1) == -1
    assert speckle(same=2) == -1 and speckle(same=-1) == -1
    assert speckle(ws_bytes=need - 1) == -1 and speckle(ws=odd) == -1    # a scratch that is too small, or not 16-byte aligned
    assert speckle(B=1 << 11, H=1 << 10, W=1 << 10, row=1 << 10, img=1 << 20) == -2        # 2^31 elements
    assert speckle(B=1 << 11, H=1 << 10, W=1 << 10, row=1 << 10, img=1 << 20, size=-1) == -1           # -1 comes first


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_scene_stereo_with_speckle(sa):
    left, right = sc.blob_scene()
    before = dict(sa.modules.PATH_COUNTS)
    got = sc.check_scene(sa, fc, left, right, lambda b, k: moved(sa, b, k))
    assert moved(sa, before, "speckle_hip") == 0 and moved(sa, before, "speckle_torch") == 3          # two scene calls and check_scene's own
    assert int(got["speckle"].sum()) == 40
    with pytest.raises(AssertionError):
        sa.SceneStereo(fc.per_pixel_model, refine=fc.REFINE, **sc.SCENE_ARGS)(left, right, want=("speckle",))      # needs speckle= ...
    with pytest.raises(AssertionError):
        sa.SceneStereo(fc.per_pixel_model, **sc.SCENE_ARGS)(left, right, want=("speckle",))                         # ... inside refine=
    with pytest.raises(ValueError):
        sa.SceneStereo(fc.per_pixel_model, refine=dict(maxdisp=4, speckle=dict(max_size=3, radius=1)))
