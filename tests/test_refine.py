"""CPU: fill_disparity and refine_disparity (semstereo_amd/refine.py; the kernel is csrc/disparity_refine.hip) -- the PyTorch composition
against the sequential restatement of tests/refine_cases.py on every case, variant and closed form, the properties that tie the outputs
together and the check to lr_consistency, the argument errors, the ABI of the entry point with its refusals, and SceneStereo(refine=)
around a per-pixel stand-in callable.  Every comparison is torch.equal: the outputs are selections, one subtraction or one comparison,
so no tolerance appears (no GPU needed)."""
import ctypes
import os
import re

import pytest
import torch

import refine_cases as fc
from abi import ROOT, declared, library

NAME = "ss_disparity_refine_fwd"
F = fc.FILL


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    return semstereo_amd


def moved(sa, before, key):
    return sa.modules.PATH_COUNTS.get(key, 0) - before.get(key, 0)


same = fc.same


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.CASES))
def test_composition_equals_the_restatement(sa, name):
    c = fc.case(name)
    before = dict(sa.modules.PATH_COUNTS)
    for variant in fc.VARIANTS:
        got = fc.call(sa, c, variant)
        assert tuple(got) == (sa.REFINE_KEYS if variant[0][0] else sa.REFINE_KEYS[:3])
        same(got, fc.expected(c, variant), f"{name} {variant}")
    assert moved(sa, before, "refine_torch") == len(fc.VARIANTS) and moved(sa, before, "refine_hip") == 0
    want = fc.expected(c, ((False, True, "y"), "background", True, None))
    assert bool((want["kind"][-1, -1] == 3).all()) and bool((want["source"][-1, -1] == -1).all())     # the row without a source
    assert bool((want["disparity"][-1, -1] == F).all())
    W = c["d"].shape[-1]
    assert want["source"][0, 1].tolist() == [0] * W and float(want["disparity"][0, 1].max()) == 1.0    # the only source is x = 0 ...
    if c["d"].shape[1] >= 4:
        assert want["source"][0, 2].tolist() == [W - 1] * W and float(want["disparity"][0, 2].min()) == -1.0      # ... x = W - 1


@pytest.mark.parametrize("name", [k for k in fc.CASES if fc.CASES[k][2] >= fc.PLANT_W])
def test_the_planted_values(sa, name):
    c = fc.case(name)
    lo, hi = c["lo"], c["hi"]
    for gap in (3, None):
        variant = ((False, True, "y"), "background", True, gap)
        want = fc.expected(c, variant)
        d, kind, src = (want[k][0, 0].tolist() for k in ("disparity", "kind", "source"))
        bits = want["disparity"][0, 0].view(torch.int32).tolist()
        assert src[0:6] == [0, 0, 3, 3, 3, 5] and kind[0:6] == [0, 1, 1, 0, 1, 0]                      # ties in disparity: the nearer, then the left
        assert src[6:11] == [6, 6, 8, 8, 10] and bits[7] == bits[6] != 0 and bits[9] == 0              # -0.0 == 0.0: the left, its sign kept
        assert src[11:16] == [14] * 5 and kind[11:16] == [1, 1, 1, 0, 1] and d[11:16] == [lo] * 5      # NaN, inf, -inf; d == lo kept, d == hi not
        assert (src[17], kind[17]) == (16, 1) if gap else kind[17] == 1                                # label 5 is an ordinary class
        assert (src[19], kind[19]) == (18, 1) if gap else kind[19] == 1                                # ... and so is 7
        assert kind[20:23] == [2, 2, 2] and src[20:22] == [18, 18] and src[22] == (23 if gap else 18)  # 8, 200, -1 are no class; a none-class source
        assert (src[24], kind[24], d[24]) == (25, 1, 0.5)                                              # keep false on an in-range pixel
        if gap:
            assert src[26:35] == [26, 26, 26, 26, -1, 34, 34, 34, 34] and kind[26:35] == [0, 1, 1, 1, 3, 2, 2, 2, 0] and d[30] == F
        else:
            assert kind[26:35] == [0] + [1] * 7 + [0]                  # (from 26, or from a class-4 source further right and further back)
        same(fc.call(sa, c, variant), want, f"{name} gap {gap}")
    floats = fc.expected(c, ((False, True, "yf"), "background", True, 3))
    assert floats["kind"][0, 0, 20:23].tolist() == [2, 2, 2] and floats["source"][0, 0, 20:23].tolist() == [18, 18, 23]      # 2.5, 200.0, NaN
    free = fc.expected(c, ((False, False, "y"), "background", True, 3))
    assert free["kind"][0, 0, 24] == 0                                                                 # without the mask it is kept


@pytest.mark.parametrize("form", fc.closed_forms(), ids=lambda f: f[0])
def test_closed_forms(sa, form):
    what, d, y, kw, out, kind, src = form
    want = {"disparity": out, "kind": kind, "source": src}
    same(fc.restate(d, label=y, lo=-4.0, hi=4.0, **kw), want, what + " (restatement)")
    same(sa.fill_disparity(d, y, maxdisp=4, want=sa.REFINE_KEYS[:3], **kw), want, what)
    got = sa.fill_disparity(d[0], None if y is None else y[0], maxdisp=4, want=sa.REFINE_KEYS[:3], **kw)
    same(got, {k: v[0] for k, v in want.items()}, what + " [H,W]")
    assert all(v.dim() == 2 for v in got.values())


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.CASES))
def test_properties(sa, name):
    c = fc.case(name)
    d = c["d"]
    x = torch.arange(d.shape[-1]).view(1, 1, -1)
    for variant in (((True, True, "y"), "background", True, None), ((False, True, "yf"), "nearest", False, 3),
                    ((True, False, None), "nearest", True, 5)):
        got = fc.call(sa, c, variant)
        kind, src, out = got["kind"], got["source"].long(), got["disparity"]
        assert torch.equal(kind == 0, src == x) and torch.equal(kind == 3, src == -1), variant
        kept = kind == 0
        assert torch.equal(out.view(torch.int32)[kept], d.view(torch.int32)[kept])                     # a kept value is its input, bit for bit
        has = src >= 0
        assert torch.equal(out.view(torch.int32)[has], d.gather(2, src.clamp(min=0)).view(torch.int32)[has])
        assert bool((out[~has] == F).all()) and int(kind.max()) <= 3
        assert bool(((src - x).abs()[has] <= (variant[3] or d.shape[-1])).all())                       # nothing travels further than max_gap
        if not variant[2]:
            assert not bool((kind == 2).any())
        if variant[0][2] is None:
            assert not bool((kind == 1).any())                                                         # without a label: tier 2 only
        if variant[0][0]:
            ok = sa.lr_consistency(d, c["dr"], threshold=fc.THRESHOLD, disp_range=(c["lo"], c["hi"]))
            assert torch.equal(got["consistent"], ok) and got["consistent"].dtype == torch.bool
            assert not bool((kept & ~ok).any())                                                        # an inconsistent pixel is never kept


def test_arguments(sa):
    c = fc.case("batch_w37")
    d, dr, y = c["d"], c["dr"], c["y"]
    nan = float("nan")
    before = dict(sa.modules.PATH_COUNTS)
    for bad in (dict(maxdisp=8, prefer="foreground"), dict(maxdisp=8, max_gap=0), dict(maxdisp=8, max_gap=-2), dict(maxdisp=8, max_gap=1.5),
                dict(), dict(maxdisp=8, disp_range=(-8, 8)), dict(disp_range=(8, 8)), dict(disp_range=(9, 8)), dict(disp_range=(nan, 8)),
                dict(maxdisp=8, want=()), dict(maxdisp=8, want=("disparity", "consistent")), dict(maxdisp=8, want=("kinds",)),
                dict(maxdisp=8, label=y[:, :, :36]), dict(maxdisp=8, keep=c["keep"][0]), dict(maxdisp=8, label=y[0])):
        with pytest.raises(ValueError):
            sa.fill_disparity(d, **bad)
    for bad in (dict(threshold=-1.0), dict(threshold=nan), dict(prefer="far"), dict(max_gap=0)):
        with pytest.raises(ValueError):
            sa.refine_disparity(d, dr, y, maxdisp=8, **bad)
    with pytest.raises(ValueError):
        sa.refine_disparity(d, dr[:, :4], y, maxdisp=8)                 # shapes that differ
    with pytest.raises(ValueError):
        sa.refine_disparity(d, None, y, maxdisp=8)
    assert moved(sa, before, "refine_torch") == 0 and moved(sa, before, "refine_hip") == 0             # before any launch, before any work
    # what is not an error: other dtypes are converted, a 2-D input gives 2-D outputs, `want` keeps the caller's order
    want = fc.expected(c, ((True, False, "y"), "background", True, None))
    got = sa.refine_disparity(d.double(), dr.double(), y.to(torch.int32), threshold=fc.THRESHOLD, maxdisp=8, want=sa.REFINE_KEYS)
    same(got, want, "float64, int32")
    two = sa.refine_disparity(d[1], dr[1], y[1], threshold=fc.THRESHOLD, maxdisp=8, want=("consistent", "source", "disparity"))
    assert tuple(two) == ("consistent", "source", "disparity") and all(v.shape == d.shape[1:] for v in two.values())
    same(two, {k: want[k][1] for k in two}, "[H,W]")
    assert tuple(sa.fill_disparity(d, maxdisp=8)) == ("disparity", "kind")
    assert not sa.fill_disparity(d.clone().requires_grad_(True), maxdisp=8)["disparity"].requires_grad


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_exported(sa):
    _l, lib = library()
    decl = declared()
    assert NAME in decl and NAME in _l._SIGNATURES and NAME in _l.EXPORTS
    assert len(_l._SIGNATURES[NAME]) == len(decl[NAME][1]) == 22 and hasattr(lib, NAME)
    assert decl[NAME][1][:4] == ["const float*", "const float*", "const unsigned char*", "const void*"]
    assert decl[NAME][1][-5:] == ["float*", "unsigned char*", "int*", "unsigned char*", "ss_stream_t"]
    assert _l.ABI_VERSION == 20 and lib.ss_abi_version() == 20          # a symbol was added, nothing changed
    srcs = re.search(r"^SRCS_HIP\s*:=(.*)$", open(os.path.join(ROOT, "semstereo_amd", "csrc", "Makefile")).read(), flags=re.M).group(1)
    assert "disparity_refine.hip" in srcs.split()
    assert "REFINE_HIP" in sa.engine.SWITCHES and isinstance(sa.engine.REFINE_HIP, bool)
    assert sa.fill_disparity is sa.refine.fill_disparity and sa.refine_disparity is sa.refine.refine_disparity
    assert sa.REFINE_KEYS == ("disparity", "kind", "source", "consistent")


def test_the_source_only_launches():
    text = open(os.path.join(ROOT, "semstereo_amd", "csrc", "disparity_refine.hip")).read()
    for word in ("hipMemcpy", "hipMemset", "Synchronize", "hipMalloc", "hipFree", "hipEvent", "atomic", "printf", "assert(", "asm"):
        assert word not in text, word
    shared = open(os.path.join(ROOT, "semstereo_amd", "csrc", "right_view.hip")).read()
    for t in (text, shared):                                            # the check is one device function, defined in right_view.h
        assert '#include "right_view.h"' in t and "lr_diff(" in t and "fabsf" not in t


def test_bad_arguments_are_refused_before_any_device_call():
    _l, lib = library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                               # pointers that are never followed
    nan = float("nan")

    def refine(d=p, dr=p, keep=p, y=p, yd=1, row=16, img=256, B=1, H=16, W=16, lo=-8.0, hi=8.0, thr=1.0, gap=16, prefer=0, fallback=1,
               outs=(p, p, p, p)):
        return lib.ss_disparity_refine_fwd(d, dr, keep, y, yd, row, img, B, H, W, lo, hi, thr, gap, prefer, fallback, -999.0, *outs, None)
    assert refine(d=None) == -1 and refine(B=0) == -1 and refine(H=0) == -1 and refine(W=-1) == -1
    assert refine(outs=(None, None, None, None)) == -1                   # nothing asked for
    assert refine(dr=None) == -1                                         # consistent needs the right map
    assert refine(yd=3) == -1 and refine(yd=-1) == -1
    assert refine(row=15) == -1 and refine(img=255) == -1                # label strides that would leave the tensor
    assert refine(lo=8.0) == -1 and refine(lo=nan) == -1 and refine(hi=nan) == -1
    assert refine(thr=-0.5) == -1 and refine(thr=nan) == -1
    assert refine(gap=0) == -1 and refine(prefer=2) == -1 and refine(prefer=-1) == -1 and refine(fallback=2) == -1
    assert refine(W=8193, row=8193, img=16 * 8193) == -2                 # 9 bytes of LDS per column
    assert refine(B=1 << 11, H=1 << 10, W=1 << 10, row=1 << 10, img=1 << 20) == -2        # 2^31 elements
    assert refine(B=1 << 16, H=1 << 15, W=1, row=1, img=1 << 15) == -2   # 2^31 rows
    assert refine(W=8193, row=8193, img=16 * 8193, gap=0) == -1          # -1 comes first


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_scene_stereo_with_refine(sa):
    left, right = fc.scene_pair(150, 203)
    args = dict(tile=(64, 96), overlap=(24, 32), batch=2)
    without = sa.SceneStereo(fc.per_pixel_model, **args)
    before = dict(sa.modules.PATH_COUNTS)
    without(left, right)
    today = {k: moved(sa, before, k) for k in sa.modules.PATH_COUNTS}
    stereo = sa.SceneStereo(fc.per_pixel_model, refine=fc.REFINE, **args)
    before = dict(sa.modules.PATH_COUNTS)
    stereo(left, right)
    assert {k: moved(sa, before, k) for k in sa.modules.PATH_COUNTS} == today                          # refine= alone changes no call
    got = fc.check_scene(sa, stereo, without, left, right)
    shares = [float((got["kind"] == k).float().mean()) for k in range(4)]
    print("kind shares", " ".join(f"{s:.3f}" for s in shares))
    assert shares[0] > 0 and shares[1] > 0 and shares[0] < 1
    with pytest.raises(AssertionError):
        without(left, right, want=("disparity", "kind"))                # the new outputs need refine=
    with pytest.raises(ValueError):
        sa.SceneStereo(fc.per_pixel_model, refine=dict(maxdisp=4, gap=3))
    # without a segmentation head the fill is class-agnostic
    bare = sa.SceneStereo(lambda a, b: fc.per_pixel_model(a, b)[0], refine=fc.REFINE, **args)
    out = bare(left, right, want=("disparity_refined", "kind"))
    want = sa.refine_disparity(got["disparity"], got["disparity_right"], want=("disparity", "kind"), **fc.REFINE)
    assert torch.equal(out["disparity_refined"], want["disparity"]) and torch.equal(out["kind"], want["kind"])
    assert not bool((out["kind"] == 1).any())
