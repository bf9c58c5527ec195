"""CPU: fill_disparity / refine_disparity with axes="both" (semstereo_amd/refine.py; the kernels are csrc/disparity_fill2d.hip) -- the
PyTorch composition against the sequential restatement of tests/fill2d_cases.py on every case, variant and closed form, the properties
that tie the two-axis fill to the row fill, the argument errors, the ABI of the two entry points with their refusals, and
SceneStereo(refine=dict(axes="both")) around a per-pixel stand-in callable.  Every comparison is torch.equal (the disparities by
their bits): the outputs are selections or comparisons, so no tolerance appears (no GPU needed)."""
import ctypes
import os
import re

import pytest
import torch

import fill2d_cases as f2
import refine_cases as fc
from abi import ROOT, declared, library

NAME, QUERY = "ss_disparity_fill2d_fwd", "ss_disparity_fill2d_scratch"
F = f2.FILL
same = f2.same


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    return semstereo_amd


def moved(sa, before, key):
    return sa.modules.PATH_COUNTS.get(key, 0) - before.get(key, 0)


def variants_of(name):
    if name in f2.SMALL_CASES:
        return f2.VARIANTS
    return f2.GPU_VARIANTS[:1] if name in f2.LONG_CASES else f2.GPU_VARIANTS


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(f2.CASES))
def test_composition_equals_the_restatement(sa, name):
    c = f2.case(name)
    before = dict(sa.modules.PATH_COUNTS)
    for variant in variants_of(name):
        got = f2.call(sa, c, variant)
        assert tuple(got) == f2.keys(sa, variant)
        same(got, f2.expected(c, variant), f"{name} {variant}")
    assert moved(sa, before, "fill2d_torch") == len(variants_of(name)) and moved(sa, before, "fill2d_hip") == 0
    assert moved(sa, before, "refine_torch") == 0 and moved(sa, before, "refine_hip") == 0


def test_the_tile_names_the_boundary_shapes(sa):
    assert sa.refine.FILL2D_TILE == f2.TILE == (64, 256)
    rows, cols = sa.refine.FILL2D_TILE
    shapes = {k: v[1:3] for k, v in f2.CASES.items()}
    assert shapes["segment_64x9"][0] == rows and shapes["segment_65x9"][0] == rows + 1 and shapes["waves_33x5"][0] == 2 * (rows // 4) + 1
    assert shapes["carry_197x260"] == (3 * rows + 5, cols + 4) and shapes["strip_66x257"] == (rows + 2, cols + 1)
    assert shapes["tall_8192x8"][0] == 128 * rows == sa.refine.MAX_WIDTH and shapes["tall_8193x4"][0] == sa.refine.MAX_WIDTH + 1


def test_the_planted_columns_of_the_carry_case(sa):
    """Both carries cross every segment and the summary scan: with "background" and no label every hole of a planted column whose
    planted source is the least value in range takes it, however far."""
    c = f2.case("carry_197x260")
    H, lo = c["d"].shape[1], c["lo"]
    want = f2.expected(c, ((False, False, None), "background", True, None))
    col = lambda k, x: want[k][0, :, x].tolist()                                            # noqa: E731
    hole = f2.CARRY_HOLE_ROW
    assert col("disparity", f2.CARRY_TOP) == [lo] * H and col("disparity", f2.CARRY_BOTTOM) == [lo] * H       # (from row 0 / H - 1, or an equal value nearer by)
    assert col("source_row", f2.CARRY_TOP)[hole] == 0 and col("source_row", f2.CARRY_BOTTOM)[hole] == H - 1   # the row without a source: only U / D
    assert col("source", f2.CARRY_TOP)[hole] == f2.CARRY_TOP and col("kind", f2.CARRY_TOP)[hole] == 2
    assert col("source_row", f2.CARRY_TOP)[H - 1] in (0, H - 1) and col("source_row", f2.CARRY_BOTTOM)[0] in (0, H - 1)
    assert all(r == h for h, r in enumerate(col("source_row", f2.CARRY_EMPTY)) if h != hole)  # a column without a source: filled along the rows
    assert col("kind", f2.CARRY_EMPTY)[hole] == 3                                            # ... but not in the row without a source
    labelled = f2.expected(c, ((False, False, "y"), "background", False, None))              # tier 1 alone: the class-3 source in segment 0
    rows = [h for h in range(H) if h not in f2.CARRY_OTHER_ROWS and h != f2.CARRY_CLASS_ROW]
    assert all(labelled["disparity"][0, h, f2.CARRY_CLASS] == lo and labelled["kind"][0, h, f2.CARRY_CLASS] == 1 for h in rows)
    assert labelled["source_row"][0, hole, f2.CARRY_CLASS] == f2.CARRY_CLASS_ROW and labelled["source_row"][0, H - 1, f2.CARRY_CLASS] in (f2.CARRY_CLASS_ROW, H - 1)


@pytest.mark.parametrize("form", f2.closed_forms(), ids=lambda f: f[0])
def test_closed_forms(sa, form):
    what, d, y, kw, out, kind, sx, sy = form
    want = {"disparity": out, "kind": kind, "source": sx, "source_row": sy}
    same(f2.restate(d, label=y, lo=-4.0, hi=4.0, **kw), want, what + " (restatement)")
    same(sa.fill_disparity(d, y, maxdisp=4, want=tuple(want), axes="both", **kw), want, what)
    got = sa.fill_disparity(d[0], None if y is None else y[0], maxdisp=4, want=tuple(want), axes="both", **kw)
    same(got, {k: v[0] for k, v in want.items()}, what + " [H,W]")
    if what == "same_class_three_rows_up":
        today = sa.fill_disparity(d, y, maxdisp=4, want=("disparity", "kind", "source"))
        assert today["kind"][0, 3, 1] == 2 and today["disparity"][0, 3, 1] == 0.5 and today["source"][0, 3, 1] == 2


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k in f2.CASES if k not in f2.LONG_CASES])
def test_kind_never_gets_worse(sa, name):
    c = f2.case(name)
    for variant in (((True, True, "y"), "background", True, None), ((False, True, "yf"), "nearest", False, 3),
                    ((False, False, None), "background", True, 5)):
        both, rows = f2.call(sa, c, variant), f2.call(sa, c, variant, want=("disparity", "kind", "source"), axes="rows")
        assert bool((both["kind"] <= rows["kind"]).all()), variant
        kind, sx, sy, out = both["kind"], both["source"].long(), both["source_row"].long(), both["disparity"]
        H, W = kind.shape[1:]
        x, y = torch.arange(W).view(1, 1, W), torch.arange(H).view(1, H, 1)
        assert torch.equal(kind == 0, (sx == x) & (sy == y)) and torch.equal(kind == 3, sx == -1) and torch.equal(sx == -1, sy == -1)
        assert bool(((sx == x) | (sy == y) | (kind == 3)).all())                              # a value travels along a row or a column
        has = sx >= 0
        picked = c["d"].reshape(kind.shape[0], -1).gather(1, (sy.clamp(min=0) * W + sx.clamp(min=0)).reshape(kind.shape[0], -1)).view(kind.shape)
        assert torch.equal(out.view(torch.int32)[has], picked.view(torch.int32)[has]) and bool((out[~has] == F).all())
        gx, gy = f2.gaps(variant[3], H, W)
        assert bool(((sx - x).abs()[has] <= gx).all()) and bool(((sy - y).abs()[has] <= gy).all())


def test_one_row_equals_the_rows_call(sa):
    c = f2.case("one_row")
    for variant in f2.VARIANTS:
        both, rows = f2.call(sa, c, variant), f2.call(sa, c, variant, want=("disparity", "kind", "source"), axes="rows")
        same({k: both[k] for k in rows}, rows, str(variant))
        assert bool(((both["source_row"] == 0) == (both["kind"] != 3)).all())


def test_rows_is_todays_call(sa):
    c = f2.case("batch_37x37")
    for variant in (f2.GPU_VARIANTS[0], ((False, True, "yf"), "nearest", False, 3)):
        before = dict(sa.modules.PATH_COUNTS)
        plain = f2.call(sa, c, variant, want=("disparity", "kind", "source"), axes=None)
        named = f2.call(sa, c, variant, want=("disparity", "kind", "source"), axes="rows")
        same(named, plain, str(variant))
        same(plain, {k: v for k, v in fc.expected(c, variant).items() if k in plain}, str(variant) + " (the row fill's restatement)")
        assert moved(sa, before, "refine_torch") == 2 and set(sa.modules.PATH_COUNTS) - set(before) <= {"refine_torch"}


def test_the_transpose(sa):
    """fill(d.T, y.T) is the transpose of fill(d, y) with source and source_row swapped, where no tie reaches the order rule: the
    sources' values are made pairwise distinct."""
    c = f2.case("batch_37x37")
    d, y, keep = c["d"].clone(), c["y"], c["keep"]
    d[(d >= c["hi"] - 1) & (d < c["hi"])] = F                                               # (what could leave the range becomes a hole)
    inside = (d >= c["lo"]) & (d < c["hi"] - 1)
    index = torch.arange(d[0].numel(), dtype=torch.float32).view(1, *d.shape[1:])         # per image: fewer than 2048, and d is on the half-pixel grid
    d = torch.where(inside, d + index * 2.0 ** -12, d)
    for b in range(d.shape[0]):
        assert d[b][inside[b]].unique().numel() == int(inside[b].sum())
    for prefer, gap in (("background", None), ("nearest", (3, 5))):
        a = sa.fill_disparity(d, y, keep, maxdisp=8, prefer=prefer, max_gap=gap, want=sa.REFINE_KEYS_2D[:3] + ("source_row",), axes="both")
        tgap = None if gap is None else (gap[1], gap[0])
        b = sa.fill_disparity(d.transpose(1, 2).contiguous(), y.transpose(1, 2).contiguous(), keep.transpose(1, 2).contiguous(), maxdisp=8,
                              prefer=prefer, max_gap=tgap, want=sa.REFINE_KEYS_2D[:3] + ("source_row",), axes="both")
        for k, kt in (("disparity", "disparity"), ("kind", "kind"), ("source", "source_row"), ("source_row", "source")):
            assert torch.equal(a[k].view(torch.int32) if k == "disparity" else a[k], (b[kt].view(torch.int32) if k == "disparity" else b[kt]).transpose(1, 2)), (prefer, k)


def test_arguments(sa):
    c = f2.case("batch_37x37")
    d, dr, y = c["d"], c["dr"], c["y"]
    before = dict(sa.modules.PATH_COUNTS)
    for bad in (dict(axes="columns"), dict(axes=None), dict(axes="rows", max_gap=(3, 2)), dict(max_gap=[3, 2]), dict(want=("source_row",)),
                dict(axes="rows", want=("disparity", "source_row")), dict(axes="both", max_gap=0), dict(axes="both", max_gap=(3, 0)),
                dict(axes="both", max_gap=(0, 3)), dict(axes="both", max_gap=(3, 2, 1)), dict(axes="both", max_gap=(1.5, 2)),
                dict(axes="both", max_gap=-1), dict(axes="both", want=("disparity", "consistent")), dict(axes="both", prefer="far")):
        with pytest.raises(ValueError):
            sa.fill_disparity(d, y, maxdisp=8, **bad)
    for bad in (dict(axes="diagonals"), dict(max_gap=(3, 2)), dict(want=("source_row",)), dict(axes="both", max_gap=(3, 0)),
                dict(axes="both", threshold=-1.0)):
        with pytest.raises(ValueError):
            sa.refine_disparity(d, dr, y, maxdisp=8, **bad)
    assert all(moved(sa, before, k) == 0 for k in ("refine_torch", "refine_hip", "fill2d_torch", "fill2d_hip"))       # before any work
    assert sa.REFINE_KEYS == ("disparity", "kind", "source", "consistent") and sa.REFINE_KEYS_2D == sa.REFINE_KEYS + ("source_row",)
    assert sa.REFINE_KEYS_2D is sa.refine.REFINE_KEYS_2D
    # what is not an error: an integer gap holds for both axes, None is (W, H), `want` keeps the caller's order, [H,W] gives [H,W]
    want = f2.expected(c, ((True, False, "y"), "background", True, 4))
    got = sa.refine_disparity(d.double(), dr, y.to(torch.int32), threshold=f2.THRESHOLD, maxdisp=8, max_gap=(4, 4), axes="both",
                              want=("source_row", "consistent", "disparity"))
    assert tuple(got) == ("source_row", "consistent", "disparity")
    same(got, {k: want[k] for k in got}, "a pair of equal gaps, float64, int32")
    whole = f2.expected(c, ((False, False, "y"), "background", True, None))
    two = sa.fill_disparity(d[1], y[1], maxdisp=8, max_gap=(37, 37), want=("kind", "source_row"), axes="both")
    same(two, {k: whole[k][1] for k in two}, "[H,W], the gaps spelt out")
    assert tuple(sa.fill_disparity(d, maxdisp=8, axes="both")) == ("disparity", "kind")


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported(sa):
    _l, lib = library()
    decl = declared()
    for name, arity in ((NAME, 26), (QUERY, 4)):
        assert name in decl and name in _l._SIGNATURES and name in _l.EXPORTS and hasattr(lib, name)
        assert len(_l._SIGNATURES[name]) == len(decl[name][1]) == arity
    assert decl[NAME][1][:4] == ["const float*", "const float*", "const unsigned char*", "const void*"]
    assert decl[NAME][1][-8:] == ["void*", "long long", "float*", "unsigned char*", "int*", "int*", "unsigned char*", "ss_stream_t"]
    assert decl[QUERY][1] == ["int", "int", "int", "long long*"]
    assert _l.ABI_VERSION == 20 and lib.ss_abi_version() == 20          # symbols were added, nothing changed
    srcs = re.search(r"^SRCS_HIP\s*:=(.*)$", open(os.path.join(ROOT, "semstereo_amd", "csrc", "Makefile")).read(), flags=re.M).group(1)
    assert "disparity_fill2d.hip" in srcs.split() and "disparity_refine.hip" in srcs.split()


def test_the_sources_only_launch_and_share_the_row_logic():
    csrc = os.path.join(ROOT, "semstereo_amd", "csrc")
    text = open(os.path.join(csrc, "disparity_fill2d.hip")).read()
    for word in ("hipMemcpy", "hipMemset", "Synchronize", "hipMalloc", "hipFree", "hipEvent", "atomic", "printf", "assert("):
        assert word not in re.sub(r"//.*|static_assert", "", text), word                     # (comments may say "no atomics"; static_assert is the compiler's)
    rows = open(os.path.join(csrc, "disparity_refine.hip")).read()
    shared, steps = open(os.path.join(csrc, "refine_rows.h")).read(), open(os.path.join(csrc, "refine_rows_steps.inc")).read()
    for t in (text, rows):                                              # steps 2 and 3 and the choice exist once: a header and a text both include
        assert '#include "refine_rows.h"' in t and t.count('#include "refine_rows_steps.inc"') == 1 and "choose(" in t
        assert "block_scan_exclusive<" not in t and "int choose(" not in t
    assert shared.count("int choose(") == 1 and steps.count("block_scan_exclusive<") == 2
    assert '#include "right_view.h"' in text and "lr_diff(" in text and "fabsf" not in text


def test_bad_arguments_are_refused_before_any_device_call():
    _l, lib = library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                               # pointers that are never followed; 16-byte aligned or not, see below
    aligned = ctypes.c_void_p((p.value + 15) // 16 * 16)
    nan = float("nan")
    big = 1 << 40

    def fill(d=p, dr=p, keep=p, y=p, yd=1, row=16, img=256, B=1, H=16, W=16, lo=-8.0, hi=8.0, thr=1.0, gx=16, gy=16, prefer=0, fallback=1,
             scratch=aligned, nbytes=big, outs=(p, p, p, p, p)):
        return lib.ss_disparity_fill2d_fwd(d, dr, keep, y, yd, row, img, B, H, W, lo, hi, thr, gx, gy, prefer, fallback, -999.0, scratch,
                                           nbytes, *outs, None)
    assert fill(d=None) == -1 and fill(scratch=None) == -1 and fill(B=0) == -1 and fill(H=0) == -1 and fill(W=-1) == -1
    assert fill(outs=(None,) * 5) == -1                                 # nothing asked for
    assert fill(dr=None) == -1                                          # consistent needs the right map
    assert fill(yd=3) == -1 and fill(yd=-1) == -1
    assert fill(row=15) == -1 and fill(img=255) == -1                   # label strides that would leave the tensor
    assert fill(lo=8.0) == -1 and fill(lo=nan) == -1 and fill(hi=nan) == -1
    assert fill(thr=-0.5) == -1 and fill(thr=nan) == -1
    assert fill(gx=0) == -1 and fill(gy=0) == -1 and fill(prefer=2) == -1 and fill(prefer=-1) == -1 and fill(fallback=2) == -1
    need = ctypes.c_longlong(0)
    assert lib.ss_disparity_fill2d_scratch(1, 16, 16, ctypes.byref(need)) == 0 and need.value > 0
    assert fill(nbytes=need.value - 1) == -1 and fill(nbytes=0) == -1   # a scratch that is too small
    assert fill(scratch=ctypes.c_void_p(aligned.value + 8)) == -1       # ... or not 16-byte aligned
    assert fill(W=8193, row=8193, img=16 * 8193) == -2 and fill(H=8193, img=8193 * 16) == -2      # rows and columns travel as 16-bit values
    assert fill(B=1 << 11, H=1 << 10, W=1 << 10, row=1 << 10, img=1 << 20) == -2                  # 2^31 elements
    assert fill(W=8193, row=8193, img=16 * 8193, gx=0) == -1            # -1 comes first
    assert lib.ss_disparity_fill2d_scratch(1, 16, 16, None) == -1 and lib.ss_disparity_fill2d_scratch(0, 16, 16, ctypes.byref(need)) == -1
    assert lib.ss_disparity_fill2d_scratch(1, 8193, 16, ctypes.byref(need)) == -2 and lib.ss_disparity_fill2d_scratch(1, 16, 8193, ctypes.byref(need)) == -2
    assert lib.ss_disparity_fill2d_scratch(1 << 11, 1 << 10, 1 << 10, ctypes.byref(need)) == -2


def test_the_scratch_query_grows_with_the_map():
    _l, lib = library()

    def need(B, H, W):
        n = ctypes.c_longlong(0)
        assert lib.ss_disparity_fill2d_scratch(B, H, W, ctypes.byref(n)) == 0
        assert n.value % 16 == 0 and n.value >= 9 * B * H * W          # a byte and two 4-byte planes per pixel at least
        return n.value
    base = need(1, 64, 256)
    assert need(2, 64, 256) == 2 * base and need(1, 128, 256) == 2 * base and need(1, 64, 512) == 2 * base
    assert need(1, 65, 256) > base and need(1, 64, 257) > base and need(1, 1, 1) < need(1, 7, 7) < base
    assert need(1, 8192, 8192) < 12 * 8192 * 8192
    assert _l.query_bytes(QUERY, 4, 1024, 1024) == need(4, 1024, 1024)


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_scene_stereo_with_both_axes(sa):
    left, right = fc.scene_pair(150, 203)
    args = dict(tile=(64, 96), overlap=(24, 32), batch=2)
    without = sa.SceneStereo(fc.per_pixel_model, **args)
    stereo = sa.SceneStereo(fc.per_pixel_model, refine=f2.REFINE, **args)
    before = dict(sa.modules.PATH_COUNTS)
    got = f2.check_scene(sa, stereo, without, left, right)
    assert moved(sa, before, "fill2d_torch") == 2 and moved(sa, before, "refine_torch") == 1      # check_scene: its own two calls, the scene's one
    shares = [float((got["kind"] == k).float().mean()) for k in range(4)]
    print("kind shares", " ".join(f"{s:.3f}" for s in shares))
    assert shares[0] > 0 and shares[1] > 0 and shares[0] < 1
    with pytest.raises(ValueError):
        sa.SceneStereo(fc.per_pixel_model, refine=dict(maxdisp=4, axis="both"))
    # the median after it keeps reading `kind`
    smooth = sa.SceneStereo(fc.per_pixel_model, refine=dict(f2.REFINE, median=dict(radius=1)), **args)
    out = smooth(left, right, want=("disparity_refined", "kind"))
    assert torch.equal(out["kind"], got["kind"])
    kept = got["kind"] == 0
    assert torch.equal(out["disparity_refined"][kept], got["disparity_refined"][kept])
