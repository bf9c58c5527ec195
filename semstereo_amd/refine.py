"""Disparity refinement: the left-right check and a hole fill that takes a hole's value from the surface it belongs to.  The
post-processing of a stereo result, acting on the mask lr_consistency produces -- with what a generic fill lacks, the predicted class
of every pixel: roof is filled from roof, ground from ground, and only then from anything.  The reference has no such step.

  fill_disparity     holes of one map (out of range, or masked by `keep`) filled row by row
  refine_disparity   the left-right check of two estimates, then the same fill of what the check rejects
  median_disparity   what follows the row fill: a 2-D median in which a pixel is smoothed only with pixels of its own class
  filter_speckles    what comes before it: small connected blobs of one class and one disparity level found and removed

CUDA tensors run csrc/disparity_refine.hip: one launch, one workgroup per row, nothing waiting on the host.  CPU tensors, other dtypes,
a label whose rows are not contiguous, rows wider than 8192 and SS_REFINE_HIP=0 take the PyTorch composition below, written without
boolean indexing and without `.item()`.  modules.PATH_COUNTS["refine_hip"] / ["refine_torch"] count the calls on each path.

The definitions (include/semstereo_hip.h, "disparity refinement", is their one full statement), per image and row:
  * source[x]: d[x] in range (lo <= d < hi, a NaN is not), and keep[x] if a mask is given, and consistent[x] if a right map is given
    (data.lr_consistency's definition, the same device function).
  * class[x]: int(v) for an integer-valued label 0 <= v < 8, none for every other value and without a label.
  * a pixel that is no source looks left and right for the nearest source of its own class within `max_gap` columns (tier 1), then --
    with `fallback` -- for the nearest source of any class (tier 2).  One side alone wins; of two, "background" takes the smaller
    disparity (the surface further from the sensor; equal values: the nearer, then the left), "nearest" the nearer (equal distances:
    the smaller disparity, then the left).
  * "disparity": d[x] bit for bit on a source, the chosen candidate's value on a filled pixel, `fill_value` elsewhere; "kind" uint8:
    0 kept, 1 filled from the same class, 2 filled from any class, 3 unfilled; "source" int32: the column the value came from, -1 on
    an unfilled pixel; "consistent" bool.
Nothing is interpolated, so the kernel and the composition agree bit for bit.

axes="both" (include/semstereo_hip.h, "disparity refinement: fill along rows and columns", is the full statement): the same fill
looking in four directions.  A pixel that is no source has up to four candidates per tier, in the order L, R (its row, within
max_gap columns), U, D (its column, within max_gap rows -- `max_gap` an integer for both or a pair (columns, rows)); "background"
takes the least (value, distance, order), "nearest" the least (distance, value, order), which with L and R alone is the rule above.
"source" is the column and "source_row" (REFINE_KEYS_2D) the row the value came from.  CUDA float32 maps up to 8192 x 8192 run
csrc/disparity_fill2d.hip -- four launches over tiles of FILL2D_TILE = 64 rows x 256 columns: classify and reduce, scan the tiles'
summaries, sweep down and up, then the row kernel's own scans and the choice; nothing waits on the host -- everything else a
composition of per-class cummax / cummin along both axes and gathers on the flattened image.  modules.PATH_COUNTS["fill2d_hip"] /
["fill2d_torch"] count these calls; axes="rows" (the default) is the call above, on the same kernel, under the same counters.  Not
built: diagonal directions, sub-pixel blending of candidates, a per-axis `prefer`, maps beyond 8192 on the kernel.

median_disparity (include/semstereo_hip.h, "disparity refinement: class-aware median", is the full statement): per pixel the lower
median of the valid pixels of its (2r + 1)^2 window that share its class (all valid pixels for a pixel of no class or with
same_class=False), in the total order of the fp32 bit patterns; border windows are smaller, nothing is padded.  A pixel is replaced
only if `where` admits it, it is valid itself or fill_holes is set, and the window holds at least min_count members; every other pixel
passes through bit for bit.  CUDA float32 tensors with radius <= 2 run csrc/disparity_median.hip (a 16 x 64 tile with its halo in
LDS, a fixed compare-exchange network per pixel), everything else a composition of shifted views and one sort of the integer keys;
modules.PATH_COUNTS["median_hip"] / ["median_torch"] count the calls.  Not built: a weighted or bilateral median, sub-pixel blending, radii above 2 on the kernel.

filter_speckles (include/semstereo_hip.h, "disparity refinement: speckle removal", is the full statement): two 4-neighbours of an
image link if both are valid, their disparities differ by at most max_diff (one fp32 subtraction) and -- with same_class -- they are
of one class (none equals none); a component is a class of the transitive closure, so a ramp 0, 1, 2, ... with max_diff = 1 is one
component.  "component" int32 is the smallest index y * W + x of a pixel's component (-1 on a pixel that is not valid), "size" int32
the number of its pixels (0), "speckle" bool: valid, size <= max_size, and admitted by `where`; "disparity" is fill_value on a speckle
and d bit for bit elsewhere.  All of it is integers fixed by the definitions: CUDA float32 tensors run csrc/disparity_speckle.hip
(union-find in LDS per 32 x 64 tile, the links across tile edges united by integer atomicMin in global memory, the tiles' counts
added up on the final roots, one pass for the outputs: four launches, nothing waiting on the host), everything else a composition
that propagates the smallest index over the four link masks with pointer jumping -- and asks the host once per round whether
anything changed: the one place in this module where the composition waits.  modules.PATH_COUNTS["speckle_hip"] /
["speckle_torch"] count the calls.  Not built: 8-connectivity, a max_diff that grows with the disparity, statistics of a component
other than its size.
"""
import numpy as np
import torch

from . import data as D
from . import engine as E
from ._host import _nograd, count
from ._lib import call, ptr, query_bytes

REFINE_KEYS = ("disparity", "kind", "source", "consistent")
REFINE_KEYS_2D = REFINE_KEYS + ("source_row",)       # what axes="both" can also name: the row the value came from
AXES = ("rows", "both")
FILL2D_TILE = (64, 256)                      # csrc/disparity_fill2d.hip: TR rows x TC columns of a workgroup; a wave owns TR / 4 rows
NUM_CLASSES = 8                              # csrc/disparity_refine.hip: classes 0 .. 7, anything else is "none"
MAX_WIDTH = 8192                             # ... and 9 bytes of LDS per column
PREFER = {"background": 0, "nearest": 1}
_DTYPES = {"disparity": torch.float32, "kind": torch.uint8, "source": torch.int32, "consistent": torch.bool, "source_row": torch.int32}
_MAX_ELEMENTS = 2 ** 31
MEDIAN_KEYS = ("disparity", "count")
MEDIAN_TILE = (16, 64)                       # csrc/disparity_median.hip: TH x TW output pixels of a workgroup
MEDIAN_MAX_RADIUS = 4                        # ... whose networks end at radius 2; 3 and 4 take the composition
_MEDIAN_KERNEL_RADIUS = 2
SPECKLE_KEYS = ("disparity", "speckle", "size", "component")
SPECKLE_TILE = (32, 64)                      # csrc/disparity_speckle.hip: TH x TW pixels of a workgroup's union-find in LDS
_SPECKLE_DTYPES = {"disparity": torch.float32, "speckle": torch.bool, "size": torch.int32, "component": torch.int32}


def _hip(*tensors):
    """The kernel takes these tensors: the switch is on and all of them are contiguous CUDA tensors on one device."""
    if not E.REFINE_HIP:
        return False
    dev = tensors[0].device
    return all(t.is_cuda and t.device == dev and t.is_contiguous() for t in tensors)


def _classes(label):
    """int64 of the label's shape: the class 0 .. 7, or NUM_CLASSES for none."""
    if label.is_floating_point():
        inside = (label >= 0) & (label < NUM_CLASSES) & (label == label.trunc())
        cls = torch.where(inside, label, torch.zeros_like(label)).long()
    else:
        cls = label.long()
        inside = (cls >= 0) & (cls < NUM_CLASSES)
    return torch.where(inside, cls, torch.full_like(cls, NUM_CLASSES))


def _nearest(mask, x, W, axis=2):
    """Per pixel the largest index x' < x and the smallest x' > x along `axis` with mask[x'] (int64 [B,H,W]; -1 and W for none): x
    the pixels' own index along that axis, W its length (axis 2: columns, axis 1: rows)."""
    left = torch.where(mask, x, torch.full_like(x, -1)).cummax(axis).values
    right = torch.where(mask, x, torch.full_like(x, W)).flip(axis).cummin(axis).values.flip(axis)
    none_l, none_r = torch.full_like(left.narrow(axis, 0, 1), -1), torch.full_like(right.narrow(axis, 0, 1), W)
    return torch.cat([none_l, left.narrow(axis, 0, W - 1)], axis), torch.cat([right.narrow(axis, 1, W - 1), none_r], axis)


def _choose(d, x, L, R, W, max_gap, prefer):
    """(a candidate exists, the winning column) of one tier."""
    has_l, has_r = (L >= 0) & (x - L <= max_gap), (R < W) & (R - x <= max_gap)
    dl, dr = d.gather(2, L.clamp(min=0)), d.gather(2, R.clamp(max=W - 1))
    gl, gr = x - L, R - x
    if prefer == 0:
        right = (dr < dl) | ((dr == dl) & (gr < gl))
    else:
        right = (gr < gl) | ((gr == gl) & (dr < dl))
    take_r = has_r & (~has_l | right)
    return has_l | has_r, torch.where(take_r, R, L)


def _sources(d, dr, keep, lo, hi, threshold):
    """(source[x] of the definitions, {"consistent": the check's map} with a right map)."""
    W = d.shape[2]
    src = (d >= lo) & (d < hi)
    if keep is not None:
        src = src & (keep != 0)
    out = {}
    if dr is not None:
        lands, t, _ = D._targets(d, lo, hi)
        m = dr.gather(2, t.clamp(max=W - 1))
        diff = torch.where(lands & (m >= lo) & (m < hi), (d - m).abs(), torch.full_like(d, float("inf")))
        out["consistent"] = diff <= threshold
        src = src & out["consistent"]
    return src, out


def _choose4(flat, cands, prefer):
    """(a candidate exists, the winner's index y* W + x*) of one tier: the least of the candidates `cands` = [(exists, index into the
    flattened image, distance)] in the order L, R, U, D, by (v, g, order) for prefer 0 and (g, v, order) for prefer 1 -- a fold in
    that order in which a later candidate wins only where it is strictly less."""
    shape = cands[0][1].shape
    has, idx, g = cands[0]
    v = flat.gather(1, idx.reshape(shape[0], -1)).view(shape)
    for has_c, idx_c, g_c in cands[1:]:
        v_c = flat.gather(1, idx_c.reshape(shape[0], -1)).view(shape)
        if prefer == 0:
            later = (v_c < v) | ((v_c == v) & (g_c < g))
        else:
            later = (g_c < g) | ((g_c == g) & (v_c < v))
        take = has_c & (~has | later)
        has, idx, g, v = has | has_c, torch.where(take, idx_c, idx), torch.where(take, g_c, g), torch.where(take, v_c, v)
    return has, idx


def _fill2d_torch(d, dr, keep, label, lo, hi, threshold, gap_x, gap_y, prefer, fallback, fill_value, want):
    """The definitions of include/semstereo_hip.h, "disparity refinement: fill along rows and columns": per class a cummax / cummin
    along both axes, gathers on the flattened image, one lexicographic four-way choice per tier."""
    B, H, W = d.shape
    x = torch.arange(W, device=d.device).view(1, 1, W).expand(B, H, W)
    y = torch.arange(H, device=d.device).view(1, H, 1).expand(B, H, W)
    src, out = _sources(d, dr, keep, lo, hi, threshold)
    if not {"disparity", "kind", "source", "source_row"} & set(want):
        return out
    flat = d.reshape(B, H * W)

    def tier(L, R, U, Dn):
        return _choose4(flat, [((L >= 0) & (x - L <= gap_x), y * W + L.clamp(min=0), x - L),
                               ((R < W) & (R - x <= gap_x), y * W + R.clamp(max=W - 1), R - x),
                               ((U >= 0) & (y - U <= gap_y), U.clamp(min=0) * W + x, y - U),
                               ((Dn < H) & (Dn - y <= gap_y), Dn.clamp(max=H - 1) * W + x, Dn - y)], prefer)
    here = y * W + x
    has1, s1 = torch.zeros_like(src), here
    if label is not None:
        cls = _classes(label)
        L, R, U, Dn = torch.full_like(x, -1), torch.full_like(x, W), torch.full_like(x, -1), torch.full_like(x, H)
        for c in range(NUM_CLASSES):                    # per class and axis a cummax / cummin; a pixel takes those of its own class
            mine = cls == c
            (l, r), (u, dn) = _nearest(src & mine, x, W), _nearest(src & mine, y, H, axis=1)
            L, R, U, Dn = torch.where(mine, l, L), torch.where(mine, r, R), torch.where(mine, u, U), torch.where(mine, dn, Dn)
        has1, s1 = tier(L, R, U, Dn)
    filled1 = ~src & has1
    if fallback:
        has2, s2 = tier(*_nearest(src, x, W), *_nearest(src, y, H, axis=1))
        filled2 = ~src & ~has1 & has2
    else:
        filled2, s2 = torch.zeros_like(src), s1
    index = torch.where(src, here, torch.where(filled1, s1, torch.where(filled2, s2, torch.full_like(x, -1))))
    found = index >= 0
    row = torch.div(index.clamp(min=0), W, rounding_mode="floor")
    if "source" in want:
        out["source"] = torch.where(found, index.clamp(min=0) - row * W, index).to(torch.int32)
    if "source_row" in want:
        out["source_row"] = torch.where(found, row, index).to(torch.int32)
    if "kind" in want:
        kind = torch.where(src, 0, torch.where(filled1, 1, torch.where(filled2, 2, 3)))
        out["kind"] = kind.to(torch.uint8)
    if "disparity" in want:
        picked = flat.gather(1, index.clamp(min=0).reshape(B, -1)).view(B, H, W)
        out["disparity"] = torch.where(found, picked, torch.full_like(d, fill_value))
    return out


def _refine_torch(d, dr, keep, label, lo, hi, threshold, max_gap, prefer, fallback, fill_value, want):
    B, H, W = d.shape
    x = torch.arange(W, device=d.device).view(1, 1, W).expand(B, H, W)
    src, out = _sources(d, dr, keep, lo, hi, threshold)
    if not {"disparity", "kind", "source"} & set(want):
        return out
    has1, s1 = torch.zeros_like(src), torch.full_like(x, -1)
    if label is not None:
        cls = _classes(label)
        L, R = torch.full_like(x, -1), torch.full_like(x, W)
        for c in range(NUM_CLASSES):                    # per class a cummax / cummin; a pixel takes those of its own class
            mine = cls == c
            l, r = _nearest(src & mine, x, W)
            L, R = torch.where(mine, l, L), torch.where(mine, r, R)
        has1, s1 = _choose(d, x, L, R, W, max_gap, prefer)
    filled1 = ~src & has1
    if fallback:
        has2, s2 = _choose(d, x, *_nearest(src, x, W), W, max_gap, prefer)
        filled2 = ~src & ~has1 & has2
    else:
        filled2, s2 = torch.zeros_like(src), s1
    minus = torch.full_like(x, -1)
    source = torch.where(src, x, torch.where(filled1, s1, torch.where(filled2, s2, minus)))
    if "source" in want:
        out["source"] = source.to(torch.int32)
    if "kind" in want:
        kind = torch.where(src, 0, torch.where(filled1, 1, torch.where(filled2, 2, 3)))
        out["kind"] = kind.to(torch.uint8)
    if "disparity" in want:
        out["disparity"] = torch.where(source >= 0, d.gather(2, source.clamp(min=0)), torch.full_like(d, fill_value))
    return out


def _gap(value, most, what):
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or int(value) != value or value < 1:
        raise ValueError(f"{what} is an integer >= 1, got {value!r}")
    return min(int(value), max(most, 1))


def _refine(disparity, disp_right, label, keep, threshold, maxdisp, disp_range, max_gap, prefer, fallback, fill_value, want, keys,
            axes="rows"):
    if axes not in AXES:
        raise ValueError(f"axes is one of {AXES}, got {axes!r}")
    both = axes == "both"
    if both:
        keys = keys + ("source_row",)
    elif isinstance(max_gap, (tuple, list)):
        raise ValueError(f'max_gap is a pair (columns, rows) only with axes="both", got {max_gap!r}')
    want = tuple(want)
    if not want or not set(want) <= set(keys):
        raise ValueError(f"want names some of {keys}, got {want}")
    if prefer not in PREFER:
        raise ValueError(f"prefer is one of {tuple(PREFER)}, got {prefer!r}")
    if (maxdisp is None) == (disp_range is None):
        raise ValueError("give exactly one of maxdisp (the signed range) and disp_range=(lo, hi)")
    lo, hi = (-maxdisp, maxdisp) if disp_range is None else disp_range
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    if not lo < hi:
        raise ValueError(f"the disparity range is lo < hi, got ({lo}, {hi})")
    threshold = float(np.float32(threshold))
    if disp_right is not None and not threshold >= 0:
        raise ValueError(f"the threshold is not negative, got {threshold}")
    if not isinstance(disparity, torch.Tensor) or disparity.dim() not in (2, 3):
        raise ValueError("maps are [B,H,W] or [H,W]")
    maps = {"disp_right": disp_right, "label": label, "keep": keep}
    for name, t in maps.items():
        if t is not None and (not isinstance(t, torch.Tensor) or t.shape != disparity.shape):
            raise ValueError(f"{name} has the disparity's shape {tuple(disparity.shape)}, got {None if not isinstance(t, torch.Tensor) else tuple(t.shape)}")
    squeeze = disparity.dim() == 2
    if squeeze:
        disparity = disparity.unsqueeze(0)
        disp_right, label, keep = (None if t is None else t.unsqueeze(0) for t in (disp_right, label, keep))
    B, H, W = disparity.shape
    if both:
        pair = (W, H) if max_gap is None else tuple(max_gap) if isinstance(max_gap, (tuple, list)) else (max_gap, max_gap)
        if len(pair) != 2:
            raise ValueError(f"max_gap is an integer or a pair (columns, rows), got {max_gap!r}")
        gap_x, gap_y = _gap(pair[0], W, "max_gap (columns)"), _gap(pair[1], H, "max_gap (rows)")
    else:
        if max_gap is None:
            max_gap = W
        if isinstance(max_gap, bool) or int(max_gap) != max_gap or max_gap < 1:
            raise ValueError(f"max_gap is an integer >= 1, got {max_gap!r}")
        max_gap = min(int(max_gap), max(W, 1))
    fill_value = float(np.float32(fill_value))
    if keep is not None and keep.dtype == torch.bool:
        keep = keep.view(torch.uint8) if keep.is_contiguous() else keep.to(torch.uint8)
    how = None if label is None else D._label_for_kernel(label, disparity)
    floats = [disparity] + ([disp_right] if disp_right is not None else [])
    dense = floats + ([keep] if keep is not None else [])
    if both:
        if (all(t.dtype == torch.float32 for t in floats) and (keep is None or keep.dtype == torch.uint8) and _hip(*dense)
                and W <= MAX_WIDTH and H <= MAX_WIDTH and 0 < disparity.numel() < _MAX_ELEMENTS and (label is None or how is not None)):
            count("fill2d_hip")
            dev = disparity.device
            code, row, img = how if how is not None else (0, W, H * W)
            nbytes = query_bytes("ss_disparity_fill2d_scratch", B, H, W)
            with torch.cuda.device(dev):
                scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
                out = {k: torch.empty((B, H, W), dtype=_DTYPES[k], device=dev) for k in want}
                call("ss_disparity_fill2d_fwd", ptr(disparity), ptr(disp_right), ptr(keep), ptr(label), code, row, img, B, H, W, lo, hi,
                     threshold, gap_x, gap_y, PREFER[prefer], int(bool(fallback)), fill_value, ptr(scratch), nbytes,
                     *(ptr(out.get(k)) for k in ("disparity", "kind", "source", "source_row", "consistent")))
        elif disparity.numel() == 0:
            count("fill2d_torch")
            out = {k: torch.empty((B, H, W), dtype=_DTYPES[k], device=disparity.device) for k in want}
        else:
            count("fill2d_torch")
            out = _fill2d_torch(disparity.to(torch.float32).contiguous(), None if disp_right is None else disp_right.to(torch.float32),
                                keep, label, lo, hi, threshold, gap_x, gap_y, PREFER[prefer], bool(fallback), fill_value, want)
    elif (all(t.dtype == torch.float32 for t in floats) and (keep is None or keep.dtype == torch.uint8) and _hip(*dense)
            and W <= MAX_WIDTH and 0 < disparity.numel() < _MAX_ELEMENTS and (label is None or how is not None)):
        count("refine_hip")
        dev = disparity.device
        out = {k: torch.empty((B, H, W), dtype=_DTYPES[k], device=dev) for k in want}
        code, row, img = how if how is not None else (0, W, H * W)
        with torch.cuda.device(dev):
            call("ss_disparity_refine_fwd", ptr(disparity), ptr(disp_right), ptr(keep), ptr(label), code, row, img, B, H, W, lo, hi,
                 threshold, max_gap, PREFER[prefer], int(bool(fallback)), fill_value, *(ptr(out.get(k)) for k in REFINE_KEYS))
    else:
        count("refine_torch")
        out = _refine_torch(disparity.to(torch.float32), None if disp_right is None else disp_right.to(torch.float32), keep, label,
                            lo, hi, threshold, max_gap, PREFER[prefer], bool(fallback), fill_value, want)
    out = {k: out[k] for k in want}
    return {k: v[0] for k, v in out.items()} if squeeze else out


@_nograd
def fill_disparity(disparity, label=None, keep=None, maxdisp=None, disp_range=None, max_gap=None, prefer="background", fallback=True,
                   fill_value=-999.0, want=("disparity", "kind"), axes="rows"):
    """The holes of a disparity map filled row by row from the surface they belong to (the module's definitions).  `disparity`
    [B,H,W] (or [H,W]) float32 -- anything else is converted first; `label` of any dtype: the class of every pixel, without it every
    pixel is of no class and only tier 2 fills; `keep`: a bool / uint8 mask of the pixels that may serve as sources (the `consistent`
    map of data.lr_consistency, a confidence threshold).  Exactly one of `maxdisp` (-maxdisp <= d < maxdisp) and `disp_range=(lo, hi)`
    names the values that are sources at all; `max_gap` (default: the row's width) bounds how far a value may travel; `prefer` is
    "background" or "nearest"; `fallback=False` leaves what the own class cannot fill.  `want` names some of ("disparity", "kind",
    "source").  Returns a dictionary of tensors on the input's device; nothing waits on the host.  An argument that makes no sense
    is a ValueError before any launch.

    `axes="both"` looks along the columns too (the module's paragraph on the two-axis fill): the candidates are the nearest sources
    to the left, to the right, above and below; `max_gap` may then be a pair (columns, rows) (default: the map's width and height)
    and `want` may name "source_row"."""
    return _refine(disparity, None, label, keep, 0.0, maxdisp, disp_range, max_gap, prefer, fallback, fill_value, want, REFINE_KEYS[:3],
                   axes)


@_nograd
def refine_disparity(disp_left, disp_right, label=None, threshold=1.0, keep=None, maxdisp=None, disp_range=None, max_gap=None,
                     prefer="background", fallback=True, fill_value=-999.0, want=("disparity", "kind"), axes="rows"):
    """The left-right check and the fill in one pass: a pixel of `disp_left` is a source only if it is also consistent with
    `disp_right` (data.lr_consistency's definition and arguments: `disp_right[r]` is the disparity of RIGHT pixel r,
    `-model(right, left)` for a model; `threshold` in pixels), everything else is filled as fill_disparity does.  `want` may also name
    "consistent", the bool map of the check.  `axes="both"`: as for fill_disparity."""
    if disp_right is None:
        raise ValueError("refine_disparity takes two estimates; fill_disparity takes one")
    return _refine(disp_left, disp_right, label, keep, threshold, maxdisp, disp_range, max_gap, prefer, fallback, fill_value, want,
                   REFINE_KEYS, axes)


def _keys(d):
    """The monotone integer key of every fp32 bit pattern (int32; the map is its own inverse)."""
    b = d.view(torch.int32)
    return b ^ ((b >> 31) & 0x7FFFFFFF)


def _median_torch(d, cls, where, lo, hi, r, same_class, fill_holes, min_count, want_count):
    """One pass of the definitions: (disparity, count or None).  d float32 [B,H,W], cls int64 [B,H,W] (NUM_CLASSES: none), where uint8
    or None.  The (2r + 1)^2 shifted views of the NaN / none-padded maps, a sort of the members' keys along the stack (a slot that is
    no member sorts last) and a gather at (n - 1) // 2."""
    B, H, W = d.shape
    pad = (r, r, r, r)
    dp = torch.nn.functional.pad(d, pad, value=float("nan"))
    cp = torch.nn.functional.pad(cls, pad, value=NUM_CLASSES)
    vp = (dp >= lo) & (dp < hi)
    kp = _keys(dp).long()
    own = (cls != NUM_CLASSES) if same_class else None
    last = torch.full((), torch.iinfo(torch.int64).max, dtype=torch.int64, device=d.device)
    slots, n = [], torch.zeros((B, H, W), dtype=torch.int64, device=d.device)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            member = vp[:, dy:dy + H, dx:dx + W]
            if same_class:
                member = member & (~own | (cp[:, dy:dy + H, dx:dx + W] == cls))
            slots.append(torch.where(member, kp[:, dy:dy + H, dx:dx + W], last))
            n = n + member
    ordered = torch.stack(slots).sort(dim=0).values
    pick = ordered.gather(0, ((n - 1) // 2).clamp(min=0).unsqueeze(0))[0].to(torch.int32)
    target = n >= min_count
    if not fill_holes:
        target = target & vp[:, r:r + H, r:r + W]
    if where is not None:
        target = target & (where != 0)
    out = torch.where(target, pick ^ ((pick >> 31) & 0x7FFFFFFF), d.view(torch.int32)).view(torch.float32)
    count = torch.where(target, n, torch.zeros_like(n)).to(torch.uint8) if want_count else None
    return out, count


@_nograd
def median_disparity(disparity, label=None, where=None, maxdisp=None, disp_range=None, radius=2, same_class=True, fill_holes=False,
                     min_count=1, iterations=1, want=("disparity",)):
    """The class-aware 2-D median of a disparity map (the module's definitions), the step after fill_disparity / refine_disparity: it
    removes the streaks and outliers a row-wise fill leaves without blurring the steps between surfaces.  `disparity` [B,H,W] (or
    [H,W]) float32 -- anything else is converted first; `label` of any dtype: the class of every pixel, without it (or with
    `same_class=False`) the median is class-agnostic; `where`: a bool / uint8 mask of the pixels that may change (`kind != 0` of a
    fill keeps the model's own values bit for bit).  Exactly one of `maxdisp` (-maxdisp <= d < maxdisp) and `disp_range=(lo, hi)`
    names the valid values; `radius` 1 .. 4 (the kernel takes 1 and 2); `fill_holes` lets a pixel that is not valid take the median
    of its window; `min_count` members at least, 1 .. (2 radius + 1)^2; `iterations` passes between two buffers -- the caller's
    tensor is never written.  `want` names some of ("disparity", "count"); "count" uint8 is the number of members of the last pass
    on a replaced pixel, 0 elsewhere.  Returns a dictionary of tensors on the input's device; nothing waits on the host.  An
    argument that makes no sense is a ValueError before any launch."""
    want = tuple(want)
    if not want or not set(want) <= set(MEDIAN_KEYS):
        raise ValueError(f"want names some of {MEDIAN_KEYS}, got {want}")
    if (maxdisp is None) == (disp_range is None):
        raise ValueError("give exactly one of maxdisp (the signed range) and disp_range=(lo, hi)")
    lo, hi = (-maxdisp, maxdisp) if disp_range is None else disp_range
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    if not lo < hi:
        raise ValueError(f"the disparity range is lo < hi, got ({lo}, {hi})")
    for name, v, least, most in (("radius", radius, 1, MEDIAN_MAX_RADIUS), ("iterations", iterations, 1, None)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < least or (most is not None and v > most):
            raise ValueError(f"{name} is an integer {least} .. {'' if most is None else most}, got {v!r}")
    radius, iterations = int(radius), int(iterations)
    window = (2 * radius + 1) ** 2
    if isinstance(min_count, bool) or not isinstance(min_count, (int, np.integer)) or not 1 <= min_count <= window:
        raise ValueError(f"min_count is an integer 1 .. {window} at radius {radius}, got {min_count!r}")
    if not isinstance(disparity, torch.Tensor) or disparity.dim() not in (2, 3):
        raise ValueError("maps are [B,H,W] or [H,W]")
    for name, t in (("label", label), ("where", where)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.shape != disparity.shape):
            raise ValueError(f"{name} has the disparity's shape {tuple(disparity.shape)}, got {None if not isinstance(t, torch.Tensor) else tuple(t.shape)}")
    same_class, fill_holes, min_count = bool(same_class), bool(fill_holes), int(min_count)
    squeeze = disparity.dim() == 2
    if squeeze:
        disparity = disparity.unsqueeze(0)
        label, where = (None if t is None else t.unsqueeze(0) for t in (label, where))
    B, H, W = disparity.shape
    if where is not None and where.dtype == torch.bool:
        where = where.view(torch.uint8) if where.is_contiguous() else where.to(torch.uint8)
    how = None if label is None else D._label_for_kernel(label, disparity)
    dense = [disparity] + ([where] if where is not None else [])
    if (disparity.dtype == torch.float32 and (where is None or where.dtype == torch.uint8) and _hip(*dense)
            and radius <= _MEDIAN_KERNEL_RADIUS and 0 < disparity.numel() < _MAX_ELEMENTS and (label is None or how is not None)):
        count("median_hip")
        dev = disparity.device
        code, row, img = how if how is not None else (0, W, H * W)
        src, counts = disparity, None
        with torch.cuda.device(dev):
            bufs = [torch.empty((B, H, W), dtype=torch.float32, device=dev) for _ in range(min(iterations, 2))]
            for i in range(iterations):
                dst = bufs[i % 2]
                if "count" in want and i == iterations - 1:
                    counts = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
                call("ss_disparity_median_fwd", ptr(src), ptr(label), code, row, img, ptr(where), B, H, W, lo, hi, radius,
                     int(same_class), int(fill_holes), min_count, ptr(dst), ptr(counts))
                src = dst
        out = {"disparity": src, "count": counts}
    else:
        count("median_torch")
        src, counts = disparity.to(torch.float32), None
        cls = torch.full((B, H, W), NUM_CLASSES, dtype=torch.int64, device=disparity.device) if label is None else _classes(label)
        for i in range(iterations):
            src, counts = _median_torch(src.contiguous(), cls, where, lo, hi, radius, same_class, fill_holes, min_count,
                                        "count" in want and i == iterations - 1)
        out = {"disparity": src, "count": counts}
    out = {k: out[k] for k in want}
    return {k: v[0] for k, v in out.items()} if squeeze else out


def _speckle_torch(d, cls, where, lo, hi, max_diff, max_size, same_class, fill_value, want):
    """The definitions by label propagation: d float32 [B,H,W], cls int64 [B,H,W] (NUM_CLASSES: none), where uint8 or None.  Every
    valid pixel starts with its own index; a round takes the minimum over the linked 4-neighbours and then follows the labels as
    pointers (label[p] = label[label[p]], three times); the rounds end when one changes nothing, which the host is asked once per
    round.  At that point a label is constant over a component, never above any of its pixels' indices and always one of them: the
    smallest."""
    B, H, W = d.shape
    HW = H * W
    dev = d.device
    valid = (d >= lo) & (d < hi)

    def link(a, b):
        m = valid[a] & valid[b] & ((d[a] - d[b]).abs() <= max_diff)
        return m & (cls[a] == cls[b]) if same_class else m
    every = slice(None)
    right = link((every, every, slice(0, W - 1)), (every, every, slice(1, W)))            # p links p + 1
    down = link((every, slice(0, H - 1), every), (every, slice(1, H), every))             # p links p + W
    no_col, no_row = torch.zeros((B, H, 1), dtype=torch.bool, device=dev), torch.zeros((B, 1, W), dtype=torch.bool, device=dev)
    to_r, to_l = torch.cat([right, no_col], 2), torch.cat([no_col, right], 2)
    to_d, to_u = torch.cat([down, no_row], 1), torch.cat([no_row, down], 1)
    none = torch.full((), HW, dtype=torch.int64, device=dev)                               # the label of a pixel that is not valid
    col, row = none.expand(B, H, 1), none.expand(B, 1, W)
    lab = torch.where(valid, torch.arange(HW, device=dev).view(1, H, W).expand(B, H, W), none)
    while True:
        new = torch.minimum(lab, torch.where(to_r, torch.cat([lab[:, :, 1:], col], 2), none))
        new = torch.minimum(new, torch.where(to_l, torch.cat([col, lab[:, :, :-1]], 2), none))
        new = torch.minimum(new, torch.where(to_d, torch.cat([lab[:, 1:], row], 1), none))
        new = torch.minimum(new, torch.where(to_u, torch.cat([row, lab[:, :-1]], 1), none)).reshape(B, HW)
        for _ in range(3):
            new = torch.cat([new, none.expand(B, 1)], 1).gather(1, new)                   # (slot HW: none points at none)
        new = new.view(B, H, W)
        if bool(torch.equal(new, lab)):                                                    # the host waits here, once per round
            break
        lab = new
    flat = lab.reshape(B, HW)
    out = {}
    if {"disparity", "speckle", "size"} & set(want):
        ones = valid.reshape(B, HW).to(torch.int64)
        size = torch.zeros((B, HW + 1), dtype=torch.int64, device=dev).scatter_add_(1, flat, ones).gather(1, flat).view(B, H, W)
        size = torch.where(valid, size, torch.zeros_like(size))
        speckle = valid & (size <= max_size)
        if where is not None:
            speckle = speckle & (where != 0)
        out["size"], out["speckle"] = size.to(torch.int32), speckle
        if "disparity" in want:
            out["disparity"] = torch.where(speckle, torch.full_like(d, fill_value), d)
    if "component" in want:
        out["component"] = torch.where(valid, lab, torch.full_like(lab, -1)).to(torch.int32)
    return out


@_nograd
def filter_speckles(disparity, label=None, where=None, maxdisp=None, disp_range=None, max_size=100, max_diff=1.0, same_class=True,
                    fill_value=-999.0, want=("disparity", "speckle")):
    """Small connected blobs of a disparity map removed (the module's definitions), the step before fill_disparity /
    refine_disparity: a blob that passed the left-right check would be a source of the fill and be smeared along its rows; marked as
    a speckle (`keep=~speckle`) it is filled from its surroundings instead.  `disparity` [B,H,W] (or [H,W]) float32 -- anything else
    is converted first; `label` of any dtype: the class of every pixel -- a roof blob is not linked to the ground it touches; without
    it (or with `same_class=False`) only the disparities decide; `where`: a bool / uint8 mask of the pixels that may be removed.
    Exactly one of `maxdisp` (-maxdisp <= d < maxdisp) and `disp_range=(lo, hi)` names the valid values; `max_diff` >= 0: the
    largest step between two linked neighbours; `max_size` >= 0: the largest component that is removed (0: none is).  `want` names
    some of ("disparity", "speckle", "size", "component"); an output that is not named is not allocated, and the caller's tensor is
    never written.  Returns a dictionary of tensors on the input's device.  On the kernel nothing waits on the host; the PyTorch
    composition (CPU tensors, other dtypes, a label whose rows are not contiguous, SS_REFINE_HIP=0) asks the host once per round of
    its label propagation whether anything changed.  An argument that makes no sense is a ValueError before any launch."""
    want = tuple(want)
    if not want or not set(want) <= set(SPECKLE_KEYS):
        raise ValueError(f"want names some of {SPECKLE_KEYS}, got {want}")
    if (maxdisp is None) == (disp_range is None):
        raise ValueError("give exactly one of maxdisp (the signed range) and disp_range=(lo, hi)")
    lo, hi = (-maxdisp, maxdisp) if disp_range is None else disp_range
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    if not lo < hi:
        raise ValueError(f"the disparity range is lo < hi, got ({lo}, {hi})")
    if isinstance(max_size, bool) or not isinstance(max_size, (int, np.integer)) or not 0 <= max_size < _MAX_ELEMENTS:
        raise ValueError(f"max_size is an integer 0 .. 2^31 - 1, got {max_size!r}")
    if isinstance(max_diff, bool) or not isinstance(max_diff, (int, float, np.integer, np.floating)) or not max_diff >= 0:
        raise ValueError(f"max_diff is a number >= 0, got {max_diff!r}")
    max_size, max_diff, same_class = int(max_size), float(np.float32(max_diff)), bool(same_class)
    if not isinstance(disparity, torch.Tensor) or disparity.dim() not in (2, 3):
        raise ValueError("maps are [B,H,W] or [H,W]")
    for name, t in (("label", label), ("where", where)):
        if t is not None and (not isinstance(t, torch.Tensor) or t.shape != disparity.shape):
            raise ValueError(f"{name} has the disparity's shape {tuple(disparity.shape)}, got {None if not isinstance(t, torch.Tensor) else tuple(t.shape)}")
    fill_value = float(np.float32(fill_value))
    squeeze = disparity.dim() == 2
    if squeeze:
        disparity = disparity.unsqueeze(0)
        label, where = (None if t is None else t.unsqueeze(0) for t in (label, where))
    B, H, W = disparity.shape
    if where is not None and where.dtype == torch.bool:
        where = where.view(torch.uint8) if where.is_contiguous() else where.to(torch.uint8)
    how = None if label is None else D._label_for_kernel(label, disparity)
    dense = [disparity] + ([where] if where is not None else [])
    if (disparity.dtype == torch.float32 and (where is None or where.dtype == torch.uint8) and _hip(*dense)
            and 0 < disparity.numel() < _MAX_ELEMENTS and (label is None or how is not None)):
        count("speckle_hip")
        dev = disparity.device
        code, row, img = how if how is not None else (0, W, H * W)
        nbytes = query_bytes("ss_disparity_speckle_scratch", B, H, W)
        with torch.cuda.device(dev):
            scratch = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            out = {k: torch.empty((B, H, W), dtype=_SPECKLE_DTYPES[k], device=dev) for k in want}
            call("ss_disparity_speckle_fwd", ptr(disparity), ptr(label), code, row, img, ptr(where), B, H, W, lo, hi, max_diff, max_size,
                 int(same_class), fill_value, ptr(scratch), nbytes, *(ptr(out.get(k)) for k in SPECKLE_KEYS))
    elif disparity.numel() == 0:
        count("speckle_torch")
        out = {k: torch.empty((B, H, W), dtype=_SPECKLE_DTYPES[k], device=disparity.device) for k in want}
    else:
        count("speckle_torch")
        cls = torch.full((B, H, W), NUM_CLASSES, dtype=torch.int64, device=disparity.device) if label is None else _classes(label)
        out = _speckle_torch(disparity.to(torch.float32), cls, where, lo, hi, max_diff, max_size, same_class, fill_value, want)
    out = {k: out[k] for k in want}
    return {k: v[0] for k, v in out.items()} if squeeze else out
