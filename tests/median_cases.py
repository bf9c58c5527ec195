"""What the median tests share (test infrastructure, like refine_cases.py): the case table, the planted values and a SEQUENTIAL
restatement of the definitions of include/semstereo_hip.h (section "disparity refinement: class-aware median"), written for these
tests from those definitions and not from the composition: per pixel a loop over its window that collects the members' integer keys,
Python's sort, the element at (n - 1) // 2.  Validity is a comparison of numpy float32 scalars; nothing else touches a value."""
import itertools

import numpy as np
import torch

import refine_cases as fc
from semstereo_amd.refine import MEDIAN_TILE

FILL = -999.0
NONE = 8                                         # the class of a pixel without one
MAXDISP = 8
LO, HI = float(-MAXDISP), float(MAXDISP)
TH, TW = MEDIAN_TILE                             # csrc/disparity_median.hip: the output pixels of a workgroup
RADII = (1, 2)                                   # what the kernel takes

#: name -> (B, H, W): the smallest shapes at which the tiling can go wrong
CASES = {
    "one_pixel": (1, 1, 1),                      # the whole halo is off the image
    "thin": (1, 2, 7),                           # H < r + 1: rows missing on both sides; W % 4 == 3
    "one_tile": (1, TH, TW),                     # exactly one tile, every halo pixel off the image
    "tile_plus_one": (1, TH + 1, TW + 1),        # a second tile row / column of one row / column, whose halo is the first tile
    "batch_minus_one": (2, TH - 1, TW - 1),      # ragged quads; the halo of image 0's last rows must not be image 1's first rows
    "grid": (2, 2 * TH + 3, 2 * TW + 3),         # 3 x 3 tiles per image, interior halos on all four sides
    "wide": (1, 3, 16 * TW + 6),                 # many tile columns, W % 4 == 2
}
PLANT_H, PLANT_W = 15, 27                        # the room the planted regions need


def has_plants(name):
    return CASES[name][1] >= PLANT_H and CASES[name][2] >= PLANT_W


#: the planted regions of image 0 (H >= 15, W >= 27); each is the 5 x 5 window of its centre at radius 2, `where` true all over it
#:   rows 1-5, cols 1-5     centre (3, 3): an even count at both radii with -0.0 and +0.0 around the median position.  The inner 3 x 3
#:                          holds -1 -1 -1 / hole 1 -0.0 / +0.0 1 1 (n = 8: -0.0 at index 3), the ring 8 times -1 and 8 times 1
#:                          (n = 24: -0.0 at index 11); class 1 everywhere
#:   rows 1-5, cols 8-12    centre (3, 10): NaN +inf -inf / lo 2 hi / 3 3 5, the ring all holes: the members are lo, 2, 3, 3, 5 at both
#:                          radii, the pick 3; the NaN at (2, 9) and hi at (3, 11) pass through unless fill_holes is set
#:   rows 1-5, cols 15-19   centre (3, 17): 6.0 of class 3 among 1.0 of class 2: the only member of its class, n = 1, itself
#:   rows 1-5, cols 22-26   centre (3, 24): a hole of class 4 among 1.5 of class 2: n = 0, untouched even with fill_holes; without a
#:                          label (or class-agnostic) it is filled with 1.5
#:   row 8                  no valid pixel, rows 7 and 9 valid all along: with fill_holes every pixel of it is filled
#:   rows 10-14, cols 1-5   centre (12, 3): 2.0 of class 5, one more member of class 5 at (12, 4) (4.0), class 0 around: n = 2, one
#:                          below min_count = 3
def _plant(d, y, where):
    nan, inf = float("nan"), float("inf")
    where[0, 1:6, 1:27] = True
    where[0, 8] = True
    where[0, 10:15, 1:6] = True
    y[0, 1:6, 1:6] = 1
    ring = torch.tensor([-1.0, 1.0] * 8)
    block = torch.zeros(5, 5)
    edge = torch.ones(5, 5, dtype=torch.bool)
    edge[1:4, 1:4] = False
    block[edge] = ring
    block[1:4, 1:4] = torch.tensor([[-1.0, -1.0, -1.0], [FILL, 1.0, -0.0], [0.0, 1.0, 1.0]])
    d[0, 1:6, 1:6] = block
    y[0, 1:6, 8:13] = 2
    d[0, 1:6, 8:13] = FILL
    d[0, 2:5, 9:12] = torch.tensor([[nan, inf, -inf], [LO, 2.0, HI], [3.0, 3.0, 5.0]])
    y[0, 1:6, 15:20], d[0, 1:6, 15:20] = 2, 1.0
    y[0, 3, 17], d[0, 3, 17] = 3, 6.0
    y[0, 1:6, 22:27], d[0, 1:6, 22:27] = 2, 1.5
    y[0, 3, 24], d[0, 3, 24] = 4, FILL
    for row in (7, 9):
        bad = ~((d[0, row] >= LO) & (d[0, row] < HI))
        d[0, row][bad] = 0.5
    d[0, 8] = FILL
    y[0, 10:15, 1:6], d[0, 10:15, 1:6] = 0, 1.0
    y[0, 12, 3:5] = 5
    d[0, 12, 3], d[0, 12, 4] = 2.0, 4.0


def make_case(name):
    """(disparity float32, label int64, label float32, where bool) [B,H,W] of a case.  Everywhere: a field on the half-pixel grid that
    leaves the range in places, no-data columns x % 11 == 10 and runs of holes, labels in blocks of 3 x 5 pixels with 7, 8, 200, -1
    sprinkled in (the float map: 2.5 and NaN too), `where` false on about a third of the pixels.  Planted where the shape has room:
    see _plant; the small shapes get the special values in row 0."""
    B, H, W = CASES[name]
    g = torch.Generator().manual_seed(9800 + 131 * H + W)
    d = torch.round((2 * torch.rand(B, H, W, generator=g) - 1) * 1.2 * MAXDISP * 2) / 2
    d[:, :, 10::11] = FILL
    runs = torch.rand(B, H, -(-W // 7), generator=g).repeat_interleave(7, dim=2)[:, :, :W] < 0.3
    d[runs] = FILL
    y = torch.randint(0, 6, (B, -(-H // 3), -(-W // 5)), generator=g).repeat_interleave(3, dim=1).repeat_interleave(5, dim=2)[:, :H, :W].contiguous()
    odd = torch.tensor([7, 8, 200, -1])
    y[:, :, 3::13] = odd[torch.arange(len(range(3, W, 13))) % 4]
    where = torch.rand(B, H, W, generator=g) >= 1 / 3
    if has_plants(name):
        _plant(d, y, where)
    elif W >= 7:
        d[0, 0, :7] = torch.tensor([float("nan"), float("inf"), float("-inf"), LO, HI, -0.0, 0.0])
    yf = y.to(torch.float32)
    yf[:, 1::2, 5::17] = 2.5
    yf[:, 0::2, 6::19] = float("nan")
    if has_plants(name):
        yf[0, 1:6, 1:27] = y[0, 1:6, 1:27].float()
        yf[0, 10:15, 1:6] = y[0, 10:15, 1:6].float()
    return d.contiguous(), y, yf, where


def class_of(v):
    """The class of a label value (a numpy scalar of any dtype): int(v) for an integer-valued 0 <= v < 8, else NONE."""
    if not (0 <= v < 8):                                     # (False for a NaN)
        return NONE
    return int(v) if v == np.trunc(v) else NONE


def key_of(b):
    """The order's integer key of a bit pattern b, a signed 32-bit integer as a Python int; its own inverse."""
    return b ^ ((b >> 31) & 0x7FFFFFFF)


def _picks(d, label, r, same_class, lo, hi, _stage={}):
    """Per pixel (n, the pick's bit pattern or None for n = 0) as nested lists [B][H][W]: what does not depend on `where`, fill_holes
    and min_count.  Computed once per (map, label, radius, same_class) -- the inputs of a case are shared and never change."""
    same_class = bool(same_class and label is not None)
    ident = (id(d), None if label is None else id(label), r, same_class, lo, hi)
    if ident not in _stage:
        a = d.numpy()
        B, H, W = a.shape
        lo32, hi32 = np.float32(lo), np.float32(hi)
        bits = a.view(np.int32).tolist()
        valid = [[[bool(lo32 <= a[b, h, x] < hi32) for x in range(W)] for h in range(H)] for b in range(B)]
        cls = None
        if same_class:
            yy = label.numpy()
            cls = [[[class_of(yy[b, h, x]) for x in range(W)] for h in range(H)] for b in range(B)]
        out = []
        for b in range(B):
            image = []
            for h in range(H):
                row = []
                for x in range(W):
                    mine = cls[b][h][x] if same_class else NONE
                    keys = []
                    for hh in range(max(h - r, 0), min(h + r, H - 1) + 1):
                        for xx in range(max(x - r, 0), min(x + r, W - 1) + 1):
                            if valid[b][hh][xx] and (mine == NONE or cls[b][hh][xx] == mine):
                                keys.append(key_of(bits[b][hh][xx]))
                    keys.sort()
                    n = len(keys)
                    row.append((n, key_of(keys[(n - 1) // 2]) if n else None))
                image.append(row)
            out.append(image)
        _stage[ident] = (out, valid, (d, label))                 # (the tensors are held: their ids stay theirs)
    return _stage[ident][:2]


def restate(d, label=None, where=None, lo=LO, hi=HI, radius=2, same_class=True, fill_holes=False, min_count=1, iterations=1):
    """{"disparity", "count"} as torch tensors, from the sequential loops."""
    for _ in range(iterations):
        picks, valid = _picks(d, label, radius, same_class, lo, hi)
        B, H, W = d.shape
        out = d.numpy().view(np.int32).copy()
        count = np.zeros((B, H, W), dtype=np.uint8)
        w = None if where is None else where.numpy()
        for b in range(B):
            for h in range(H):
                for x in range(W):
                    n, pick = picks[b][h][x]
                    if (w is None or w[b, h, x] != 0) and (valid[b][h][x] or fill_holes) and n >= max(1, min_count):
                        out[b, h, x], count[b, h, x] = pick, n
        d = torch.from_numpy(out.view(np.float32))
    return {"disparity": d, "count": torch.from_numpy(count)}


_MEMO = {}


def case(name):
    """{"d", "y", "yf", "where"} of a case, computed once and shared: leave it unchanged."""
    if name not in _MEMO:
        d, y, yf, where = make_case(name)
        _MEMO[name] = dict(d=d, y=y, yf=yf, where=where)
    return _MEMO[name]


#: (label: None / "y" / "yf", with where, (same_class, fill_holes, min_count))
FLAGS = ((1, 0, 1), (1, 1, 3), (0, 1, 1))
VARIANTS = tuple(itertools.product((None, "y", "yf"), (False, True), FLAGS))
#: what the device tests run of them
GPU_VARIANTS = (("y", True, (1, 1, 3)), ("yf", False, (1, 0, 1)), (None, True, (0, 1, 1)), ("y", False, (0, 1, 1)))
#: the variant that also runs two iterations, on the case TWICE
TWICE = ("tile_plus_one", ("y", False, (1, 1, 3)))


def arguments(c, variant, radius, iterations=1):
    which, with_where, (same_class, fill_holes, min_count) = variant
    return dict(label=None if which is None else c[which], where=c["where"] if with_where else None, radius=radius,
                same_class=bool(same_class), fill_holes=bool(fill_holes), min_count=min_count, iterations=iterations)


def call(sa, c, variant, radius, want=("disparity", "count"), move=lambda t: t, iterations=1):
    kw = {k: move(v) if isinstance(v, torch.Tensor) else v for k, v in arguments(c, variant, radius, iterations).items()}
    return sa.median_disparity(move(c["d"]), disp_range=(LO, HI), want=want, **kw)


def expected(c, variant, radius, iterations=1):
    return restate(c["d"], **arguments(c, variant, radius, iterations))


def closed_forms():
    """(what, disparity [1,3,3], label or None, keyword arguments, disparity, count) as literals, maxdisp = 4, radius = 1."""
    t = lambda v, dtype=torch.float32: torch.tensor(v, dtype=dtype).view(1, 3, 3)        # noqa: E731
    spike = [[1.0, 1.0, 1.0], [1.0, 3.0, 1.0], [1.0, 1.0, 1.0]]
    alone = [[0, 0, 0], [0, 1, 0], [0, 0, 0]]
    line = [[2.0, 0.0, 2.0]] * 3
    line_y = [[1, 0, 1]] * 3
    border = [[4, 6, 4], [6, 9, 6], [4, 6, 4]]                       # the sizes of the windows of a 3 x 3 image
    forms = [
        # a spike in the middle is removed; a border window holds it once among 3 or 5 ones
        ("spike", t(spike), None, {}, [[1.0] * 3] * 3, border),
        # ... the same spike of a class of its own is the only member of its window: kept
        ("spike_of_another_class", t(spike), t(alone, torch.int64), {}, spike, [[3, 5, 3], [5, 1, 5], [3, 5, 3]]),
        # a line one pixel wide between another class: the class-aware median keeps both surfaces where they are ...
        ("line_kept", t(line), t(line_y, torch.int64), {}, line, [[2, 2, 2], [3, 3, 3], [2, 2, 2]]),
        # ... the class-agnostic one moves them: the line takes the majority, the sides' even windows the lower half
        ("line_moved", t(line), t(line_y, torch.int64), {"same_class": False}, [[0.0, 2.0, 0.0]] * 3, border),
        # a hole is filled only when asked
        ("hole_kept", t([[1.0, 1.0, 1.0], [1.0, FILL, 2.0], [2.0, 2.0, 2.0]]), None, {},
         [[1.0, 1.0, 1.0], [1.0, FILL, 2.0], [2.0, 2.0, 2.0]], [[3, 5, 3], [5, 0, 5], [3, 5, 3]]),
        ("hole_filled", t([[1.0, 1.0, 1.0], [1.0, FILL, 2.0], [2.0, 2.0, 2.0]]), None, {"fill_holes": True},
         [[1.0, 1.0, 1.0], [1.0, 1.0, 2.0], [2.0, 2.0, 2.0]], [[3, 5, 3], [5, 8, 5], [3, 5, 3]]),
    ]
    return [(what, d, y, kw, t(out), t(count, torch.uint8)) for what, d, y, kw, out, count in forms]


def full_batch():
    """(disparity float32 [2,1024,1024], label uint8) on the host: the first two images of refine_cases.full_batch."""
    d, label = fc.full_batch()
    return d[:2].contiguous(), label[:2].contiguous()


def same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        a, b = (got[k].view(torch.int32), want[k].view(torch.int32)) if k == "disparity" else (got[k], want[k])      # bits: -0.0 is not 0.0
        assert torch.equal(a, b), f"{what} {k}: {(a != b).sum().item()} of {b.numel()} values differ"


# ------------------------------------------------------------------------------------------------ SceneStereo(refine=dict(median=))
MEDIAN = dict(radius=2, iterations=2, fill_holes=True)


def check_scene(sa, stereo, left, right):
    """SceneStereo(refine=dict(..., median=MEDIAN)) against one median_disparity call on its own refined mosaic; returns the outputs."""
    got = stereo(left, right, want=("disparity_refined", "kind", "label", "disparity_median"))
    assert tuple(got) == ("disparity_refined", "kind", "label", "disparity_median")
    want = sa.median_disparity(got["disparity_refined"], label=got["label"], where=got["kind"] != 0, maxdisp=fc.REFINE["maxdisp"], **MEDIAN)
    bits = lambda t: t.view(torch.int32)                                                   # noqa: E731
    assert torch.equal(bits(got["disparity_median"]), bits(want["disparity"]))
    kept = got["kind"] == 0                                                                # where="filled": the model's values stay
    assert torch.equal(torch.where(kept, bits(got["disparity_median"]), 0), torch.where(kept, bits(got["disparity_refined"]), 0))
    assert not torch.equal(bits(got["disparity_median"]), bits(got["disparity_refined"]))  # ... and something else moved
    only = stereo(left, right, want=("disparity_median",))
    assert tuple(only) == ("disparity_median",) and torch.equal(bits(only["disparity_median"]), bits(got["disparity_median"]))
    return got
