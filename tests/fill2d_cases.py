"""What the tests of the two-axis fill share (test infrastructure, like refine_cases.py): the case table, the planted values and a
SEQUENTIAL restatement of the definitions of include/semstereo_hip.h, section "disparity refinement: fill along rows and columns",
written for these tests from those definitions.  refine_cases._candidates -- the raster loop that carries the last source per class
forward and backward along a line -- is applied to every row and to every column; then the two gaps, the tiers and Python's min()
over the tuples (v, g, order) / (g, v, order), v a numpy float32 scalar, pixel by pixel.  The left-right check is
right_view_cases.restate_lr, nothing of it is restated here."""
import numpy as np
import torch

import refine_cases as fc
import right_view_cases as rc

FILL = fc.FILL
NONE = fc.NONE
THRESHOLD = fc.THRESHOLD
same = fc.same
TILE = (64, 256)                                 # semstereo_amd.refine.FILL2D_TILE: rows x columns of a workgroup; a wave owns 16 rows

#: name -> (B, H, W, maxdisp).  The kernels work on tiles of 64 rows (segments) x 256 columns (strips), a wave owns 16 rows of a
#: segment, a thread 4 columns; the last launch is the row kernel's (chunks of columns, row-quad trips).  The shapes are the smallest
#: at which each of those can go wrong.
CASES = {
    "one_row": (1, 1, 37, 8),            # no vertical neighbour: equals axes="rows" on disparity, kind, source
    "one_col": (1, 37, 1, 8),            # only vertical neighbours
    "quads_7x7": (1, 7, 7, 4),           # the smallest two-axis case
    "batch_37x37": (2, 37, 37, 8),       # refine_cases' planted row 0, and the same plant down column 0
    "waves_33x5": (1, 33, 5, 8),         # rows 15 / 16 / 17 and 31 / 32: the wave boundaries inside a segment
    "segment_64x9": (1, 64, 9, 8),       # exactly one segment
    "segment_65x9": (1, 65, 9, 8),       # a second segment of one row
    "carry_197x260": (1, 197, 260, 16),  # 3 segments + 5 rows, a second strip of 4 columns; the planted columns (make_case)
    "strip_66x257": (1, 66, 257, 16),    # a second strip one column wide
    "rows_70x1030": (1, 70, 1030, 48),   # the row kernel's chunk 8 and second trip, with two segments
    "tall_8192x8": (1, 8192, 8, 8),      # the tallest map the kernel takes: 128 segments, 16-bit rows
    "tall_8193x4": (1, 8193, 4, 8),      # taller than the kernel's limit: the composition, silently
    "wide_3x8200": (1, 3, 8200, 48),     # wider than it: the composition, silently
}
KERNEL_CASES = tuple(k for k in CASES if CASES[k][1] <= 8192 and CASES[k][2] <= 8192)
SMALL_CASES = ("one_row", "one_col", "quads_7x7", "batch_37x37", "waves_33x5", "segment_64x9", "segment_65x9")
LONG_CASES = ("tall_8192x8", "tall_8193x4", "wide_3x8200")          # one variant each on the CPU

#: the planted columns of carry_197x260 (image 0) and its row without a source; lo is the least value in range, so with "background"
#: a planted source wins wherever it is a candidate
CARRY_TOP, CARRY_BOTTOM, CARRY_EMPTY, CARRY_CLASS, CARRY_HOLE_ROW = 100, 101, 102, 103, 131
CARRY_CLASS_ROW, CARRY_OTHER_ROWS = 10, (40, 70, 140, 195)


def make_case(name):
    """(disparity float32, label int64, label float32, keep bool) [B,H,W] of a case, built as refine_cases.make_case builds its own: a
    field on the half-pixel grid that leaves the range in places, labels in blocks of 4 x 5 pixels with 7, 8, 200, -1 sprinkled in
    (the float map: 2.5 and NaN too), keep false on a tenth of the pixels.  The holes are runs along rows, runs along columns AND
    3 x 3 blobs -- no whole no-data columns: a column that is all hole has no vertical candidate.  Planted: refine_cases' row 0 of
    image 0 (W >= 37) and the same values down column 0 (H >= 37); the special values alone on a narrower and shorter map; the last
    row of the last image without any source (H >= 3); and carry_197x260's columns."""
    B, H, W, maxdisp = CASES[name]
    g = torch.Generator().manual_seed(9800 + 13 * H + W)
    lo, hi = float(-maxdisp), float(maxdisp)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    d = torch.round((2 * torch.rand(B, H, W, generator=g) - 1) * 1.2 * maxdisp * 2) / 2
    d[torch.rand(B, H, -(-W // 7), generator=g).repeat_interleave(7, dim=2)[:, :, :W] < 0.25] = FILL
    d[torch.rand(B, -(-H // 9), W, generator=g).repeat_interleave(9, dim=1)[:, :H] < 0.15] = FILL
    d[:, (xx // 3 + 2 * (yy // 3)) % 5 == 0] = FILL
    y = torch.randint(0, 6, (B, -(-H // 4), -(-W // 5)), generator=g).repeat_interleave(4, dim=1).repeat_interleave(5, dim=2)[:, :H, :W].contiguous()
    odd = torch.tensor([7, 8, 200, -1])
    sprinkled = (xx + 3 * yy) % 13 == 3
    y[:, sprinkled] = odd[(xx + yy) % 4][sprinkled]
    yf = y.to(torch.float32)
    yf[:, (xx + 2 * yy) % 17 == 5] = 2.5
    yf[:, (xx + yy) % 19 == 6] = float("nan")
    keep = torch.rand(B, H, W, generator=g) >= 0.1
    plant_d = torch.tensor([{14: lo, 15: hi}[i] if v is None else v for i, v in enumerate(fc._PLANT_D)])
    plant_y, plant_yf = torch.tensor(fc._PLANT_Y), torch.tensor(fc._PLANT_Y, dtype=torch.float32)
    for i, v in fc._PLANT_YF.items():
        plant_yf[i] = v
    plant_keep = torch.ones(fc.PLANT_W, dtype=torch.bool)
    plant_keep[24] = False
    n = fc.PLANT_W
    if W >= n:
        d[0, 0, :n], y[0, 0, :n], yf[0, 0, :n], keep[0, 0, :n] = plant_d, plant_y, plant_yf, plant_keep
    if H >= n:
        d[0, :n, 0], y[0, :n, 0], yf[0, :n, 0], keep[0, :n, 0] = plant_d, plant_y, plant_yf, plant_keep
    if W < n and H < n:
        special = torch.tensor([float("nan"), float("inf"), float("-inf"), lo, hi, 1.0, FILL])
        d[0, 0] = special[torch.arange(W) % 7]
    if H >= 3:
        bad = torch.tensor([float("nan"), FILL, hi, float("inf"), hi + 0.5, lo - 0.5, float("-inf")])
        d[B - 1, H - 1] = bad[torch.arange(W) % len(bad)]
    if name == "carry_197x260":
        # a column whose only source is row 0, one whose only source is row H - 1, one without any source: both carries cross every
        # segment and the summary scan
        for col, row, v in ((CARRY_TOP, 0, lo), (CARRY_BOTTOM, H - 1, lo), (CARRY_EMPTY, None, None)):
            d[0, :, col] = FILL
            if row is not None:
                d[0, row, col], keep[0, row, col] = v, True
        # a column of class 3 whose only same-class source lies in the first segment, while sources of class 4 lie in every segment
        d[0, :, CARRY_CLASS], y[0, :, CARRY_CLASS], yf[0, :, CARRY_CLASS] = FILL, 3, 3.0
        d[0, CARRY_CLASS_ROW, CARRY_CLASS], keep[0, CARRY_CLASS_ROW, CARRY_CLASS] = lo, True
        for row in CARRY_OTHER_ROWS:
            d[0, row, CARRY_CLASS], y[0, row, CARRY_CLASS], yf[0, row, CARRY_CLASS], keep[0, row, CARRY_CLASS] = 2.0, 4, 4.0, True
        d[0, CARRY_HOLE_ROW] = FILL                                                    # a row without any source
    return d.contiguous(), y, yf, keep


def _least(cands, prefer):
    """The chosen candidate of one tier, None for none: cands = [(v, g, order, y*, x*)] of those within their gaps."""
    if not cands:
        return None
    if prefer == "background":
        return min(cands, key=lambda c: (c[0], c[1], c[2]))                            # (tuples of numpy float32 and ints: plain comparisons)
    return min(cands, key=lambda c: (c[1], c[0], c[2]))


def gaps(max_gap, H, W):
    if max_gap is None:
        return W, H
    return tuple(max_gap) if isinstance(max_gap, (tuple, list)) else (max_gap, max_gap)


def restate(disparity, disp_right=None, label=None, keep=None, lo=-4.0, hi=4.0, threshold=THRESHOLD, max_gap=None, prefer="background",
            fallback=True, fill_value=FILL, _stage={}):
    """{"disparity", "kind", "source", "source_row", and with disp_right "consistent"} as torch tensors, from the sequential loops."""
    d = disparity.numpy().astype(np.float32)
    B, H, W = d.shape
    lo32, hi32 = np.float32(lo), np.float32(hi)
    gap_x, gap_y = gaps(max_gap, H, W)
    key = tuple(None if t is None else id(t) for t in (disparity, disp_right, label, keep)) + (lo, hi, threshold)
    if key not in _stage:                                    # (the inputs of a case are shared and never change: see case())
        lab = None if label is None else label.numpy()
        k = None if keep is None else keep.numpy()
        ok = None if disp_right is None else rc.restate_lr(disparity, disp_right, lo, hi, threshold)[0].numpy()
        images = []
        for b in range(B):
            src = [[bool(lo32 <= d[b, h, x] < hi32) and (k is None or bool(k[b, h, x])) and (ok is None or bool(ok[b, h, x]))
                    for x in range(W)] for h in range(H)]
            cls = [[NONE if lab is None else fc.class_of(lab[b, h, x]) for x in range(W)] for h in range(H)]
            rows = [fc._candidates(src[h], cls[h]) for h in range(H)]                                   # (L own, L any, R own, R any) per row
            cols = [fc._candidates([src[h][x] for h in range(H)], [cls[h][x] for h in range(H)]) for x in range(W)]      # (U, U, D, D) per column
            images.append((src, cls, rows, cols))
        _stage[key] = (images, ok, (disparity, disp_right, label, keep))       # (the tensors are held: their ids stay theirs)
    images, ok, _ = _stage[key]
    out = np.full((B, H, W), fill_value, dtype=np.float32)
    kind = np.full((B, H, W), 3, dtype=np.uint8)
    source = np.full((B, H, W), -1, dtype=np.int32)
    source_row = np.full((B, H, W), -1, dtype=np.int32)
    for b, (src, cls, rows, cols) in enumerate(images):
        for h in range(H):
            for x in range(W):
                if src[h][x]:
                    kind[b, h, x], source[b, h, x], source_row[b, h, x], out[b, h, x] = 0, x, h, d[b, h, x]
                    continue

                def tier(own):
                    found = []
                    for order, at in enumerate((rows[h][0 if own else 1][x], rows[h][2 if own else 3][x])):          # L, R
                        if at >= 0 and abs(x - at) <= gap_x:
                            found.append((d[b, h, at], abs(x - at), order, h, at))
                    for order, at in enumerate((cols[x][0 if own else 1][h], cols[x][2 if own else 3][h]), start=2):  # U, D
                        if at >= 0 and abs(h - at) <= gap_y:
                            found.append((d[b, at, x], abs(h - at), order, at, x))
                    return _least(found, prefer)
                won, kd = None, 3
                if cls[h][x] != NONE:
                    won, kd = tier(True), 1
                if won is None and fallback:
                    won, kd = tier(False), 2
                if won is not None:
                    kind[b, h, x], source[b, h, x], source_row[b, h, x], out[b, h, x] = kd, won[4], won[3], won[0]
    res = {"disparity": torch.from_numpy(out), "kind": torch.from_numpy(kind), "source": torch.from_numpy(source),
           "source_row": torch.from_numpy(source_row)}
    if ok is not None:
        res["consistent"] = torch.from_numpy(ok.copy())
    return res


_MEMO = {}


def case(name):
    """{"d", "dr", "y", "yf", "keep", "lo", "hi", "maxdisp"} of a case, computed once and shared: leave it unchanged.  "dr" is a
    right-view estimate as refine_cases.case builds it."""
    if name not in _MEMO:
        d, y, yf, keep = make_case(name)
        maxdisp = CASES[name][3]
        lo, hi = float(-maxdisp), float(maxdisp)
        dr = rc.restate(d, None, lo, hi)["right_disparity"].clone()
        dr[..., 1::3] += 0.25
        dr[..., 5::7] = float("nan")
        _MEMO[name] = dict(d=d, dr=dr, y=y, yf=yf, keep=keep, lo=lo, hi=hi, maxdisp=maxdisp)
    return _MEMO[name]


#: ((with dR, with keep, label: None / "y" / "yf"), prefer, fallback, max_gap): the full product, and the gap pair with everything given
VARIANTS = tuple((i, p, f, None) for i in fc.INPUTS for p in ("background", "nearest") for f in (True, False)) + \
    tuple(((True, True, "y"), p, f, (3, 2)) for p in ("background", "nearest") for f in (True, False)) + \
    (((False, True, "y"), "background", True, 3),)
#: what the device tests run of them: everything given, the float label without fallback, no label, the gap pair with everything
#: given, "nearest" with the gap pair
GPU_VARIANTS = (((True, True, "y"), "background", True, None), ((False, False, "yf"), "nearest", False, None),
                ((False, False, None), "background", True, None), ((True, True, "y"), "background", True, (3, 2)),
                ((True, True, "y"), "nearest", True, (3, 2)))


def keys(sa, variant):
    return sa.REFINE_KEYS_2D if variant[0][0] else ("disparity", "kind", "source", "source_row")


def call(sa, c, variant, want=None, move=lambda t: t, axes="both"):
    """The package on a variant: refine_disparity with dR, fill_disparity without; `move` takes every tensor to its device."""
    (d, dr), kw = fc.arguments(c, variant)
    kw = {k: move(v) if isinstance(v, torch.Tensor) else v for k, v in kw.items()}
    if axes is not None:
        kw["axes"] = axes
    if axes != "both" and isinstance(kw["max_gap"], tuple):
        kw["max_gap"] = kw["max_gap"][0]                                                # (the rows call takes the columns' gap)
    if dr is None:
        return sa.fill_disparity(move(d), disp_range=(c["lo"], c["hi"]), want=want or keys(sa, variant), **kw)
    return sa.refine_disparity(move(d), move(dr), threshold=THRESHOLD, disp_range=(c["lo"], c["hi"]), want=want or keys(sa, variant), **kw)


def expected(c, variant):
    (d, dr), kw = fc.arguments(c, variant)
    return restate(d, dr, lo=c["lo"], hi=c["hi"], **kw)


def closed_forms():
    """(what, disparity [1,H,W], label or None, keyword arguments, disparity, kind, source, source_row) as literals, maxdisp = 4."""
    F = FILL
    t = lambda v, dtype=torch.float32: torch.tensor(v, dtype=dtype).unsqueeze(0)          # noqa: E731
    own = lambda H, W: ([[x for x in range(W)] for _ in range(H)], [[h] * W for h in range(H)])          # noqa: E731
    forms = []
    # two rows of holes between a row of 3.0 above and a row of 1.0 below: "background" takes the smaller, 1.0, for both ...
    d = [[3.0] * 3, [F] * 3, [F] * 3, [1.0] * 3]
    sx, sy = own(4, 3)
    forms.append(("rows_between_background", d, [[0] * 3] * 4, {}, [[3.0] * 3, [1.0] * 3, [1.0] * 3, [1.0] * 3],
                  [[0] * 3, [1] * 3, [1] * 3, [0] * 3], sx, [[0] * 3, [3] * 3, [3] * 3, [3] * 3]))
    # ... "nearest" the nearer one: row 1 from above, row 2 from below
    forms.append(("rows_between_nearest", d, [[0] * 3] * 4, {"prefer": "nearest"}, [[3.0] * 3, [3.0] * 3, [1.0] * 3, [1.0] * 3],
                  [[0] * 3, [1] * 3, [1] * 3, [0] * 3], sx, [[0] * 3, [0] * 3, [3] * 3, [3] * 3]))
    # a class-1 hole with class-2 neighbours left and right and a class-1 source three rows up takes that source (today's call: 0.5,
    # kind 2, see test_fill2d.py)
    d = [[2.0, 3.0, 2.0], [2.0, 2.0, 2.0], [2.0, 2.0, 2.0], [1.0, F, 0.5]]
    y = [[2, 1, 2], [2, 2, 2], [2, 2, 2], [2, 1, 2]]
    sx, sy = own(4, 3)
    sy[3][1] = 0
    forms.append(("same_class_three_rows_up", d, y, {}, d[:3] + [[1.0, 3.0, 0.5]], [[0] * 3] * 3 + [[0, 1, 0]], sx, sy))
    # a four-way tie in value and distance takes L, and -0.0 == 0.0: the sign of L is kept
    for what, l, others in (("four_way_tie_minus_zero", -0.0, 0.0), ("four_way_tie_plus_zero", 0.0, -0.0)):
        d = [[1.0, others, 1.0], [l, F, others], [1.0, others, 1.0]]
        sx, sy = own(3, 3)
        sx[1][1] = 0
        forms.append((what, d, [[0] * 3] * 3, {}, [d[0], [l, l, others], d[2]], [[0] * 3, [0, 1, 0], [0] * 3], sx, sy))
    # max_gap = (W, 1) drops a source two rows away
    sx, sy = [[0], [0], [-1], [-1]], [[0], [0], [-1], [-1]]
    forms.append(("gap_of_one_row", [[2.0], [F], [F], [F]], None, {"max_gap": (1, 1)}, [[2.0], [2.0], [F], [F]], [[0], [2], [3], [3]], sx, sy))
    # fallback=False leaves a pixel of class NONE unfilled
    d = [[1.0] * 3, [1.0, F, 1.0], [1.0] * 3]
    sx, sy = own(3, 3)
    sx[1][1] = sy[1][1] = -1
    forms.append(("none_without_fallback", d, [[0] * 3, [0, 8, 0], [0] * 3], {"fallback": False}, d, [[0] * 3, [0, 3, 0], [0] * 3], sx, sy))
    return [(what, t(d), None if y is None else t(y, torch.int64), kw, t(out), t(kind, torch.uint8), t(sx, torch.int32), t(sy, torch.int32))
            for what, d, y, kw, out, kind, sx, sy in forms]


def blob_batch():
    """(disparity float32 [4,1024,1024], label uint8) on the host: refine_cases.full_batch() with its no-data columns replaced by
    12 x 12 hole blobs, its rows without a source kept, and one hole of 600 rows x 610 columns in image 0."""
    g = torch.Generator().manual_seed(9700)
    yy, xx = torch.meshgrid(torch.arange(1024.0), torch.arange(1024.0), indexing="ij")
    maps = []
    for b in range(4):
        smooth = 20 * torch.sin(xx / (37.0 + 9 * b)) * torch.cos(yy / 61.0) + 0.01 * (b + 1) * xx
        steps = 14.0 * ((xx // (96 + 32 * b)) % 3) - 14.0
        maps.append(torch.round(2 * (smooth + steps)) / 2)
    d = torch.stack(maps)
    yi, xi = yy.long(), xx.long()
    d[:, ((xi // 12 + 2 * (yi // 12)) % 7 == 0) | (((xi // 40) % 9 == 3) & ((yi // 24) % 2 == 0))] = FILL
    d[:, 5::97] += 0.25
    d[:, 7::113] = FILL                                                 # rows without a source
    d[0, 200:800, 200:810] = FILL
    blocks = torch.randint(0, 6, (4, 16, 16), generator=g, dtype=torch.uint8)
    label = blocks.repeat_interleave(64, dim=1).repeat_interleave(64, dim=2).contiguous()
    label[:, :, 5::29] = 200
    return d, label


def blob_conditions(both, rows):
    """The conditions on the blob fixture, from the two calls' outputs (kind, source_row / kind): every kind has a positive share, some
    pixels the rows call leaves unfilled are filled, some move from kind 2 to kind 1, a vertical candidate wins on some pixels the
    rows call fills too, some stay unfilled."""
    kb, kr = both["kind"], rows["kind"]
    H = kb.shape[1]
    own_row = torch.arange(H, device=kb.device).view(1, H, 1)
    shares = [float((kb == k).float().mean()) for k in range(4)]
    assert all(s > 0 for s in shares), shares
    assert bool(((kr == 3) & (kb < 3)).any()) and bool(((kr == 2) & (kb == 1)).any())
    assert bool(((kr != 0) & (kr != 3) & (kb != 3) & (both["source_row"] != own_row)).any())
    assert bool((kb == 3).any())
    assert bool((kb <= kr).all())
    return shares


# ------------------------------------------------------------------------------------------------ SceneStereo(refine=dict(axes="both"))
REFINE = dict(fc.REFINE, axes="both", max_gap=(12, 8))


def check_scene(sa, stereo_with, stereo_without, left, right):
    """SceneStereo(refine=dict(..., axes="both")) against one direct refine_disparity(..., axes="both") call over the mosaics; returns
    the refined dictionary.  The pattern of refine_cases.check_scene."""
    base = ("disparity", "label", "spread")
    forth, back = stereo_without(left, right, want=("disparity", "label")), stereo_without(right, left, want=("disparity",))
    want = sa.refine_disparity(forth["disparity"], -back["disparity"], forth["label"], want=("disparity", "kind", "consistent"), **REFINE)
    rows = sa.refine_disparity(forth["disparity"], -back["disparity"], forth["label"], want=("kind",), **dict(REFINE, axes="rows", max_gap=12))
    got = stereo_with(left, right, want=base + fc.NEW)
    assert tuple(got) == base + fc.NEW
    assert torch.equal(got["disparity"], forth["disparity"]) and torch.equal(got["disparity_right"], -back["disparity"])
    assert torch.equal(got["disparity_refined"], want["disparity"]) and torch.equal(got["kind"], want["kind"])
    assert torch.equal(got["consistent"], want["consistent"]) and got["consistent"].dtype == torch.bool
    assert bool((got["kind"] <= rows["kind"]).all())
    return got
