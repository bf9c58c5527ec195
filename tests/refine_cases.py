"""What the refinement tests share (test infrastructure, like right_view_cases.py): the case table, the planted values and a SEQUENTIAL
restatement of the definitions of include/semstereo_hip.h (section "disparity refinement"), written for these tests from those
definitions: per row a raster loop that carries the last source column per class (and of any class) forward, the same loop backward,
then max_gap, the tiers and the choice pixel by pixel.  All arithmetic is numpy float32 scalars; the left-right check is
right_view_cases.restate_lr (its _targets), nothing of it is restated here."""
import itertools

import numpy as np
import torch

import right_view_cases as rc

FILL = -999.0
NONE = 8                                         # the class of a pixel without one
THRESHOLD = 0.25                                 # of the cases' left-right check: right_estimate moves a third of the columns by 0.25
BLOCK = 256                                      # csrc/stream.h

#: name -> (B, H, W, maxdisp).  The kernel gives thread t the columns [t * chunk, (t + 1) * chunk) with chunk = ceil(W / 256) rounded up
#: to 4, and reads a row in quads of 4 columns, 256 quads per trip: the shapes are the smallest at which each of those can go wrong.
CASES = {
    "quads_w7": (1, 3, 7, 4),            # less than two quads, W % 4 == 3: two threads hold all columns, 254 chunks are empty
    "batch_w37": (2, 5, 37, 8),          # batch and row indexing, odd W; thread 9's chunk is partial (one column)
    "full_w1024": (1, 6, 1024, 48),      # the widest row with chunk 4: every chunk full, the last thread's too; exactly one trip
    "chunk8_w1025": (1, 6, 1025, 48),    # the chunk length changes to 8: thread 128 holds ONE column, threads 129 .. 255 none
    "trips_w1030": (1, 4, 1030, 48),     # a lane makes a second row-quad trip; ragged chunks (thread 128: 6 of 8); W % 4 == 2
    "chunk16_w4096": (1, 4, 4096, 48),   # chunk 16, the benchmark's mosaic width: four flag words and four candidate quads per thread
    "chunk32_w8192": (1, 3, 8192, 48),   # the widest row the kernel takes: chunk 32, 73.9 KB of LDS (above the 64 KB a launch has by default)
    "wide_w8200": (1, 3, 8200, 48),      # wider than the kernel's limit: the composition, silently
}
KERNEL_CASES = tuple(k for k in CASES if CASES[k][2] <= 8192)

#: the planted row 0 of image 0 for W >= 37 (columns 0 .. 34), with lo = -maxdisp and hi = maxdisp; H_ = a hole
#:   0-5    a tie in disparity: holes 1, 2 between equal sources 0 and 3 (unequal distances: the nearer), hole 4 between 3 and 5 (equal: the left)
#:   6-10   -0.0 against 0.0: hole 7 between -0.0 and 0.0, hole 9 between 0.0 and -0.0 (equal values, equal distances: the left, sign kept)
#:   11-15  NaN, +inf, -inf (holes), d == lo (kept), d == hi (a hole)
#:   16-23  labels 5 and 7 are ordinary classes; 8, 200, -1 (float map: 2.5, 200, NaN) are none: tier 2, which the none-class source 23 serves
#:   24-25  keep false on the in-range pixel 24
#:   26-34  sources 26 (class 4) and 34 (class 0), seven holes of class 4 between them: with max_gap = 3 hole 27 is tier 1, hole 30 has its
#:          same-class and its any-class candidates beyond the gap (unfilled), hole 31 only its same-class one (tier 2 from 34)
_H = FILL
_PLANT_D = [1.0, _H, _H, 1.0, _H, 1.0, -0.0, _H, 0.0, _H, -0.0, float("nan"), float("inf"), float("-inf"), None, None,
            2.0, _H, 3.0, _H, _H, _H, _H, 4.0, 1.5, 0.5, 5.0, _H, _H, _H, _H, _H, _H, _H, 6.0]
_PLANT_Y = [1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 5, 5, 7, 7, 8, 200, -1, 8, 0, 0, 4, 4, 4, 4, 4, 4, 4, 4, 0]
_PLANT_YF = {20: 2.5, 21: 200.0, 22: float("nan")}
PLANT_W = len(_PLANT_D)


def make_case(name):
    """(disparity float32, label int64, label float32, keep bool) [B,H,W] of a case.  Everywhere: a field on the half-pixel grid that leaves
    the range in places, no-data columns x % 11 == 10 and runs of holes, labels in runs of 5 columns with 7, 8, 200, -1 sprinkled in
    (the float map: 2.5 and NaN too), keep false on a tenth of the pixels.  Planted: row 0 of image 0 (see _PLANT_D; W = 7 gets the
    special values only), row 1 with x = 0 as its only source and (H >= 4) row 2 with x = W - 1 as its only source -- every other
    pixel of those rows a hole, a run longer than 4 * BLOCK columns in the wide cases, the carry crossing every thread and all four
    waves -- and the last row of the last image without any source."""
    B, H, W, maxdisp = CASES[name]
    g = torch.Generator().manual_seed(9600 + W)
    lo, hi = float(-maxdisp), float(maxdisp)
    d = torch.round((2 * torch.rand(B, H, W, generator=g) - 1) * 1.2 * maxdisp * 2) / 2
    d[:, :, 10::11] = FILL
    runs = torch.rand(B, H, -(-W // 7), generator=g).repeat_interleave(7, dim=2)[:, :, :W] < 0.3
    d[runs] = FILL
    y = torch.randint(0, 6, (B, H, -(-W // 5)), generator=g).repeat_interleave(5, dim=2)[:, :, :W].contiguous()
    odd = torch.tensor([7, 8, 200, -1])
    y[:, :, 3::13] = odd[torch.arange(len(range(3, W, 13))) % 4]
    yf = y.to(torch.float32)
    yf[:, :, 5::17] = 2.5
    yf[:, :, 6::19] = float("nan")
    keep = torch.rand(B, H, W, generator=g) >= 0.1
    if W >= PLANT_W:
        for x, v in enumerate(_PLANT_D):
            d[0, 0, x] = {14: lo, 15: hi}[x] if v is None else v
        y[0, 0, :PLANT_W] = torch.tensor(_PLANT_Y)
        yf[0, 0, :PLANT_W] = torch.tensor(_PLANT_Y, dtype=torch.float32)
        for x, v in _PLANT_YF.items():
            yf[0, 0, x] = v
        keep[0, 0, :PLANT_W] = True
        keep[0, 0, 24] = False
    else:
        d[0, 0] = torch.tensor([float("nan"), float("inf"), float("-inf"), lo, hi, 1.0, FILL])[:W]
    d[0, 1], d[0, 1, 0] = FILL, 1.0
    keep[0, 1, 0] = True
    if H >= 4:
        d[0, 2], d[0, 2, W - 1] = FILL, -1.0
        keep[0, 2, W - 1] = True
    bad = torch.tensor([float("nan"), FILL, hi, float("inf"), hi + 0.5, lo - 0.5, float("-inf")])
    d[B - 1, H - 1] = bad[torch.arange(W) % len(bad)]
    return d.contiguous(), y, yf, keep


def class_of(v):
    """class[x] of a label value (a numpy scalar of any dtype): int(v) for an integer-valued 0 <= v < 8, else NONE."""
    if not (0 <= v < 8):                                     # (False for a NaN)
        return NONE
    return int(v) if v == np.trunc(v) else NONE


def _pick(x, L, R, row, max_gap, prefer):
    """The winning candidate of one tier, -1 for none: L, R columns or -1."""
    if L >= 0 and x - L > max_gap:
        L = -1
    if R >= 0 and R - x > max_gap:
        R = -1
    if L < 0 or R < 0:
        return max(L, R)
    dl, dr = row[L], row[R]                                  # numpy float32 scalars: plain fp32 comparisons
    if prefer == "background":
        right = dr < dl or (dr == dl and R - x < x - L)
    else:
        right = R - x < x - L or (R - x == x - L and dr < dl)
    return R if right else L


def _candidates(src, cls):
    """Per pixel (left own-class, left any, right own-class, right any) source columns, -1 for none: the two raster loops."""
    W = len(src)
    out = [[-1] * W for _ in range(4)]
    for first, second, order in ((0, 1, range(W)), (2, 3, range(W - 1, -1, -1))):
        last = [-1] * (NONE + 1)                             # per class 0 .. 7, and of any class
        for x in order:
            if cls[x] != NONE:
                out[first][x] = last[cls[x]]
            out[second][x] = last[NONE]
            if src[x]:
                last[NONE] = x
                if cls[x] != NONE:
                    last[cls[x]] = x
    return out


def restate(disparity, disp_right=None, label=None, keep=None, lo=-4.0, hi=4.0, threshold=THRESHOLD, max_gap=None, prefer="background",
            fallback=True, fill_value=FILL, _stage={}):
    """{"disparity", "kind", "source", and with disp_right "consistent"} as torch tensors, from the sequential loops."""
    d = disparity.numpy().astype(np.float32)
    B, H, W = d.shape
    lo32, hi32 = np.float32(lo), np.float32(hi)
    max_gap = W if max_gap is None else max_gap
    key = tuple(None if t is None else id(t) for t in (disparity, disp_right, label, keep)) + (lo, hi, threshold)
    if key not in _stage:                                    # (the inputs of a case are shared and never change: see case())
        y = None if label is None else label.numpy()
        k = None if keep is None else keep.numpy()
        ok = None if disp_right is None else rc.restate_lr(disparity, disp_right, lo, hi, threshold)[0].numpy()
        rows = []
        for b in range(B):
            for h in range(H):
                row = d[b, h]
                src = [bool(lo32 <= row[x] < hi32) and (k is None or bool(k[b, h, x])) and (ok is None or bool(ok[b, h, x])) for x in range(W)]
                cls = [NONE if y is None else class_of(y[b, h, x]) for x in range(W)]
                rows.append((src, cls, _candidates(src, cls)))
        _stage[key] = (rows, ok, (disparity, disp_right, label, keep))       # (the tensors are held: their ids stay theirs)
    rows, ok, _ = _stage[key]
    out = np.full((B, H, W), fill_value, dtype=np.float32)
    kind = np.full((B, H, W), 3, dtype=np.uint8)
    source = np.full((B, H, W), -1, dtype=np.int32)
    for r, (src, cls, (lown, lany, rown, rany)) in enumerate(rows):
        b, h = divmod(r, H)
        row = d[b, h]
        for x in range(W):
            if src[x]:
                s, kd = x, 0
            else:
                s, kd = -1, 3
                if cls[x] != NONE:
                    s, kd = _pick(x, lown[x], rown[x], row, max_gap, prefer), 1
                if s < 0 and fallback:
                    s, kd = _pick(x, lany[x], rany[x], row, max_gap, prefer), 2
                if s < 0:
                    kd = 3
            kind[b, h, x], source[b, h, x] = kd, s
            if s >= 0:
                out[b, h, x] = row[s]
    res = {"disparity": torch.from_numpy(out), "kind": torch.from_numpy(kind), "source": torch.from_numpy(source)}
    if ok is not None:
        res["consistent"] = torch.from_numpy(ok.copy())
    return res


_MEMO = {}


def case(name):
    """{"d", "dr", "y", "yf", "keep", "lo", "hi", "maxdisp"} of a case, computed once and shared: leave it unchanged.  "dr" is a right-view
    estimate as right_view_cases.right_estimate builds it: the case's own right view, every third column moved by a quarter (still
    consistent at THRESHOLD) and some made invalid."""
    if name not in _MEMO:
        d, y, yf, keep = make_case(name)
        maxdisp = CASES[name][3]
        lo, hi = float(-maxdisp), float(maxdisp)
        dr = rc.restate(d, None, lo, hi)["right_disparity"].clone()
        dr[..., 1::3] += 0.25
        dr[..., 5::7] = float("nan")
        _MEMO[name] = dict(d=d, dr=dr, y=y, yf=yf, keep=keep, lo=lo, hi=hi, maxdisp=maxdisp)
    return _MEMO[name]


#: (with dR, with keep, label: None / "y" / "yf") x prefer x fallback, max_gap None; and the finite gap with everything given
INPUTS = tuple(itertools.product((False, True), (False, True), (None, "y", "yf")))
VARIANTS = tuple((i, p, f, None) for i in INPUTS for p in ("background", "nearest") for f in (True, False)) + \
    tuple(((True, True, "y"), p, f, 3) for p in ("background", "nearest") for f in (True, False)) + \
    (((False, True, "y"), "background", True, 3),)
#: what the device tests run of them: everything at once, the float map without a fallback, nothing but the map, the finite gap
GPU_VARIANTS = (((True, True, "y"), "background", True, None), ((False, False, "yf"), "nearest", False, None),
                ((False, False, None), "background", True, None), ((False, True, "y"), "background", True, 3))


def arguments(c, variant):
    """(positional tensors (d, dr or None), keyword arguments) of a variant of case dictionary c, for the package and for restate."""
    (with_dr, with_keep, which), prefer, fallback, max_gap = variant
    kw = dict(label=None if which is None else c[which], keep=c["keep"] if with_keep else None, max_gap=max_gap, prefer=prefer,
              fallback=fallback)
    return (c["d"], c["dr"] if with_dr else None), kw


def call(sa, c, variant, want=None, move=lambda t: t):
    """The package on a variant: refine_disparity with dR, fill_disparity without; `move` takes every tensor to its device."""
    (d, dr), kw = arguments(c, variant)
    kw = {k: move(v) if isinstance(v, torch.Tensor) else v for k, v in kw.items()}
    if dr is None:
        return sa.fill_disparity(move(d), disp_range=(c["lo"], c["hi"]), want=want or ("disparity", "kind", "source"), **kw)
    return sa.refine_disparity(move(d), move(dr), threshold=THRESHOLD, disp_range=(c["lo"], c["hi"]), want=want or sa.REFINE_KEYS, **kw)


def expected(c, variant):
    (d, dr), kw = arguments(c, variant)
    return restate(d, dr, lo=c["lo"], hi=c["hi"], **kw)


def closed_forms():
    """(what, disparity [1,1,10], label or None, keyword arguments, disparity, kind, source) as literals, maxdisp = 4."""
    F = FILL
    t = lambda v, dtype=torch.float32: torch.tensor(v, dtype=dtype).view(1, 1, -1)        # noqa: E731
    step_down = [f for f in rc.closed_forms() if f[0] == "step_down"][0][4]          # its right view: [0] * 5 + [F] * 2 + [-2] * 3
    forms = [
        # the two holes a step down leaves in the right view lie between the surfaces 0 and -2: the background (-2) fills both
        ("step_down", step_down, None, {}, [0.0] * 5 + [-2.0] * 5, [0] * 5 + [2, 2] + [0] * 3, [0, 1, 2, 3, 4, 7, 7, 7, 8, 9]),
        # the hole x = 2 of class 1 between sources of class 2 at x = 1 and x = 3: it takes the class-1 source x = 0 across them
        ("same_class_across", t([3.0, 1.0, F, 0.5, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0]), t([1, 2, 1, 2, 0, 0, 0, 0, 0, 0], torch.int64), {},
         [3.0, 1.0, 3.0, 0.5] + [2.0] * 6, [0, 0, 1] + [0] * 7, [0, 1, 0, 3, 4, 5, 6, 7, 8, 9]),
        # ... and without its class it is an ordinary hole: the smaller of the neighbours 1.0 and 0.5
        ("same_class_across_unlabelled", t([3.0, 1.0, F, 0.5, 2.0, 2.0, 2.0, 2.0, 2.0, 2.0]), None, {},
         [3.0, 1.0, 0.5, 0.5] + [2.0] * 6, [0, 0, 2] + [0] * 7, [0, 1, 3, 3, 4, 5, 6, 7, 8, 9]),
        # holes 1..3 between 1.0 at x = 0 and 3.0 at x = 4: the background takes 1.0 for all three
        ("background_side", t([1.0, F, F, F] + [3.0] * 6), t([0] * 10, torch.int64), {},
         [1.0] * 4 + [3.0] * 6, [0, 1, 1, 1] + [0] * 6, [0, 0, 0, 0, 4, 5, 6, 7, 8, 9]),
        # ... "nearest" the other side for x = 3 (x = 2 is equally far from both: the smaller disparity)
        ("nearest_side", t([1.0, F, F, F] + [3.0] * 6), t([0] * 10, torch.int64), {"prefer": "nearest"},
         [1.0] * 3 + [3.0] * 7, [0, 1, 1, 1] + [0] * 6, [0, 0, 0, 4, 4, 5, 6, 7, 8, 9]),
    ]
    return [(what, d, y, kw, t(out), t(kind, torch.uint8), t(src, torch.int32)) for what, d, y, kw, out, kind, src in forms]


def full_batch():
    """(disparity float32 [4,1024,1024], label uint8) on the host, built like test_right_view_gpu.py's `full` fixture -- a smooth field
    plus steps on the half-pixel grid, no-data columns -- plus rows without any valid value (unfilled pixels) and a label map of
    64 x 64 blocks with a no-class value sprinkled in (tier 2)."""
    g = torch.Generator().manual_seed(9700)
    yy, xx = torch.meshgrid(torch.arange(1024.0), torch.arange(1024.0), indexing="ij")
    maps = []
    for b in range(4):
        smooth = 20 * torch.sin(xx / (37.0 + 9 * b)) * torch.cos(yy / 61.0) + 0.01 * (b + 1) * xx
        steps = 14.0 * ((xx // (96 + 32 * b)) % 3) - 14.0
        maps.append(torch.round(2 * (smooth + steps)) / 2)
    d = torch.stack(maps)
    d[:, :, 10::11] = FILL
    d[:, 5::97] += 0.25
    d[:, 7::113] = FILL                                                 # rows without a source
    blocks = torch.randint(0, 6, (4, 16, 16), generator=g, dtype=torch.uint8)
    label = blocks.repeat_interleave(64, dim=1).repeat_interleave(64, dim=2).contiguous()
    label[:, :, 5::29] = 200
    return d, label


def same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        a, b = (got[k].view(torch.int32), want[k].view(torch.int32)) if k == "disparity" else (got[k], want[k])      # bits: -0.0 is not 0.0
        assert torch.equal(a, b), f"{what} {k}: {(a != b).sum().item()} of {b.numel()} values differ"


# ------------------------------------------------------------------------------------------------ SceneStereo(refine=)
COMBOS = torch.tensor([[1.0, 0.5, -0.25], [-0.5, 1.0, 0.25], [0.25, -1.0, 0.5], [0.75, 0.25, -1.0], [-1.0, 0.5, 0.5], [0.5, -0.75, 1.0]])
REFINE = dict(maxdisp=4, threshold=1.0, max_gap=12, prefer="background", fallback=True)
NEW = ("disparity_right", "consistent", "disparity_refined", "kind")


def per_pixel_model(first, second):
    """A callable with the reference's eval convention: a disparity of a few pixels from the two views, logits from the first alone."""
    disp = 1.5 * (first[:, 0] - second[:, 0])
    logits = torch.stack([sum(float(COMBOS[k, c]) * first[:, c] for c in range(3)) for k in range(6)], dim=1)
    return [disp], logits


def scene_pair(H, W, seed=7):
    """Smooth views (blocks of 4 x 4 pixels), so that neighbouring pixels agree often enough for the check to pass somewhere."""
    g = torch.Generator().manual_seed(seed)
    small = torch.randint(0, 256, (2, -(-H // 4), -(-W // 4), 3), generator=g, dtype=torch.uint8)
    big = small.repeat_interleave(4, dim=1).repeat_interleave(4, dim=2)[:, :H, :W].contiguous()
    return big[0], (big[0] // 2 + big[1] // 8).contiguous()


def check_scene(sa, stereo_with, stereo_without, left, right):
    """SceneStereo(refine=) against two plain calls and one refine_disparity call; returns the refined dictionary."""
    base = ("disparity", "label", "spread")
    today = stereo_without(left, right)
    plain = stereo_with(left, right)
    assert tuple(plain) == tuple(today) == base
    for k in base:
        assert torch.equal(plain[k], today[k]), k
    forth, back = stereo_without(left, right, want=("disparity", "label")), stereo_without(right, left, want=("disparity",))
    want = sa.refine_disparity(forth["disparity"], -back["disparity"], forth["label"], want=("disparity", "kind", "consistent"), **REFINE)
    got = stereo_with(left, right, want=base + NEW)
    assert tuple(got) == base + NEW and 1 <= stereo_with.peak_resident_tile_rows <= 3
    for k in base:
        assert torch.equal(got[k], today[k]), k
    assert torch.equal(got["disparity_right"], -back["disparity"])
    assert torch.equal(got["disparity_refined"], want["disparity"]) and torch.equal(got["kind"], want["kind"])
    assert torch.equal(got["consistent"], want["consistent"]) and got["consistent"].dtype == torch.bool
    only = stereo_with(left, right, want=("kind", "count"))              # neither mosaic asked for: they are built all the same
    assert tuple(only) == ("kind", "count") and torch.equal(only["kind"], want["kind"])
    return got
