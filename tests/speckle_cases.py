"""What the speckle tests share (test infrastructure, like median_cases.py): the case table and a SEQUENTIAL restatement of the
definitions of include/semstereo_hip.h (section "disparity refinement: speckle removal"), written for these tests from those
definitions and from neither product path: the two link masks as comparisons of numpy float32 arrays (one subtraction each), then a
plain flood fill in raster order over Python lists -- the first pixel of a component that the raster meets is its smallest index."""
import numpy as np
import torch

from semstereo_amd.refine import SPECKLE_TILE

FILL = -999.0
NONE = 8                                         # the class of a pixel without one
LO, HI = -8.0, 8.0
TH, TW = SPECKLE_TILE                            # csrc/disparity_speckle.hip: the pixels of a workgroup's tile
KEYS = ("disparity", "speckle", "size", "component")


def classes(label):
    """int64 numpy array: int(v) for an integer-valued 0 <= v < 8, else NONE (a NaN fails the first comparison)."""
    y = label.numpy()
    with np.errstate(invalid="ignore"):
        inside = (y >= 0) & (y < 8) & (y == np.trunc(y))
    return np.where(inside, np.where(inside, y, 0).astype(np.int64), NONE)


def _components(d, label, lo, hi, max_diff, same_class, _stage={}):
    """(component int32, size int32, valid bool) numpy [B,H,W]: what does not depend on `where`, max_size and fill_value.  Computed
    once per (map, label, range, max_diff, same_class) -- the inputs of a case are shared and never change."""
    same_class = bool(same_class and label is not None)
    ident = (id(d), None if label is None else id(label), lo, hi, max_diff, same_class)
    if ident not in _stage:
        a = d.numpy()
        B, H, W = a.shape
        with np.errstate(invalid="ignore"):
            valid = (a >= np.float32(lo)) & (a < np.float32(hi))
            right = valid[:, :, :-1] & valid[:, :, 1:] & (np.abs(a[:, :, :-1] - a[:, :, 1:]) <= np.float32(max_diff))
            down = valid[:, :-1] & valid[:, 1:] & (np.abs(a[:, :-1] - a[:, 1:]) <= np.float32(max_diff))
        if same_class:
            c = classes(label)
            right &= c[:, :, :-1] == c[:, :, 1:]
            down &= c[:, :-1] == c[:, 1:]
        comp = np.full((B, H * W), -1, dtype=np.int32)
        size = np.zeros((B, H * W), dtype=np.int32)
        for b in range(B):
            ok = valid[b].reshape(-1).tolist()
            r = np.concatenate([right[b], np.zeros((H, 1), dtype=bool)], axis=1).reshape(-1).tolist()      # p links p + 1
            dn = np.concatenate([down[b], np.zeros((1, W), dtype=bool)], axis=0).reshape(-1).tolist()     # p links p + W
            seen = [False] * (H * W)
            for first in range(H * W):
                if not ok[first] or seen[first]:
                    continue
                seen[first] = True
                members, stack = [], [first]
                while stack:
                    p = stack.pop()
                    members.append(p)
                    for q, linked in ((p + 1, r[p]), (p + W, dn[p]), (p - 1, p % W > 0 and r[p - 1]), (p - W, p >= W and dn[p - W])):
                        if linked and not seen[q]:
                            seen[q] = True
                            stack.append(q)
                assert min(members) == first
                comp[b, members] = first
                size[b, members] = len(members)
        _stage[ident] = (comp.reshape(B, H, W), size.reshape(B, H, W), valid, (d, label))       # (the tensors are held: their ids stay theirs)
    return _stage[ident][:3]


def restate(d, label=None, where=None, lo=LO, hi=HI, max_diff=1.0, max_size=0, same_class=True, fill_value=FILL):
    """{"disparity", "speckle", "size", "component"} as torch tensors, from the flood fill."""
    comp, size, valid = _components(d, label, lo, hi, max_diff, same_class)
    speckle = valid & (size <= max_size)
    if where is not None:
        speckle = speckle & (where.numpy() != 0)
    out = d.numpy().view(np.int32).copy()
    out[speckle] = np.float32(fill_value).view(np.int32)
    return {"disparity": torch.from_numpy(out.view(np.float32)), "speckle": torch.from_numpy(speckle), "size": torch.from_numpy(size.copy()),
            "component": torch.from_numpy(comp.copy())}


# ------------------------------------------------------------------------------------------------ the cases
def _random(B, H, W):
    """Blocks of 12 x 20 pixels on four levels 3 apart plus noise of up to 1.15 (neighbours of a block link mostly, not always: sizes
    from 1 to hundreds), labels 0 .. 8 in blocks of 10 x 14 with 255 sprinkled in (8 and 255 are none), no-data columns and runs, and in
    row 0 of image 0 the special values; `where` false on a third of the pixels."""
    g = torch.Generator().manual_seed(9900 + 131 * H + W)
    level = torch.randint(0, 4, (B, -(-H // 12), -(-W // 20)), generator=g).repeat_interleave(12, dim=1).repeat_interleave(20, dim=2)[:, :H, :W]
    d = (3.0 * level - 6.0 + 1.15 * torch.rand(B, H, W, generator=g)).contiguous()
    d[:, :, 10::11] = FILL
    d[torch.rand(B, H, -(-W // 7), generator=g).repeat_interleave(7, dim=2)[:, :, :W] < 0.15] = FILL
    y = torch.randint(0, 9, (B, -(-H // 10), -(-W // 14)), generator=g).repeat_interleave(10, dim=1).repeat_interleave(14, dim=2)[:, :H, :W].contiguous()
    y[:, :, 3::13] = 255
    special = torch.tensor([float("nan"), FILL, 9.0, -0.0, 0.0, -0.0, float("inf"), HI, LO, LO, float("-inf"), 0.5])
    d[0, 0, :len(special)] = special
    y[0, 0, :len(special)] = 2
    where = torch.rand(B, H, W, generator=g) >= 1 / 3
    return dict(d=d, y=y, where=where, sizes=(0, 1, 7, 40, 200, 10 ** 6), both=True)


def _serpentine():
    H, W = 2 * TH + 1, 2 * TW + 1
    d = torch.full((1, H, W), FILL)
    d[0, 0::2] = 1.0
    d[0, 1::4, W - 1] = 1.0                      # rows 1, 5, 9 ... link at the right end, rows 3, 7, 11 ... at the left
    d[0, 3::4, 0] = 1.0
    return dict(d=d, sizes=(0, (H + 1) // 2 * W + H // 2 - 1, (H + 1) // 2 * W + H // 2))


def _u_across_tiles():
    d = torch.full((1, 2 * TH, TW), FILL)
    d[0, 2:TH, 3] = 2.0                          # two bars inside the upper tile ...
    d[0, 2:TH, 10] = 2.0
    d[0, TH, 3:11] = 2.0                         # ... joined only by a row of the tile below
    return dict(d=d, sizes=(0, 2 * (TH - 2) + 7, 2 * (TH - 2) + 8))


def _tile_corner():
    d = torch.full((3, 2 * TH, 2 * TW), FILL)
    a, b = TH - 1, TW - 1                        # the four pixels around the interior corner: (a, b) (a, b + 1) / (a + 1, b) (a + 1, b + 1)
    d[0, a, b] = d[0, a + 1, b + 1] = 1.0        # one diagonal: two components of size 1
    d[1, a, b + 1] = d[1, a + 1, b] = 1.0        # the other
    d[2, a, b] = d[2, a, b + 1] = d[2, a + 1, b + 1] = 1.0          # an L: one component of 3
    return dict(d=d, sizes=(0, 1, 2, 3))


def _checkerboard():
    H, W = TH + 2, TW + 3
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return dict(d=(2.0 * ((yy + xx) % 2)).view(1, H, W).contiguous(), sizes=(0, 1))


def _threshold():
    W = 2 * TW
    d = torch.full((1, 5, W), FILL)
    d[0, 0] = 0.5 * torch.arange(W)              # a chain 0, 0.5, 1.0 ... across the tile boundary: one component
    above = float(np.nextafter(np.float32(0.5), np.float32(np.inf)))
    d[0, 2, 0:2] = torch.tensor([0.25, 0.75])    # exactly max_diff apart: linked
    d[0, 2, 3:5] = torch.tensor([0.0, above])    # the next float32 above it: not linked
    d[0, 2, TW - 1:TW + 1] = torch.tensor([above, 0.0])             # ... nor across the tile boundary
    d[0, 4, TW - 1:TW + 1] = torch.tensor([1.0, 0.5])               # ... where exactly max_diff is
    return dict(d=d, max_diff=0.5, lo=-1.0, hi=100.0, sizes=(0, 1, 2, W))


def _batch():
    return dict(d=torch.full((3, TH + 1, TW + 1), 1.0), sizes=(0, (TH + 1) * (TW + 1) - 1, (TH + 1) * (TW + 1)))


def _thin(H, W):
    i = torch.arange(H * W)
    d = (3.0 * ((i // 5) % 2) + 0.25 * (i % 3)).view(1, H, W).contiguous()          # runs of 5 on two levels
    y = ((i // 7) % 3).view(1, H, W).contiguous()
    return dict(d=d, y=y, sizes=(0, 2, 4, 5), both=True)


def _constant():
    H, W = 4 * TH, 4 * TW
    return dict(d=torch.full((1, H, W), -0.0), sizes=(H * W - 1, H * W))


BUILDERS = {
    "random_one_tile": lambda: _random(1, TH - 3, TW - 5),
    "random_ragged": lambda: _random(2, 2 * TH + 3, 2 * TW + 5),
    "serpentine": _serpentine,
    "u_across_tiles": _u_across_tiles,
    "tile_corner": _tile_corner,
    "checkerboard": _checkerboard,
    "threshold": _threshold,
    "batch": _batch,
    "thin_row": lambda: _thin(1, 2 * TW + 7),
    "thin_column": lambda: _thin(2 * TH + 7, 1),
    "one_pixel": lambda: dict(d=torch.full((1, 1, 1), 1.0), sizes=(0, 1)),
    "constant_4x4_tiles": _constant,
}
CASES = tuple(BUILDERS)
RAGGED = "random_ragged"
_MEMO = {}


def case(name):
    """{"d", "y" or None, "where" or None, "lo", "hi", "max_diff", "sizes", "both"} of a case, computed once and shared: leave it unchanged."""
    if name not in _MEMO:
        c = dict(y=None, where=None, lo=LO, hi=HI, max_diff=1.0, both=False)
        c.update(BUILDERS[name]())
        _MEMO[name] = c
    return _MEMO[name]


def variants(c):
    """(same_class, max_size) of a case: every max_size of it, class-aware and -- where the case has a label -- class-agnostic too."""
    return tuple((same, n) for same in ((True, False) if c["both"] else (True,)) for n in c["sizes"])


def arguments(c, variant, with_where=True):
    same_class, max_size = variant
    return dict(label=c["y"], where=c["where"] if with_where else None, max_diff=c["max_diff"], max_size=max_size, same_class=same_class)


def call(sa, c, variant, want=KEYS, move=lambda t: t, **over):
    kw = dict(arguments(c, variant), **over)
    kw = {k: move(v) if isinstance(v, torch.Tensor) else v for k, v in kw.items()}
    return sa.filter_speckles(move(c["d"]), disp_range=(c["lo"], c["hi"]), want=want, **kw)


def expected(c, variant, **over):
    return restate(c["d"], lo=c["lo"], hi=c["hi"], **dict(arguments(c, variant), **over))


def same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        a, b = (got[k].view(torch.int32), want[k].view(torch.int32)) if k == "disparity" else (got[k], want[k])      # bits: -0.0 is not 0.0
        assert torch.equal(a, b), f"{what} {k}: {(a != b).sum().item()} of {b.numel()} values differ"


def closed_forms(out, name):
    """What a case's result must be whatever computed it (`out`: all four keys at any max_size, without `where`)."""
    c = case(name)
    comp, size, valid = out["component"], out["size"], (c["d"] >= c["lo"]) & (c["d"] < c["hi"])
    B, H, W = c["d"].shape
    if name == "serpentine":
        n = int(valid.sum())
        assert n == (H + 1) // 2 * W + H // 2 and bool((size[valid] == n).all()) and bool((comp[valid] == 0).all())
    elif name == "u_across_tiles":
        assert bool((size[valid] == 2 * (TH - 2) + 8).all()) and bool((comp[valid] == 2 * W + 3).all())
    elif name == "tile_corner":
        a, b = TH - 1, TW - 1
        assert size[0, a, b] == 1 and size[0, a + 1, b + 1] == 1 and comp[0, a, b] == a * W + b and comp[0, a + 1, b + 1] == (a + 1) * W + b + 1
        assert size[1, a, b + 1] == 1 and size[1, a + 1, b] == 1 and comp[1, a + 1, b] == (a + 1) * W + b
        assert size[2, a, b] == 3 and size[2, a, b + 1] == 3 and size[2, a + 1, b + 1] == 3 and comp[2, a + 1, b + 1] == a * W + b
        assert int(size.sum()) == 2 + 2 + 9
    elif name == "checkerboard":
        assert bool((size == 1).all()) and torch.equal(comp.view(-1), torch.arange(H * W, dtype=torch.int32))
    elif name == "threshold":
        assert bool((size[0, 0] == W).all()) and bool((comp[0, 0] == 0).all())
        assert size[0, 2, :5].tolist() == [2, 2, 0, 1, 1] and size[0, 2, TW - 1:TW + 1].tolist() == [1, 1]
        assert size[0, 4, TW - 1:TW + 1].tolist() == [2, 2] and comp[0, 4, TW] == 4 * W + TW - 1
    elif name == "batch":
        assert bool((size == H * W).all()) and bool((comp == 0).all())             # per image: component restarts at 0
    elif name == "constant_4x4_tiles":
        assert bool((size == H * W).all()) and bool((comp == 0).all())
    elif name == "one_pixel":
        assert size.tolist() == [[[1]]] and comp.tolist() == [[[0]]]


# ------------------------------------------------------------------------------------------------ SceneStereo(refine=dict(speckle=))
SPECKLE = dict(max_size=64, max_diff=0.25)
BLOB = (slice(40, 45), slice(60, 68))            # 5 x 8 = 40 pixels of the scene
SCENE_ARGS = dict(tile=(64, 64), overlap=(32, 32), batch=2)


def blob_scene(H=96, W=160):
    """A scene pair for refine_cases.per_pixel_model, whose disparity is 1.5 x the difference of the normalised red channels at the
    SAME pixel, in both directions: one colour on the left (one class everywhere), red lower by 10 on the right -- a disparity of
    0.257 all over -- and lower by 30 on the 40 pixels of BLOB: 0.771 there, a blob in the stand-in's disparity.  It is inside the
    range and consistent in both directions (a blob pixel x lands on x - 1, where the right view's map holds 0.771 or 0.257: within
    the threshold 1.0 either way), so the left-right check keeps it, and it is 0.514 > max_diff away from its surroundings."""
    left = torch.empty((H, W, 3), dtype=torch.uint8)
    left[...] = torch.tensor([120, 90, 60], dtype=torch.uint8)
    right = left.clone()
    right[..., 0] = 110
    right[BLOB + (0,)] = 90
    return left, right


def check_scene(sa, fc, left, right, moved):
    """SceneStereo(refine=dict(..., speckle=SPECKLE)) on blob_scene: the blob is the speckle map, is filled from its surroundings, and
    nothing else changes; without the key the refined outputs are those of refine_cases.check_scene and no speckle path is counted.
    `moved(before, key)`: how far a path counter went."""
    plain = sa.SceneStereo(fc.per_pixel_model, **SCENE_ARGS)
    refined = sa.SceneStereo(fc.per_pixel_model, refine=fc.REFINE, **SCENE_ARGS)
    stereo = sa.SceneStereo(fc.per_pixel_model, refine=dict(fc.REFINE, speckle=SPECKLE), **SCENE_ARGS)
    want = ("disparity", "disparity_refined", "kind", "consistent", "label")
    # 2: without the key -- today's outputs, no speckle call
    before = dict(sa.modules.PATH_COUNTS)
    today = fc.check_scene(sa, refined, plain, left, right)
    base = refined(left, right, want=want)
    assert moved(before, "speckle_hip") == 0 and moved(before, "speckle_torch") == 0
    blob = torch.zeros(left.shape[:2], dtype=torch.bool, device=base["kind"].device)
    blob[BLOB] = True
    assert bool(base["consistent"].all()) and bool((base["kind"] == 0).all())                      # the check keeps the blob: it stays
    assert torch.equal(base["disparity_refined"], base["disparity"]) and torch.equal(today["disparity_refined"], base["disparity_refined"])
    assert float(base["disparity"][BLOB].min()) > 0.7 and float(base["disparity"][~blob].max()) < 0.3
    # ... nor with the key when nothing refined is asked for
    before = dict(sa.modules.PATH_COUNTS)
    same = stereo(left, right, want=("disparity", "label", "disparity_right"))
    assert moved(before, "speckle_hip") == 0 and moved(before, "speckle_torch") == 0
    assert torch.equal(same["disparity"], base["disparity"]) and torch.equal(same["label"], base["label"])
    # 1: with it
    before = dict(sa.modules.PATH_COUNTS)
    got = stereo(left, right, want=want + ("speckle",))
    assert moved(before, "speckle_hip") + moved(before, "speckle_torch") == 1
    assert got["speckle"].dtype == torch.bool and torch.equal(got["speckle"], blob)
    assert torch.equal(got["disparity"], base["disparity"]) and torch.equal(got["consistent"], base["consistent"])
    assert bool((got["kind"][BLOB] == 1).all()) and bool((got["kind"][~blob] == 0).all())          # filled from its own class
    rows, cols = BLOB
    sides = torch.stack([got["disparity"][rows, cols.start - 1], got["disparity"][rows, cols.stop]], dim=1)        # [5, 2]
    filled = got["disparity_refined"][BLOB]
    assert bool(((filled == sides[:, :1]) | (filled == sides[:, 1:])).all())                       # its surroundings' value
    assert torch.equal(got["disparity_refined"][~blob], base["disparity"][~blob])
    direct = sa.filter_speckles(got["disparity"], label=got["label"], maxdisp=fc.REFINE["maxdisp"], want=("speckle", "size"), **SPECKLE)
    assert torch.equal(direct["speckle"], got["speckle"]) and bool((direct["size"][BLOB] == 40).all())
    only = stereo(left, right, want=("speckle",))
    assert tuple(only) == ("speckle",) and torch.equal(only["speckle"], blob)
    return got
