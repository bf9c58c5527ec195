"""Scene inference: a rectified pair of any size in, a disparity mosaic and a label mosaic out.  The reference's scripts assume that the
input is one US3D tile that fits the network (its evaluation loader carries `top_pad` / `right_pad` keys that are always 0); a scene
several thousand pixels on a side, of a size that is no multiple of 32, is cut into overlapping windows, every window goes through
the model as it is after `install` + `accelerate`, and the finished tiles are feathered into the mosaic.

  TilePlan       the windows, the feather weights and the bands of a scene: host integers only
  tile_views     the windows of a scene pair cut and normalised (ToTensor + Normalize) in one pass: csrc/scene_tiles.hip
  blend_tiles    finished tiles gathered into rows of the mosaic: disparity, logits, label, spread, count
  SceneStereo    the loop around the model: tiles ride a PairPipeline's lanes, a band is blended as soon as its tile rows are done

CUDA tensors run the two kernels of csrc/scene_tiles.hip.  CPU tensors, other dtypes or layouts, sizes outside the kernels' limits and
SS_SCENE_HIP=0 take the PyTorch composition below, written without boolean indexing and without `.item()`.
modules.PATH_COUNTS["scene_hip"] / ["scene_torch"] count the calls on each path.

The definitions, used by both paths:
  * windows, per axis with scene extent S: T = min(tile, round_up(S, 32)).  S <= T: one window at 0, overhanging the scene at the
    bottom / right.  Otherwise s = T - overlap, n = ceil((S - T) / s) + 1 and origin[k] = min(k s, S - T): the last window is shifted
    back into the scene, not padded.  With 0 <= overlap <= T // 2 a pixel lies in at most 3 windows per axis.
  * views: out[c][y][x] = table[c][scene[oy + y][ox + x][c]] with data.view_table() inside the scene and 0.0 off it: the mean colour
    in normalised space, what padding after Normalize gives.
  * weights: integers.  Per axis w(i) = min(i + 1, T - i, R) for window-local index i and ramp R (default max(overlap, 1)); a tile
    pixel weighs float(wy) * float(wx) >= 1, so no pixel has zero total weight.  R = 1 is plain stitching (an average where tiles overlap).
  * blend, per mosaic pixel over the covering resident tiles in ascending (ty, tx): num = num + w * v and den = den + w, every
    product and every sum rounded to fp32, then ONE division num / den.  Under ONE tile the value is the tile's own, v, not
    (w * v) / w, which rounds twice: where nothing overlaps, the mosaic is the model's output bit for bit.  The same per logit
    channel.  The order is fixed and nothing is atomic: two calls give the same bits whatever lanes produced the tiles, and the
    kernel gives the composition's bits.
  * label: the lowest index of the largest blended logit (np.argmax's rule); spread: max - min of the covering tiles' disparities, 0
    under one tile -- the seam diagnostic to threshold; count: the number of covering tiles.
  * bands: tile row r finishes mosaic rows [origin_y[r], origin_y[r + 1]) (the last band ends at H): those rows are covered only by
    tile rows <= r, and by at most 3 of them.
"""
import torch
import torch.nn as nn

from . import data as D
from . import engine as E
from . import refine as R
from ._host import _const, _nograd, argmax_first, count
from ._lib import call, ptr

OUTPUTS = ("disparity", "logits", "label", "spread", "count")
#: what SceneStereo(refine=...) adds: the right view's mosaic (minus the swapped pair's), the check and the filled mosaic
REFINED_OUTPUTS = ("disparity_right", "consistent", "disparity_refined", "kind", "disparity_median", "speckle")
_REFINE_ARGS = ("maxdisp", "disp_range", "threshold", "max_gap", "prefer", "fallback", "fill_value", "axes", "median", "speckle")
#: refine=dict(..., speckle=dict(...)): filter_speckles' arguments
_SPECKLE_ARGS = ("max_size", "max_diff", "same_class")
#: refine=dict(..., median=dict(...)): median_disparity's arguments, and which pixels may change ("filled": kind != 0; "all")
_MEDIAN_ARGS = ("radius", "iterations", "where", "same_class", "fill_holes", "min_count")
_DTYPES = {"label": torch.uint8, "count": torch.uint8}
MAX_CHANNELS = 8                             # csrc/scene_tiles.hip: logit channels
MAX_WINDOWS = 256                            # ... and windows per axis
_MAX_ELEMENTS = 2 ** 31


def _pair(v):
    return (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))


def _axis_origins(S, T, overlap):
    if S <= T:
        return (0,)
    s = T - overlap
    n = -(-(S - T) // s) + 1
    return tuple(min(k * s, S - T) for k in range(n))


def feather_weights(T, R):
    """w(i) = min(i + 1, T - i, R) for i in 0 .. T - 1: a list of integers >= 1."""
    return [min(i + 1, T - i, R) for i in range(T)]


class TilePlan:
    """The windows of an `height` x `width` scene (see the module's definitions): `tile`, `overlap` and `ramp` are (y, x) pairs or one
    integer for both axes.  `tile` is a multiple of 32, 0 <= overlap <= T // 2 for the effective tile size T; anything else is a
    ValueError.  Host integers only:
      size                  (th, tw), the effective tile size
      origin_y, origin_x    the window origins per axis, strictly increasing; tile (ty, tx) has number ty * ntx + tx
      origins               the (y, x) of every tile in that order
      ramp                  (ry, rx)
      bands                 per tile row r: (y0, y1, rows) -- tile row r finishes mosaic rows [y0, y1), which need the tile rows `rows`
      last_use              per tile row: the last band that needs it"""

    def __init__(self, height, width, tile=(1024, 1024), overlap=(256, 256), ramp=None):
        self.height, self.width = int(height), int(width)
        if self.height < 1 or self.width < 1:
            raise ValueError(f"a scene has at least one pixel, got {height} x {width}")
        tile, overlap = _pair(tile), _pair(overlap)
        size = []
        for S, t, o, axis in zip((self.height, self.width), tile, overlap, "yx"):
            if t < 32 or t % 32:
                raise ValueError(f"tile_{axis} = {t} is not a positive multiple of 32")
            T = min(t, -(-S // 32) * 32)
            if not 0 <= o <= T // 2:
                raise ValueError(f"overlap_{axis} = {o} is outside [0, {T // 2}] for the effective tile size {T}")
            size.append(T)
        self.size, self.overlap = tuple(size), overlap
        self.ramp = tuple(max(o, 1) for o in overlap) if ramp is None else _pair(ramp)
        if min(self.ramp) < 1:
            raise ValueError(f"ramp = {self.ramp} is below 1")
        self.origin_y = _axis_origins(self.height, size[0], overlap[0])
        self.origin_x = _axis_origins(self.width, size[1], overlap[1])
        self.nty, self.ntx = len(self.origin_y), len(self.origin_x)
        self.origins = tuple((y, x) for y in self.origin_y for x in self.origin_x)
        th = size[0]
        self.bands = []
        for r, y0 in enumerate(self.origin_y):
            y1 = self.origin_y[r + 1] if r + 1 < self.nty else self.height
            self.bands.append((y0, y1, tuple(k for k in range(r + 1) if self.origin_y[k] + th > y0)))
        self.last_use = tuple(max(r for r, (_, _, rows) in enumerate(self.bands) if k in rows) for k in range(self.nty))

    def __len__(self):
        return self.nty * self.ntx

    def row_origins(self, r):
        """The (y, x) origins of tile row r."""
        return self.origins[r * self.ntx:(r + 1) * self.ntx]


def _hip(*tensors):
    """The kernels take these tensors: the switch is on and all of them are contiguous CUDA tensors on one device."""
    if not E.SCENE_HIP:
        return False
    dev = tensors[0].device
    return all(t.is_cuda and t.device == dev and t.is_contiguous() for t in tensors)


def _upload(values, dtype, device):
    """A small host table on `device` without a host wait: through pinned memory (the caching host allocator keeps the buffer until
    the copy has run)."""
    t = torch.tensor(values, dtype=dtype)
    return t.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else t


# ------------------------------------------------------------------------------------------------ windows
def _tile_views_torch(u8, origins, size):
    th, tw = size
    H, W, _ = u8.shape
    out = torch.zeros((len(origins), 3, th, tw), dtype=torch.float32, device=u8.device)
    for i, (oy, ox) in enumerate(origins):
        y0, y1, x0, x1 = max(oy, 0), min(oy + th, H), max(ox, 0), min(ox + tw, W)
        if y0 < y1 and x0 < x1:
            out[i, :, y0 - oy:y1 - oy, x0 - ox:x1 - ox] = D._views_torch(u8[y0:y1, x0:x1].unsqueeze(0))[0]
    return out


@_nograd
def tile_views(left_u8, right_u8, origins, size):
    """The windows of a scene (pair), cut and normalised in one pass: uint8 [H,W,3] -> float32 [n,3,th,tw] per view, ready for the
    model.  `origins`: n (y, x) pairs of host integers, anywhere (TilePlan.origins, or one tile row of them); `size` = (th, tw).
    Inside the scene a value is ToTensor + Normalize of the pixel (data.normalize_views' table), off the scene it is 0.0.  With
    `right_u8` None one tensor is returned, else the pair."""
    origins = tuple((int(y), int(x)) for y, x in origins)
    th, tw = int(size[0]), int(size[1])
    views = [left_u8] if right_u8 is None else [left_u8, right_u8]
    assert all(isinstance(v, torch.Tensor) and v.dim() == 3 and v.shape[-1] == 3 and v.numel() > 0 for v in views), "a scene is [H,W,3]"
    assert all(v.shape == left_u8.shape for v in views) and origins and th > 0 and tw > 0
    H, W, _ = left_u8.shape
    n = len(origins)
    if (all(v.dtype == torch.uint8 for v in views) and _hip(*views) and left_u8.numel() < _MAX_ELEMENTS
            and n * 3 * th * tw < _MAX_ELEMENTS and all(abs(v) < 2 ** 30 for o in origins for v in o)):
        count("scene_hip")
        dev = left_u8.device
        table = _const("view_table", dev, D.view_table)
        org = _const(("scene_origins", origins), dev, lambda: _upload(origins, torch.int32, dev))
        outs = [torch.empty((n, 3, th, tw), dtype=torch.float32, device=dev) for _ in views]
        with torch.cuda.device(dev):
            call("ss_tile_views_fwd", ptr(left_u8), ptr(right_u8), ptr(org), ptr(table), n, th, tw, H, W, ptr(outs[0]),
                 ptr(outs[1]) if right_u8 is not None else None)
    else:
        count("scene_torch")
        outs = [_tile_views_torch(v if v.dtype == torch.uint8 else v.clamp(0, 255).to(torch.uint8), origins, (th, tw)) for v in views]
    return outs[0] if right_u8 is None else (outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ the mosaic
def _as_tiles(tiles, n, what):
    """A list of n entries (a tensor or None) from a list or a batch tensor."""
    if tiles is None:
        return None
    tiles = list(tiles.unbind(0)) if isinstance(tiles, torch.Tensor) else list(tiles)
    assert len(tiles) == n, f"{what}: {len(tiles)} tiles for a plan of {n}"
    return tiles


def _blend_torch(plan, disp, logit, y0, y1, want, dtype, device, C):
    """Rows [y0, y1) of every output in `want`, [y1 - y0, W] each ([C, y1 - y0, W] for the logits): the definition, tile by tile in
    ascending (ty, tx) on slices."""
    (th, tw), (ry, rx), H, W = plan.size, plan.ramp, plan.height, plan.width
    wy = torch.tensor(feather_weights(th, ry), dtype=dtype, device=device)
    wx = torch.tensor(feather_weights(tw, rx), dtype=dtype, device=device)
    rows = y1 - y0
    num, den = torch.zeros((rows, W), dtype=dtype, device=device), torch.zeros((rows, W), dtype=dtype, device=device)
    hi, lo = torch.full_like(num, float("-inf")), torch.full_like(num, float("inf"))
    cnt = torch.zeros((rows, W), dtype=torch.int32, device=device)
    with_logits = C > 0 and ("logits" in want or "label" in want)
    numl = torch.zeros((C, rows, W), dtype=dtype, device=device) if with_logits else None
    one, onel = torch.zeros_like(num), None if numl is None else torch.zeros_like(numl)       # the value under ONE tile: the last writer
    for ty, oy in enumerate(plan.origin_y):
        a, b = max(oy, y0), min(oy + th, y1, H)
        if a >= b:
            continue
        for tx, ox in enumerate(plan.origin_x):
            v = disp[ty * plan.ntx + tx]
            c1 = min(ox + tw, W)
            if v is None or ox >= c1:
                continue
            m = (slice(a - y0, b - y0), slice(ox, c1))                          # of the band
            t = (slice(a - oy, b - oy), slice(0, c1 - ox))                      # of the tile
            w = wy[t[0]].unsqueeze(1) * wx[t[1]].unsqueeze(0)
            v = v[t].to(dtype)
            num[m] += w * v
            den[m] += w
            hi[m] = torch.maximum(hi[m], v)
            lo[m] = torch.minimum(lo[m], v)
            cnt[m] += 1
            one[m] = v
            if with_logits:
                z = logit[ty * plan.ntx + tx][(slice(None),) + t].to(dtype)
                numl[(slice(None),) + m] += w.unsqueeze(0) * z
                onel[(slice(None),) + m] = z
    out = {}
    if "disparity" in want:
        out["disparity"] = torch.where(cnt == 1, one, num / den)
    if "spread" in want:
        out["spread"] = hi - lo
    if "count" in want:
        out["count"] = cnt.to(torch.uint8)
    if with_logits:
        blended = torch.where((cnt == 1).unsqueeze(0), onel, numl / den.unsqueeze(0))
        if "logits" in want:
            out["logits"] = blended
        if "label" in want:
            out["label"] = argmax_first(blended.unsqueeze(0))[0].to(torch.uint8)
    return out


@_nograd
def blend_tiles(plan, disp_tiles, logit_tiles=None, rows=None, out=None, want=("disparity", "label", "spread")):
    """Finished tiles gathered into the mosaic of `plan` (the module's definitions: weights, order, label, spread, count).
    `disp_tiles`: the disparity [th,tw] of every tile in the plan's order -- a list whose entries may be None (not resident: the tile
    is skipped), or one tensor [n,th,tw]; `logit_tiles` the same with [C,th,tw] entries, resident wherever the disparity is.  The
    tensors are read where they are: views of the model's batched outputs need no copy.  `rows` = (y0, y1): only those mosaic rows are
    written (default: all), from the resident tiles; `out`: a dictionary of mosaics from an earlier call to write into (what is
    missing is allocated, zero outside the rows).  `want` names some of OUTPUTS; "logits" and "label" need logit_tiles.  Returns the
    dictionary: "disparity", "spread" [H,W] and "logits" [C,H,W] in the tiles' dtype, "label" and "count" uint8 [H,W]."""
    want = tuple(want)
    assert want and set(want) <= set(OUTPUTS), f"want names some of {OUTPUTS}"
    n, (th, tw), H, W = len(plan), plan.size, plan.height, plan.width
    disp, logit = _as_tiles(disp_tiles, n, "disp_tiles"), _as_tiles(logit_tiles, n, "logit_tiles")
    assert logit is not None or not {"logits", "label"} & set(want), "logits and label need logit_tiles"
    y0, y1 = (0, H) if rows is None else (int(rows[0]), int(rows[1]))
    assert 0 <= y0 <= y1 <= H, "rows = (y0, y1) within the scene"
    resident = [i for i, v in enumerate(disp) if v is not None]
    assert resident, "no tile is resident"
    first = disp[resident[0]]
    dtype, dev = first.dtype, first.device
    assert all(disp[i].shape == (th, tw) for i in resident), f"a disparity tile is [{th},{tw}]"
    C = 0
    if logit is not None:
        C = logit[resident[0]].shape[0]
        assert all(logit[i] is not None and logit[i].shape == (C, th, tw) for i in resident), f"a logit tile is [C,{th},{tw}]"
    out = {} if out is None else out
    shapes = {k: (C, H, W) if k == "logits" else (H, W) for k in want}
    for k in want:
        if k not in out:
            make = torch.empty if (y0, y1) == (0, H) else torch.zeros
            out[k] = make(shapes[k], dtype=_DTYPES.get(k, dtype), device=dev)
        assert out[k].shape == shapes[k] and out[k].device == dev and out[k].dtype == _DTYPES.get(k, dtype), f"out[{k!r}]"
    used = [disp[i] for i in resident] + ([logit[i] for i in resident] if logit is not None else [])
    if (dtype == torch.float32 and all(t.dtype == dtype for t in used) and _hip(*used, *(out[k] for k in want)) and C <= MAX_CHANNELS
            and plan.nty <= MAX_WINDOWS and plan.ntx <= MAX_WINDOWS and max(C, 1) * max(H * W, th * tw) < _MAX_ELEMENTS):
        count("scene_hip")
        org = _const(("scene_axes", plan.origin_y, plan.origin_x), dev,
                     lambda: _upload(plan.origin_y + plan.origin_x, torch.int32, dev))
        tables = [[0 if t is None else t.data_ptr() for t in disp]]
        if logit is not None:
            tables.append([0 if disp[i] is None else logit[i].data_ptr() for i in range(n)])
        tab = _upload(tables, torch.int64, dev)
        with torch.cuda.device(dev):
            call("ss_tile_blend_fwd", ptr(tab[0]), ptr(tab[1]) if logit is not None else None, ptr(org), ptr(org[plan.nty:]),
                 plan.nty, plan.ntx, th, tw, C, plan.ramp[0], plan.ramp[1], H, W, y0, y1,
                 *(ptr(out[k]) if k in want else None for k in OUTPUTS))
    else:
        count("scene_torch")
        if y0 < y1:
            band = _blend_torch(plan, disp, logit, y0, y1, want, dtype, dev, C)
            for k in want:
                out[k][..., y0:y1, :] = band[k]
    return out


# ------------------------------------------------------------------------------------------------ the loop around the model
class SceneStereo:
    """`SceneStereo(model, tile=, overlap=, ramp=, lanes=6, batch=1, refine=None)(left_u8, right_u8, want=("disparity", "label", "spread"))`: the
    model on a scene pair of any size.  Scenes are uint8 [H,W,3] on the device or on the host (a host scene is copied once, to the
    model's device).  `model` is any callable with the reference's eval convention -- `([disp [B,h,w]], logits [B,C,h,w])`, or
    `[disp]` alone without a segmentation head -- taking the two normalised views [B,3,th,tw].  An nn.Module in eval mode on the
    device goes through a PairPipeline of `lanes` lanes, `batch` tiles of one tile row per call; every other callable is called
    directly.  Returns a dictionary of tensors on the device, named by `want` (see blend_tiles); nothing waits on the host.

    Tile row r + 1 is issued before band r is blended, so the lanes never drain between tile rows; the outputs of a tile row are
    joined onto the calling stream (`pipe.join`) before the first band that reads them and are dropped after the last one
    (TilePlan.last_use).  `peak_resident_tile_rows` is the largest number of tile rows held at once in the last call: at most 3.

    What the overlap is for: a pixel within `maxdisp` columns of a window's vertical edge may have its match outside the window, and
    the network's answer there is a guess.  The feather gives such a pixel a weight near 1 against up to `ramp` for the neighbour
    that sees it well inside, so overlap_x of about 2 * maxdisp with the default ramp (= the overlap) is the sensible setting; the
    default (256, 256) suits maxdisp = 128.  `spread` shows where the tiles still disagree.

    The left-right check per scene: with `refine=dict(maxdisp=, threshold=, max_gap=, prefer=, fallback=, axes=)` (refine_disparity's
    arguments; `axes="both"` fills along rows and columns) `want` may also name "disparity_right", "consistent", "disparity_refined" and "kind".  If it does, every tile row is also
    issued with the views swapped -- the same windows, `model(right_tile, left_tile)` -- and those disparities are blended into a second
    mosaic band by band alongside the first.  The blend of negated tiles is the exact negation of the blend (products, sums and the
    division are sign-symmetric), so that mosaic is negated once, in place, after the last band: "disparity_right", the form
    lr_consistency takes.  One refine_disparity call over the two mosaics and the label mosaic gives the rest; without logits the
    fill is class-agnostic (tier 2 only).  The swapped tile rows live exactly as long as the others: at most 3 per direction.

    The median after the fill: with `refine=dict(..., median=dict(radius=2, iterations=1, where="filled", fill_holes=True, ...))`
    (median_disparity's arguments) `want` may also name "disparity_median": one median_disparity call over "disparity_refined" and
    the label mosaic, with the refine arguments' range, follows the refine_disparity call.  where="filled" (the default) lets only
    the pixels the fill touched or left unfilled change (`kind != 0`), so the model's kept values stay bit for bit; where="all"
    gives no mask.  A call that does not name "disparity_median" makes no further launch.

    Speckles before the fill: with `refine=dict(..., speckle=dict(max_size=, max_diff=, same_class=))` (filter_speckles' arguments)
    one filter_speckles call over the left mosaic and the label mosaic, with the refine arguments' range, comes before the
    refine_disparity call, which gets `keep=~speckle`: a small blob that passes the left-right check is then no source, its pixels
    have `kind != 0` and take their surroundings' value.  `want` may also name "speckle", the bool map.  Without the `speckle` key no
    such call is made and every output keeps its bits.

    Not here: a column pass proper for rows without any source (fill_holes reaches radius x iterations rows), reading GeoTIFFs."""

    def __init__(self, model, tile=(1024, 1024), overlap=(256, 256), ramp=None, lanes=6, batch=1, refine=None):
        assert callable(model) and int(lanes) >= 1 and int(batch) >= 1
        if refine is not None:
            refine = dict(refine)
            if not set(refine) <= set(_REFINE_ARGS):
                raise ValueError(f"refine names some of {_REFINE_ARGS}, got {tuple(refine)}")
            median = refine.pop("median", None)
            if median is not None:
                median = dict(median)
                if not set(median) <= set(_MEDIAN_ARGS) or median.setdefault("where", "filled") not in ("filled", "all"):
                    raise ValueError(f'median names some of {_MEDIAN_ARGS} with where "filled" or "all", got {median}')
            speckle = refine.pop("speckle", None)
            if speckle is not None:
                speckle = dict(speckle)
                if not set(speckle) <= set(_SPECKLE_ARGS):
                    raise ValueError(f"speckle names some of {_SPECKLE_ARGS}, got {tuple(speckle)}")
        self.refine, self.median = refine, (median if refine is not None else None)
        self.speckle = speckle if refine is not None else None
        self.model, self.tile, self.overlap, self.ramp = model, tile, overlap, ramp
        self.lanes, self.batch = int(lanes), int(batch)
        self.pipe, self.plan, self.peak_resident_tile_rows = None, None, 0

    def _device(self, left):
        if left.is_cuda:
            return left.device
        if isinstance(self.model, nn.Module):
            p = next(self.model.parameters(), None)
            if p is not None:
                return p.device
        return left.device

    def _pipelined(self, dev):
        if not (dev.type == "cuda" and isinstance(self.model, nn.Module)):
            return False
        assert not self.model.training, "SceneStereo is inference: put the model in eval mode"
        if self.pipe is None:
            from .segment import PairPipeline
            self.pipe = PairPipeline(self.model, lanes=self.lanes)
        return True

    @staticmethod
    def _outputs(result):
        """(disp [B,h,w], logits [B,C,h,w] or None) of the reference's eval convention."""
        if isinstance(result, tuple) and len(result) == 2 and isinstance(result[0], (list, tuple)):
            return result[0][0], result[1]
        return result[0], None

    def _issue(self, r, left, right, piped, both=False):
        """Tile row r through the model: a list of (disp, logits, event) per call, in tile order; with `both` the pair (that list, the
        same for the swapped views of the same windows)."""
        views = tile_views(left, right, self.plan.row_origins(r), self.plan.size)
        calls = self._run(views[0], views[1], piped)
        return (calls, self._run(views[1], views[0], piped)) if both else calls

    def _run(self, first, second, piped):
        plan = self.plan
        calls = []
        for b in range(0, plan.ntx, self.batch):
            l, rt = first[b:b + self.batch], second[b:b + self.batch]
            if piped:
                disp, logits = self._outputs(self.pipe(l, rt))
                event = self.pipe.last_event
            else:
                with torch.no_grad():
                    disp, logits = self._outputs(self.model(l, rt))
                event = None
            assert disp.shape == (l.shape[0],) + plan.size, f"the model returns disparities {tuple(disp.shape)} for tiles {plan.size}"
            calls.append((disp, logits, event))
        return calls

    def _join(self, calls):
        """The outputs of one tile row on the calling stream: the disparity and logit tiles in tile order."""
        disp, logit = [], []
        for d, lg, event in calls:
            if event is not None:
                self.pipe.join((d, lg), event=event)
            d = d if d.dtype == torch.float32 else d.float()
            disp += [t if t.is_contiguous() else t.contiguous() for t in d.unbind(0)]
            if lg is not None:
                lg = lg if lg.dtype == torch.float32 else lg.float()
                logit += [t if t.is_contiguous() else t.contiguous() for t in lg.unbind(0)]
        return disp, (logit if logit else None)

    def __call__(self, left_u8, right_u8, want=("disparity", "label", "spread")):
        want = tuple(want)
        extra = tuple(k for k in want if k in REFINED_OUTPUTS)
        if extra:
            return self._refined(left_u8, right_u8, want, extra)
        return self._mosaic(left_u8, right_u8, want)

    def _refined(self, left_u8, right_u8, want, extra):
        """The mosaics of both directions, then one refine_disparity call."""
        assert self.refine is not None, f"{extra} need SceneStereo(refine=dict(maxdisp=..., ...))"
        base = tuple(k for k in want if k in OUTPUTS)
        assert len(base) + len(extra) == len(want), f"want names some of {OUTPUTS + REFINED_OUTPUTS}"
        out, swapped = self._mosaic(left_u8, right_u8, base + tuple(k for k in ("disparity", "label") if k not in base), both=True)
        names = {"disparity_refined": "disparity", "kind": "kind", "consistent": "consistent"}
        asked = tuple(names[k] for k in extra if k in names)
        median = None
        if "disparity_median" in extra:
            assert self.median is not None, "disparity_median needs SceneStereo(refine=dict(..., median=dict(...)))"
            median = dict(self.median)
            masked = median.pop("where") == "filled"
            asked += tuple(k for k in (("disparity", "kind") if masked else ("disparity",)) if k not in asked)
        valid = {k: self.refine[k] for k in ("maxdisp", "disp_range") if k in self.refine}
        keep = None
        if "speckle" in extra or (self.speckle is not None and {"disparity", "kind"} & set(asked)):       # (the check itself knows no keep)
            assert self.speckle is not None, "speckle needs SceneStereo(refine=dict(..., speckle=dict(...)))"
            out["speckle"] = R.filter_speckles(out["disparity"], label=out.get("label"), want=("speckle",), **valid, **self.speckle)["speckle"]
            keep = ~out["speckle"]
        if asked:
            got = R.refine_disparity(out["disparity"], swapped, label=out.get("label"), keep=keep, want=asked, **self.refine)
            out.update({k: got[names[k]] for k in extra if k in names})
        if median is not None:
            out["disparity_median"] = R.median_disparity(got["disparity"], label=out.get("label"), where=(got["kind"] != 0) if masked else None,
                                                         **valid, **median)["disparity"]
        out["disparity_right"] = swapped
        assert all(k in out for k in want), "the model returned no logits: no label mosaic"
        return {k: out[k] for k in want}

    def _mosaic(self, left_u8, right_u8, want, both=False):
        """The mosaics named by `want`; with `both` the pair (those, the right view's disparity mosaic from the swapped tiles) and a
        "label" the model has no logits for is left out, not an error."""
        assert left_u8.dim() == 3 and left_u8.shape[-1] == 3 and right_u8.shape == left_u8.shape, "scenes are uint8 [H,W,3]"
        dev = self._device(left_u8)
        left, right = (v if v.device == dev else v.to(dev, non_blocking=True) for v in (left_u8, right_u8))
        H, W, _ = left.shape
        plan = self.plan = TilePlan(H, W, self.tile, self.overlap, self.ramp)
        piped = self._pipelined(dev)
        n, ntx = len(plan), plan.ntx
        disp, logit = [None] * n, [None] * n
        held, out, self.peak_resident_tile_rows = {}, {}, 0
        back, disp_back, out_back = {}, [None] * n, {}                          # the swapped direction: the same lifetimes
        for r in range(plan.nty + 1):
            if r < plan.nty:
                if both:
                    held[r], back[r] = self._issue(r, left, right, piped, both=True)
                else:
                    held[r] = self._issue(r, left, right, piped)               # (one tile row ahead of the band that is blended)
                self.peak_resident_tile_rows = max(self.peak_resident_tile_rows, len(held))
            if r == 0:
                continue
            band = r - 1
            y0, y1, rows = plan.bands[band]
            if disp[band * ntx] is None:
                d, lg = self._join(held[band])
                disp[band * ntx:(band + 1) * ntx] = d
                if lg is not None:
                    logit[band * ntx:(band + 1) * ntx] = lg
                if both:
                    disp_back[band * ntx:(band + 1) * ntx] = self._join(back[band])[0]
            has_logits = logit[band * ntx] is not None
            if both and not has_logits:
                want = tuple(k for k in want if k != "label")
            assert has_logits or not {"logits", "label"} & set(want), "the model returned no logits: ask for disparity, spread, count"
            if not out:                                                         # (every row is written by its band)
                C = logit[0].shape[0] if has_logits else 0
                out = {k: torch.empty((C, H, W) if k == "logits" else (H, W), dtype=_DTYPES.get(k, torch.float32), device=dev) for k in want}
            blend_tiles(plan, disp, logit if has_logits else None, rows=(y0, y1), out=out, want=want)
            if both:
                if not out_back:
                    out_back = {"disparity": torch.empty((H, W), dtype=torch.float32, device=dev)}
                blend_tiles(plan, disp_back, None, rows=(y0, y1), out=out_back, want=("disparity",))
            for k in [k for k in held if plan.last_use[k] <= band]:             # no later band reads these tile rows
                del held[k]
                disp[k * ntx:(k + 1) * ntx] = [None] * ntx
                logit[k * ntx:(k + 1) * ntx] = [None] * ntx
                if both:
                    del back[k]
                    disp_back[k * ntx:(k + 1) * ntx] = [None] * ntx
        out = {k: out[k] for k in want}
        return (out, out_back["disparity"].neg_()) if both else out

    def close(self):
        if self.pipe is not None:
            self.pipe.close()
            self.pipe = None
