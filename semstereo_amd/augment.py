"""Training augmentation on the device: the reference's KITTI recipe (datasets/kitti_dataset_15_aug.py:100-156; the SceneFlow file
datasets/sceneflow_dataset_augmentation.py:52-113 is the same recipe with a doubled contrast call, its slip) from the raw arrays that
DeviceLoader uploads, plus the two flips a rectified satellite pair allows.

  AugmentParams      the draws of a batch as CPU tensors: crop origin, flips, occluder, four factors per (item, output view)
  Augmentation       the ranges and probabilities; .draw(B, H, W) -> AugmentParams from a CPU torch.Generator; .us3d(crop, maxdisp)
  augment_sample     prepare_sample's training dictionary at crop size, augmented
  DeviceLoader(..., augment=Augmentation(...))   data.py: draws on the host per batch, augments on the side stream

CUDA tensors run csrc/augment.hip: at most three launches (luma sums, occluder sums when an item has one, the write), plus right_view's
launch when an item swaps, nothing waiting on the host; the parameters go up as one small byte buffer from pinned memory.  CPU tensors,
other dtypes or layouts and SS_AUGMENT_HIP=0 take the PyTorch composition below, written without boolean indexing and without `.item()`.
modules.PATH_COUNTS["augment_hip"] / ["augment_torch"] count the calls on each path.  With the swap an int32 (WHU) disparity is scaled to
float32 by two PyTorch elementwise calls first, because right_view reads float32.

The arithmetic, defined once (include/semstereo_hip.h, "training augmentation") and used by both paths.  Every photometric step works
on uint8 values, each stage rounded as PIL rounds it; u is a channel value of the source view that feeds OUTPUT view v of an item and
(b, g, c, s) are that output view's factors:
  * luma(r, g, b) = (19595 r + 38470 g + 7471 b + 0x8000) >> 16 (data.luma); blend(deg, x, f) = trunc(clamp(float(deg) + float32(f) *
    float(x - deg), 0, 255)) in fp32, the product rounded before the sum: Image.blend as ImageEnhance calls it.
  * brightness u1 = blend(0, u, b); gamma u2 = G[u1], G[e] = int((255 + 1 - 1e-3) * pow(e / 255.0, g)) in Python doubles
    (torchvision's adjust_gamma on a PIL image, gain 1).  Both are one 256-entry uint8 table T1 per (item, output view), built on the host.
  * contrast u3 = blend(m, u2, c), m = int(S / N + 0.5) in double, S the exact integer sum of luma(T1[r], T1[g], T1[b]) over the WHOLE
    source image (before the crop, as in the reference), N = H W.
  * saturation u4[ch] = blend(luma(u3), u3[ch], s), per pixel.
  * geometry: output pixel (y, x) of the th x tw crop at origin (y0, x0) reads source row y0 + (vflip ? th - 1 - y : y) and column
    x0 + x.  With the swap the whole IMAGE is mirrored and the views are exchanged, then the window is applied: the new left is the old
    right mirrored, the new right the old left mirrored, source column W - 1 - (x0 + x); factors belong to the OUTPUT view.
  * the swapped maps: right_view gives, for right pixel r, rd[r] = d[owner(r)], the owner's left column being r + rd[r] up to the
    rounding of its landing.  Mirroring puts old-right pixel r at new-left column x' = W - 1 - r and old-left column r + rd[r] at
    new-right column W - 1 - (r + rd[r]) = x' - rd[r].  So the new disparity d'[x'] = rd[W - 1 - x'] keeps the convention: a new left
    pixel x' with a valid d' matches the new right at x' - d'.  The label goes the same way.  right_view runs on full rows before the
    crop (an owner may lie outside the window) with its default fills -999.0 / 5.0: holes fall out of the loss's range mask and into
    the ignored class.
  * occluder, output right view of a flagged item: crop pixels inside [cy - sy, cy + sy) x [cx - sx, cx + sx) (crop coordinates, rows
    first, clipped to the crop) take floor(Sc / (th tw)) per channel, Sc the exact integer sum of u4 over the crop of that view.  The
    reference truncates numpy's two-stage float64 mean, which can differ only where the exact mean is an integer up to double rounding.
  * left / right = data.view_table()[ch][u4]; disparity and label are the selected pixels (an integer disparity scaled by disp_scale as
    prepare_sample does, the label float32); disparity_4/8/16 and label_2/4 are nearest_pyramid of the AUGMENTED full-resolution map.
Everything is a table lookup, a selection or an exact integer sum, plus one non-contracted fp32 blend: both paths give the same bits.
"""
import itertools
import math

import numpy as np
import torch

from . import _lib
from . import data as D
from . import engine as E
from ._host import _const, _nograd, count
from ._lib import call, ptr

#: what augment_sample can return: the training keys of prepare_sample without gx / gy
AUGMENT_KEYS = tuple(k for k in D.KEYS[("us3d", True)] if k not in ("gx", "gy"))
RECORD_BYTES = 560                           # include/semstereo_hip.h: the parameter record of one item
MAX_ITEMS = 65535
_MAX_ELEMENTS = 2 ** 31
_RECORD = np.dtype([("y0", "<i4"), ("x0", "<i4"), ("flags", "<i4"), ("cy", "<i4"), ("sy", "<i4"), ("cx", "<i4"), ("sx", "<i4"),
                    ("reserved", "<i4"), ("contrast", "<f4", (2,)), ("saturation", "<f4", (2,)), ("t1", "u1", (2, 256))])
assert _RECORD.itemsize == RECORD_BYTES
_UNIT = [e / 255.0 for e in range(256)]


def _i64(v, shape):
    t = torch.as_tensor(v).to(torch.int64).reshape(shape)
    assert not t.is_cuda, "parameters are CPU tensors"
    return t.clone()


def gamma_table(g):
    """G of torchvision's adjust_gamma on a PIL image, gain 1: 256 Python ints."""
    return [int((255 + 1 - 1e-3) * pow(e / 255.0, g)) for e in range(256)]


class AugmentParams:
    """The draws of one batch, CPU tensors: `origin` int64 [B,2] as (y0, x0); `vflip`, `swap` bool [B]; `occluder` int64 [B,4] as
    (cy, sy, cx, sx) in crop coordinates, rows first, a row of -1 (or None for the batch) = none; `brightness`, `gamma`, `contrast`,
    `saturation` float64 [B,2] per OUTPUT view (0 left, 1 right; None = 1).  `crop` = (th, tw) and `image` = (H, W) are what the window
    is checked against: it lies inside the image; the factors are finite and >= 0."""

    def __init__(self, crop, image, origin, vflip=None, swap=None, occluder=None, brightness=None, gamma=None, contrast=None,
                 saturation=None):
        self.crop, self.image = (int(crop[0]), int(crop[1])), (int(image[0]), int(image[1]))
        (th, tw), (H, W) = self.crop, self.image
        assert 0 < th <= H and 0 < tw <= W, f"the crop {self.crop} lies inside the image {self.image}"
        self.origin = _i64(origin, (-1, 2))
        B = self.B = self.origin.shape[0]
        assert B > 0, "at least one item"
        self.vflip = torch.zeros(B, dtype=torch.bool) if vflip is None else _i64(vflip, (B,)) != 0
        self.swap = torch.zeros(B, dtype=torch.bool) if swap is None else _i64(swap, (B,)) != 0
        self.occluder = torch.full((B, 4), -1, dtype=torch.int64) if occluder is None else _i64(occluder, (B, 4))
        for name, v in (("brightness", brightness), ("gamma", gamma), ("contrast", contrast), ("saturation", saturation)):
            t = torch.ones(B, 2, dtype=torch.float64) if v is None else torch.as_tensor(v, dtype=torch.float64).reshape(B, 2).clone()
            assert bool(torch.isfinite(t).all()) and bool((t >= 0).all()), f"{name} is finite and >= 0"
            setattr(self, name, t)
        y0, x0 = self.origin[:, 0], self.origin[:, 1]
        assert bool(((y0 >= 0) & (y0 <= H - th) & (x0 >= 0) & (x0 <= W - tw)).all()), "the window lies inside the image"
        assert int(self.occluder.abs().max()) < 2 ** 30, "occluder coordinates are pixels"

    @property
    def has_occluder(self):
        """bool [B]: the item paints a rectangle (both half-sizes positive)."""
        return (self.occluder[:, 1] > 0) & (self.occluder[:, 3] > 0)

    def rectangle(self):
        """int64 [B,4]: (r0, r1, c0, c1), the half-open rectangle clipped to the crop; empty without an occluder."""
        th, tw = self.crop
        cy, sy, cx, sx = self.occluder.unbind(1)
        r = torch.stack([(cy - sy).clamp(0, th), (cy + sy).clamp(0, th), (cx - sx).clamp(0, tw), (cx + sx).clamp(0, tw)], 1)
        return torch.where(self.has_occluder.view(-1, 1), r, torch.zeros_like(r))

    def t1_tables(self):
        """uint8 numpy [B,2,256]: brightness then gamma of every channel value, T1[u] = G[blend(0, u, b)].  The powers are Python's own
        (math.pow of doubles, one call per entry); the products and truncations around them are IEEE operations numpy shares."""
        u1 = np.clip(self.brightness.numpy().astype(np.float32)[..., None] * np.arange(256, dtype=np.float32), 0, 255).astype(np.int64)
        powers = np.array([list(map(math.pow, _UNIT, itertools.repeat(g))) for g in self.gamma.reshape(-1).tolist()])
        G = ((255 + 1 - 1e-3) * powers).astype(np.int64).reshape(self.B, 2, 256)
        return np.take_along_axis(G, u1, 2).astype(np.uint8)

    def pack(self):
        """The parameter block of the kernels: uint8 [B * 560], the records of include/semstereo_hip.h."""
        rec = np.zeros(self.B, dtype=_RECORD)
        origin, occluder = self.origin.numpy(), self.occluder.numpy()
        rec["y0"], rec["x0"] = origin[:, 0], origin[:, 1]
        rec["flags"] = self.vflip.numpy() + 2 * self.swap.numpy() + 4 * ((occluder[:, 1] > 0) & (occluder[:, 3] > 0))
        rec["cy"], rec["sy"], rec["cx"], rec["sx"] = occluder.T
        rec["contrast"], rec["saturation"] = self.contrast.numpy(), self.saturation.numpy()      # (rounded to float32 by the assignment)
        rec["t1"] = self.t1_tables()
        return torch.from_numpy(rec.view(np.uint8).reshape(-1).copy())


class Augmentation:
    """The recipe: ranges of the four factors (drawn per item and view), the crop, the occluder's probability and half-size ranges, and
    the probabilities of the two flips.  The defaults are the reference's KITTI recipe; `seed` seeds the CPU generator every draw
    comes from (None: a fresh seed)."""

    def __init__(self, crop=(256, 512), brightness=(0.5, 2.0), gamma=(0.8, 1.2), contrast=(0.8, 1.2), saturation=(0.0, 1.4),
                 p_occluder=0.2, occluder_rows=(35, 100), occluder_cols=(25, 75), p_vflip=0.0, p_swap=0.0, seed=None, maxdisp=None):
        self.crop = (int(crop[0]), int(crop[1]))
        self.ranges = {"brightness": brightness, "gamma": gamma, "contrast": contrast, "saturation": saturation}
        for name, (lo, hi) in self.ranges.items():
            assert 0 <= lo <= hi, f"{name}: 0 <= lo <= hi"
        self.p_occluder, self.p_vflip, self.p_swap = float(p_occluder), float(p_vflip), float(p_swap)
        self.occluder_rows, self.occluder_cols = tuple(occluder_rows), tuple(occluder_cols)
        self.maxdisp = maxdisp               # what DeviceLoader hands right_view when it is given no range of its own
        self.generator = torch.Generator()
        if seed is None:
            self.generator.seed()
        else:
            self.generator.manual_seed(int(seed))

    @classmethod
    def us3d(cls, crop, maxdisp, **kwargs):
        """The preset for rectified satellite pairs: the KITTI recipe with both flips at 0.5; `maxdisp` is the signed range the swap's
        right_view takes."""
        kwargs.setdefault("p_vflip", 0.5)
        kwargs.setdefault("p_swap", 0.5)
        return cls(crop=crop, maxdisp=maxdisp, **kwargs)

    def _uniform(self, lo, hi, *shape):
        return lo + (hi - lo) * torch.rand(*shape, dtype=torch.float64, generator=self.generator)

    def draw(self, B, H, W):
        """AugmentParams of a batch of B items of H x W pixels.  The crop shrinks to the image as the reference's RandomCrop does; the
        occluder's half-size is int(U(lo, hi)) and its centre int(U(half, dim - half)), as the reference draws them."""
        th, tw = min(self.crop[0], H), min(self.crop[1], W)
        factors = {name: self._uniform(lo, hi, B, 2) for name, (lo, hi) in self.ranges.items()}
        y0 = torch.randint(0, H - th + 1, (B,), generator=self.generator)
        x0 = torch.randint(0, W - tw + 1, (B,), generator=self.generator)
        vflip = torch.rand(B, dtype=torch.float64, generator=self.generator) < self.p_vflip
        swap = torch.rand(B, dtype=torch.float64, generator=self.generator) < self.p_swap
        flag = torch.rand(B, dtype=torch.float64, generator=self.generator) < self.p_occluder
        occluder = None
        if self.p_occluder > 0:
            (rlo, rhi), (clo, chi) = self.occluder_rows, self.occluder_cols
            assert th > 2 * (rhi - 1) and tw > 2 * (chi - 1), "the crop is larger than the largest occluder"
            sy, sx = self._uniform(rlo, rhi, B).long(), self._uniform(clo, chi, B).long()
            uy, ux = torch.rand(B, dtype=torch.float64, generator=self.generator), torch.rand(B, dtype=torch.float64, generator=self.generator)
            cy, cx = (sy + (th - 2 * sy) * uy).long(), (sx + (tw - 2 * sx) * ux).long()
            occluder = torch.where(flag.view(B, 1), torch.stack([cy, sy, cx, sx], 1), torch.full((B, 4), -1, dtype=torch.int64))
        return AugmentParams((th, tw), (H, W), torch.stack([y0, x0], 1), vflip, swap, occluder, **factors)


# ------------------------------------------------------------------------------------------------ the composition
def _up(t, device):
    """A small host tensor on `device` without a host wait (scene._upload's way)."""
    return t.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else t


def _blend(deg, x, f):
    """blend of int64 tensors with a float32 factor tensor: the product is a tensor of its own, so it is rounded before the sum."""
    t = deg.to(torch.float32) + f * (x - deg).to(torch.float32)
    return t.clamp(0, 255).long()


def _source_index(P, device):
    """(rows int64 [B,th], cols int64 [B,tw]): the source row / column of every output row / column."""
    (th, tw), (_, W) = P.crop, P.image
    y, x = torch.arange(th).view(1, th), torch.arange(tw).view(1, tw)
    y0, x0 = P.origin[:, :1], P.origin[:, 1:]
    rows = y0 + torch.where(P.vflip.view(-1, 1), th - 1 - y, y)
    cols = torch.where(P.swap.view(-1, 1), W - 1 - (x0 + x), x0 + x)
    return _up(rows, device), _up(cols, device)


def _views_torch(left, right, P, want):
    dev = left.device
    B, H, W, _ = left.shape
    th, tw = P.crop
    bi = torch.arange(B, device=dev)
    src = _up(torch.stack([P.swap.long(), 1 - P.swap.long()], 1), dev)          # the source view of output view v
    imgs = torch.stack([left, right], 1)[bi.view(B, 1), src]                     # [B,2,H,W,3]
    t1 = _up(torch.from_numpy(P.t1_tables()).long(), dev)                        # [B,2,256]
    c32, s32 = _up(P.contrast.to(torch.float32), dev), _up(P.saturation.to(torch.float32), dev)
    u2 = torch.gather(t1, 2, imgs.reshape(B, 2, -1).long()).view(B, 2, H, W, 3)
    S = D.luma(u2).reshape(B, 2, -1).sum(2)
    m = (S.double() / float(H * W) + 0.5).long()
    t13 = _blend(m.view(B, 2, 1).expand(B, 2, 256), t1, c32.view(B, 2, 1))
    rows, cols = _source_index(P, dev)
    crop = imgs[bi.view(B, 1, 1, 1), torch.arange(2, device=dev).view(1, 2, 1, 1), rows.view(B, 1, th, 1), cols.view(B, 1, 1, tw)]
    u3 = torch.gather(t13, 2, crop.reshape(B, 2, -1).long()).view(B, 2, th, tw, 3)
    u4 = _blend(D.luma(u3).unsqueeze(-1).expand_as(u3), u3, s32.view(B, 2, 1, 1, 1))
    out_left, out_right = u4[:, 0], u4[:, 1]
    if bool(P.has_occluder.any()):                                               # (host tensors: nothing waits)
        colour = out_right.reshape(B, -1, 3).sum(1) // (th * tw)
        r = _up(P.rectangle(), dev)
        y, x = torch.arange(th, device=dev).view(1, th, 1), torch.arange(tw, device=dev).view(1, 1, tw)
        inside = (y >= r[:, 0].view(B, 1, 1)) & (y < r[:, 1].view(B, 1, 1)) & (x >= r[:, 2].view(B, 1, 1)) & (x < r[:, 3].view(B, 1, 1))
        out_right = torch.where(inside.unsqueeze(-1), colour.view(B, 1, 1, 3).expand(B, th, tw, 3), out_right)
    table = _const("view_table", dev, D.view_table)
    out = {}
    for k, u in (("left", out_left), ("right", out_right)):
        if k in want:
            out[k] = torch.stack([table[ch][u[..., ch]] for ch in range(3)], dim=1)
    return out


def _maps_torch(disparity, label, warped, P, maps, scale):
    dev = disparity.device
    B = disparity.shape[0]
    rows, cols = _source_index(P, dev)
    bi = torch.arange(B, device=dev).view(B, 1, 1)
    swap = _up(P.swap.clone(), dev).view(B, 1, 1) if warped else None
    d = D._scaled(disparity, scale)
    if warped:
        d = torch.where(swap, warped["right_disparity"], d)
    d = d[bi, rows.unsqueeze(2), cols.unsqueeze(1)]
    y = None
    if label is not None:
        y = label.to(torch.float32)
        if warped:
            y = torch.where(swap, warped["right_label"], y)
        y = y[bi, rows.unsqueeze(2), cols.unsqueeze(1)]
    pyr = D.nearest_pyramid(d, y, disp_levels=[int(k.split("_")[1]) for k in maps if k.startswith("disparity_")],
                            label_levels=[int(k.split("_")[1]) for k in maps if k.startswith("label_")])
    return {k: pyr[k] for k in maps}


# ------------------------------------------------------------------------------------------------ the entry point
def workspace_bytes(B, H, W, th, tw):
    """Scratch of the three passes (asked once per shape)."""
    return _lib.query_bytes("ss_augment_scratch_bytes", B, H, W, th, tw)


def _hip(views, disparity, label, maps, P):
    """(label code, row stride, image stride) or () where the kernels take these tensors, else None."""
    if not E.AUGMENT_HIP:
        return None
    left = views[0]
    dev = left.device
    if not all(t.is_cuda and t.device == dev and t.is_contiguous() and t.dtype == torch.uint8 for t in views):
        return None
    B, H, W, _ = left.shape
    th, tw = P.crop
    if left.numel() >= _MAX_ELEMENTS or B > MAX_ITEMS:
        return None
    if any("_" in k for k in maps) and (th % 16 or tw % 16):
        return None
    how = ()
    if maps:
        if not (disparity.is_cuda and disparity.device == dev and disparity.is_contiguous() and disparity.dtype in D._DISP_CODES):
            return None
        if bool(P.swap.any()) and W > D.MAX_RIGHT_VIEW_WIDTH:
            return None
        if label is not None:
            how = D._label_for_kernel(label, disparity)
    return how


@_nograd
def augment_sample(raw, params, keys=None, disp_scale=None, maxdisp=None, disp_range=None):
    """The training-branch dictionary of prepare_sample at crop size, augmented as `params` (an AugmentParams) says; the module
    docstring is the definition.  `raw` is prepare_sample's `raw` dictionary and is never modified; without a label (WHU) the swap
    delivers right_disparity only.  `keys` names some of AUGMENT_KEYS (None: all of them that the sample has) and only what it names is
    computed; "gx", "gy" and RIGHT_VIEW_KEYS of an augmented sample are out of scope and an AssertionError.  `disp_scale` as in
    prepare_sample.  When any item swaps and a map is asked for, exactly one of `maxdisp` / `disp_range` is needed: right_view's range.
    Returns tensors on the inputs' device; nothing waits on the host."""
    P = params
    assert isinstance(P, AugmentParams), "params is an AugmentParams"
    left, right, disparity, label = raw["left_u8"], raw["right_u8"], raw["disparity"], raw.get("label")
    assert D._is_views(left) and right.shape == left.shape, "views are [B,H,W,3]"
    B, H, W, _ = left.shape
    assert P.B == B and P.image == (H, W), f"the parameters are for {P.B} items of {P.image}, the batch has {B} of {(H, W)}"
    assert disparity.shape == (B, H, W) and (label is None or label.shape == (B, H, W)), "maps are [B,H,W]"
    names = tuple(k for k in D.KEYS[("us3d" if label is not None else "whu", True)] if k in AUGMENT_KEYS)
    if keys is not None:
        refused = set(keys) & ({"gx", "gy"} | set(D.RIGHT_VIEW_KEYS))
        assert not refused, f"{sorted(refused)} of an augmented sample are not computed"
        unknown = set(keys) - {k for v in D.KEYS.values() for k in v}
        assert not unknown, f"not keys of any sample: {sorted(unknown)}"
    want = names if keys is None else tuple(k for k in names if k in set(keys))
    maps = [k for k in want if k.startswith(("disparity", "label"))]
    need_label = any(k.startswith("label") for k in maps)
    swaps = bool(P.swap.any()) and bool(maps)
    if swaps:
        assert (maxdisp is None) != (disp_range is None), "a swapped item needs exactly one of maxdisp and disp_range"
    if disp_scale is None:
        disp_scale = 1.0 if disparity.is_floating_point() else 1.0 / 256.0
    scale = float(disp_scale)
    th, tw = P.crop
    dev = left.device

    def warp():
        d = D._scaled(disparity, scale)
        return D.right_view(d, label if need_label else None, maxdisp=maxdisp, disp_range=disp_range,
                            want=("right_disparity",) + (("right_label",) if need_label else ()))
    how = _hip((left, right), disparity, label if need_label else None, maps, P) if want else None
    if how is None:
        count("augment_torch")
        u8 = [v if v.dtype == torch.uint8 else v.clamp(0, 255).to(torch.uint8) for v in (left, right)]
        out = _views_torch(u8[0], u8[1], P, want) if "left" in want or "right" in want else {}
        if maps:
            out.update(_maps_torch(disparity, label if need_label else None, warp() if swaps else None, P, maps, scale))
        return {k: out[k] for k in want}
    count("augment_hip")
    warped = warp() if swaps else {}
    code, row, img = how if how else (0, W, H * W)
    block = P.pack().pin_memory().to(dev, non_blocking=True)
    ws = torch.empty(workspace_bytes(B, H, W, th, tw) // 8, dtype=torch.int64, device=dev)
    table = _const("view_table", dev, D.view_table)
    shape = {k: (B, th // int(k.split("_")[1]), tw // int(k.split("_")[1])) if "_" in k else (B, th, tw) for k in maps}
    shape.update(left=(B, 3, th, tw), right=(B, 3, th, tw))
    out = {k: torch.empty(shape[k], dtype=torch.float32, device=dev) for k in want}
    views = "left" in want or "right" in want
    occluder = views and "right" in want and bool(P.has_occluder.any())
    size = (B, H, W, th, tw, ptr(ws), ws.numel() * 8)
    with torch.cuda.device(dev):
        if views:
            call("ss_augment_stats_fwd", ptr(left), ptr(right), ptr(block), *size)
        if occluder:
            call("ss_augment_occluder_fwd", ptr(left), ptr(right), ptr(block), *size)
        call("ss_augment_write_fwd", ptr(left), ptr(right), ptr(block), ptr(table), ptr(disparity) if maps else None,
             D._DISP_CODES.get(disparity.dtype, 0), scale, ptr(label) if need_label else None, code, row, img,
             ptr(warped.get("right_disparity")), ptr(warped.get("right_label")), *size, int(occluder),
             *(ptr(out.get(k)) for k in ("left", "right", "disparity", "disparity_4", "disparity_8", "disparity_16", "label", "label_2",
                                         "label_4")))
    return out
