"""Sample preparation of the reference's datasets (datasets/us3d_.py:70-215, datasets/whu_dataset.py:42-92) on the device: what
`__getitem__` computes on the host for every item -- 30 ms on one CPU thread, mostly float64 work for gx / gy, and 43.6 MB of float
tensors per 1024 x 1024 item (tools/bench_data.py) -- from the 11 MB of raw arrays behind it, next to the losses that read the results.

  normalize_views    datasets/data_io.py:6-13     ToTensor + Normalize of both views
  nearest_pyramid    us3d_.py:178-182             the five cv2.resize(..., INTER_NEAREST) calls and the float32 label
  image_gradients    us3d_.py:98-109              gx / gy: three convert("L"), a float64 mean and std, two float64 convolve2d
  prepare_sample     us3d_.py:184-215             the sample dictionary with the reference's keys, per branch and per dataset
  right_view         us3d_.py:115-133, :193       the commented-out forward warp: right-view label and disparity, the left view's visibility
  lr_consistency     loss.py:121-135 (the idea)   the left-right check of two estimates, for inference without ground truth
  RawStereoDataset   us3d_.py:38-74               the list files and the decode (PIL only); no arithmetic on the host
  DeviceLoader                                    copies a raw batch from pinned memory on a side stream and prepares it there, one batch ahead

CUDA tensors run csrc/sample_prep.hip: one launch for the views, one for the pyramids, two for the gradients (no atomics: integer
partial sums per workgroup, added by the second), every result staying on the device and nothing waiting on the host.  CPU tensors, non-contiguous or oddly typed inputs, sizes outside the kernels' limits and
SS_DATA_HIP=0 take the PyTorch composition below, written without boolean indexing and without `.item()`.
modules.PATH_COUNTS["data_hip"] / ["data_torch"] count the calls on each path.

The arithmetic, defined once and used by both paths:
  * views: (u / 255 - mean[c]) / std[c] in fp32, in that order, with the constants of data_io.py:7-8.  Only 3 x 256 values exist; the
    768-entry table is built once on the host with exactly those torch operations and indexed by both paths.
  * luma: L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 in integers, PIL's convert("L").
  * statistics, per image: S1 = sum L and S2 = sum L^2 as 64-bit integers, mean = double(S1) / N, std = sqrt(double(N S2 - S1^2)) / N.
    The integer sums are exact in any order, so two calls give the same bits.  N S2 - S1^2 is exact in 64 bits up to H W <= 2^23;
    larger images take the composition, which there forms the variance from the centred squares in float64 (not exact: numpy's own
    form).  numpy's np.std differs from the exact form by at most an ulp of double.
  * gx[y,x] = float32(z(y,x-1) - z(y,x+1)), gy[y,x] = float32(z(y-1,x) - z(y+1,x)) with z = (L - mean) / std in double (a 256-entry
    table per image) and zero outside the image -- convolve2d flips the kernel.  The centre tap 0 * z(y,x) of the convolution is
    kept, so a constant image (std = 0) is NaN on every pixel, borders included, as in the reference.
  * pyramids: cv2.resize(a, (w // k, h // k), INTER_NEAREST) reads source index min(floor(d * ifx), size - 1) with
    ifx = 1.0 / (double(dst) / double(src)) in double, as OpenCV's resizeNN forms it; for H and W divisible by k that is d * k exactly.
    cv2 is not installed where this was written: for sizes that k does not divide, the formula is taken from OpenCV's source and is
    unverified.  The kernel takes H and W divisible by 16; other sizes take the composition.
  * right view (csrc/right_view.hip; rows up to 8192 wide): per row, a left pixel x with a valid disparity (lo <= d < hi) lands on
    right column t = round(float(x) - d), fp32, half to even, if 0 <= t < W; the largest x landing on a column owns it.  Selections
    only, so both paths give the same bits; the kernel's owners are an integer maximum in LDS.  See right_view and lr_consistency.

The right view in use, with m = maxdisp and `sample` from prepare_sample / DeviceLoader(keys=(..., "right_label", "left_visible"), maxdisp=m):
    loss_r = F.cross_entropy(pred_label_r, sample["right_label"].long(), ignore_index=5)       # the right head on its own ground truth
    noc = disparity_metrics(ests, sample["disparity"], maxdisp=m, mask_img=sample["left_visible"])   # "noc"; without mask_img: "all"
    ok = lr_consistency(model(left, right), -model(right, left), threshold=1.0, maxdisp=m)      # without ground truth

Departures from the reference: every entry is a tensor on the inputs' device (the reference returns numpy arrays for `disparity`, the
pyramid levels and `label`, which the collate turns into the same tensors); the statistics are the exact-integer form above.
"""
import os

import numpy as np
import torch

from . import _lib
from . import engine as E
from ._host import LABEL_CODES, _const, _nograd, count
from ._lib import call, ptr

#: datasets/data_io.py:7-8
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DISP_LEVELS, LABEL_LEVELS = (4, 8, 16), (2, 4)
MAX_STAT_PIXELS = 2 ** 23                    # N S2 - S1^2 is exact in 64 bits up to here
_DISP_CODES = {torch.float32: 0, torch.int32: 1}
_MAX_ELEMENTS = 2 ** 31
_TABLE = []

#: the reference's keys per dataset kind and branch (us3d_.py:184-215, whu_dataset.py:68-92)
KEYS = {
    ("us3d", True): ("left", "right", "disparity", "disparity_4", "disparity_8", "disparity_16", "label", "label_2", "label_4", "gx", "gy"),
    ("us3d", False): ("left", "right", "disparity", "label", "top_pad", "right_pad", "left_filename", "gx", "gy"),
    ("whu", True): ("left", "right", "disparity", "disparity_4", "disparity_8", "disparity_16", "gx", "gy"),
    ("whu", False): ("left", "right", "disparity", "top_pad", "right_pad", "left_filename", "gx", "gy"),
}
_PASS_THROUGH = ("top_pad", "right_pad", "left_filename")
#: what right_view adds to a sample when `keys` names it (no name starts with "disparity" or "label": those are pyramid levels)
RIGHT_VIEW_KEYS = ("right_label", "right_disparity", "left_visible")
MAX_RIGHT_VIEW_WIDTH = 8192                  # the owners of a row are 4 W bytes of LDS


def view_table():
    """float32 [3,256] on the host: (u / 255 - mean[c]) / std[c] with the operations of ToTensor (`.div(255)`) and Normalize
    (`.sub_(mean).div_(std)`, mean and std as float32 tensors), in that order."""
    if not _TABLE:
        u = torch.arange(256, dtype=torch.float32).div(255).view(1, 256).expand(3, 256).clone()
        mean = torch.as_tensor(MEAN, dtype=torch.float32).view(3, 1)
        std = torch.as_tensor(STD, dtype=torch.float32).view(3, 1)
        _TABLE.append(u.sub_(mean).div_(std).contiguous())
    return _TABLE[0]


def _hip(*tensors):
    """The kernels take these tensors: the switch is on and all of them are contiguous CUDA tensors on one device."""
    if not E.DATA_HIP:
        return False
    dev = tensors[0].device
    return all(t.is_cuda and t.device == dev and t.is_contiguous() for t in tensors)


def workspace_bytes(B, H, W):
    """Scratch of the luma / gradient pair (asked once per shape)."""
    return _lib.query_bytes("ss_prep_workspace_bytes", B, H, W)


# ------------------------------------------------------------------------------------------------ views
def _views_torch(u8):
    table = _const("view_table", u8.device, view_table)
    idx = u8.permute(0, 3, 1, 2).long()                                        # [B,3,H,W]
    return torch.stack([table[c][idx[:, c]] for c in range(3)], dim=1)


def _is_views(t):
    return isinstance(t, torch.Tensor) and t.dim() == 4 and t.shape[-1] == 3 and t.numel() > 0


@_nograd
def normalize_views(left_u8, right_u8=None):
    """ToTensor + Normalize of the reference's get_transform(): uint8 [B,H,W,3] (or [H,W,3]) -> float32 [B,3,H,W] (or [3,H,W]).  With
    `right_u8` both views are prepared in one launch and a pair is returned."""
    if left_u8.dim() == 3:
        out = normalize_views(left_u8.unsqueeze(0), None if right_u8 is None else right_u8.unsqueeze(0))
        return out[0] if right_u8 is None else (out[0][0], out[1][0])
    views = [left_u8] if right_u8 is None else [left_u8, right_u8]
    assert all(_is_views(v) for v in views) and all(v.shape == left_u8.shape for v in views), "views are [B,H,W,3]"
    B, H, W, _ = left_u8.shape
    if all(v.dtype == torch.uint8 for v in views) and _hip(*views) and left_u8.numel() < _MAX_ELEMENTS:
        count("data_hip")
        table = _const("view_table", left_u8.device, view_table)
        outs = [torch.empty((B, 3, H, W), dtype=torch.float32, device=left_u8.device) for _ in views]
        with torch.cuda.device(left_u8.device):
            call("ss_prep_views_fwd", ptr(left_u8), ptr(right_u8), ptr(table), B, H, W, ptr(outs[0]), ptr(outs[1]) if right_u8 is not None else None)
    else:
        count("data_torch")
        outs = [_views_torch(v if v.dtype == torch.uint8 else v.clamp(0, 255).to(torch.uint8)) for v in views]
    return outs[0] if right_u8 is None else (outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ pyramids
def nearest_index(dst, src, device):
    """Source indices of cv2.resize's INTER_NEAREST for `dst` samples of `src`: min(floor(d * ifx), src - 1), ifx = 1 / (dst / src) in
    double (OpenCV's resizeNN).  Sizes are host integers, so nothing waits."""
    ifx = 1.0 / (float(dst) / float(src))
    d = torch.arange(dst, dtype=torch.float64, device=device)
    return torch.floor(d * ifx).clamp(max=src - 1).long()


def _resize_torch(a, k):
    H, W = a.shape[-2:]
    ys, xs = nearest_index(H // k, H, a.device), nearest_index(W // k, W, a.device)
    return a.index_select(-2, ys).index_select(-1, xs)


def _scaled(disparity, scale):
    d = disparity if disparity.dtype == torch.float32 else disparity.to(torch.float32)
    return d if scale == 1.0 else d * torch.full((), scale, dtype=torch.float32, device=d.device)


@_nograd
def nearest_pyramid(disparity, label=None, disp_levels=DISP_LEVELS, label_levels=LABEL_LEVELS, disp_scale=1.0):
    """The ground-truth pyramids of the training branch (us3d_.py:178-182).  `disparity` [B,H,W] float32, or int32 with `disp_scale`
    (WHU: 1 / 256, exact in fp32); `label` [B,H,W] uint8, int64 or float32 with any strides that keep a row contiguous.  Returns a
    dictionary: "disparity" (float32, the input itself where it already is that), "disparity_<k>" for k in `disp_levels`, and with a
    label "label" (float32, as the dataset returns it) and "label_<k>" for k in `label_levels`; level k is [B, H // k, W // k]."""
    disp_levels, label_levels = tuple(disp_levels), tuple(label_levels)
    squeeze = disparity.dim() == 2
    if squeeze:
        disparity, label = disparity.unsqueeze(0), None if label is None else label.unsqueeze(0)
    assert disparity.dim() == 3 and (label is None or label.shape == disparity.shape), "maps are [B,H,W]"
    B, H, W = disparity.shape
    scale = float(disp_scale)
    plain = disparity.dtype == torch.float32 and scale == 1.0                   # `disparity` passes through
    hip = (H % 16 == 0 and W % 16 == 0 and 0 < disparity.numel() < _MAX_ELEMENTS and set(disp_levels) <= set(DISP_LEVELS)
           and set(label_levels) <= set(LABEL_LEVELS) and disparity.dtype in _DISP_CODES and _hip(disparity)
           and (label is None or (label.is_cuda and label.device == disparity.device and label.dtype in LABEL_CODES))
           and (label is not None or disp_levels or not plain))
    out = {}
    if hip:
        count("data_hip")
        dev = disparity.device
        new = lambda k: torch.empty((B, H // k, W // k), dtype=torch.float32, device=dev)                  # noqa: E731
        out["disparity"] = disparity if plain else new(1)
        for k in disp_levels:
            out[f"disparity_{k}"] = new(k)
        y, code, row, img = None, 0, W, H * W
        if label is not None:
            y = label
            if y.stride(2) != 1 or y.stride(1) < W or (B > 1 and y.stride(0) < (H - 1) * y.stride(1) + W):
                y = y.contiguous()
            code, row = LABEL_CODES[y.dtype], y.stride(1)
            img = max(y.stride(0), (H - 1) * row + W)                            # (the stride of a batch of one is arbitrary)
            out["label"] = new(1)
            for k in label_levels:
                out[f"label_{k}"] = new(k)
        with torch.cuda.device(dev):
            call("ss_prep_pyramid_fwd", ptr(disparity), _DISP_CODES[disparity.dtype], scale, ptr(y), code, row, img, B, H, W,
                 None if plain else ptr(out["disparity"]), ptr(out.get("disparity_4")), ptr(out.get("disparity_8")),
                 ptr(out.get("disparity_16")), ptr(out.get("label")), ptr(out.get("label_2")), ptr(out.get("label_4")))
    else:
        count("data_torch")
        d = _scaled(disparity, scale)
        out["disparity"] = d
        for k in disp_levels:
            out[f"disparity_{k}"] = _resize_torch(d, k)
        if label is not None:
            y = label.to(torch.float32)
            out["label"] = y
            for k in label_levels:
                out[f"label_{k}"] = _resize_torch(y, k)
    return {k: v[0] for k, v in out.items()} if squeeze else out


# ------------------------------------------------------------------------------------------------ gx / gy
def luma(u8):
    """PIL's convert("L") of uint8 [...,3]: int64 [...]."""
    v = u8.long()
    return (19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 0x8000) >> 16


def luma_statistics(L):
    """(mean, std) float64 [B] of int64 luma [B,H,W], from the exact integer sums while N S2 - S1^2 fits 64 bits."""
    B = L.shape[0]
    N = L[0].numel()
    flat = L.reshape(B, -1)
    S1 = flat.sum(1)
    mean = S1.double() / N
    if N <= MAX_STAT_PIXELS:
        S2 = (flat * flat).sum(1)
        std = torch.sqrt((N * S2 - S1 * S1).double()) / N
    else:
        std = torch.sqrt(((flat.double() - mean.view(B, 1)) ** 2).sum(1) / N)
    return mean, std


def _gradients_torch(u8):
    B, H, W, _ = u8.shape
    L = luma(u8)
    mean, std = luma_statistics(L)
    table = (torch.arange(256, dtype=torch.float64, device=u8.device).view(1, 256) - mean.view(B, 1)) / std.view(B, 1)
    z = torch.gather(table, 1, L.reshape(B, -1)).view(B, H, W)
    p = torch.nn.functional.pad(z, (1, 1, 1, 1))
    centre = 0.0 * z
    gx = (p[:, 1:-1, :-2] - p[:, 1:-1, 2:]) + centre
    gy = (p[:, :-2, 1:-1] - p[:, 2:, 1:-1]) + centre
    return gx.to(torch.float32).unsqueeze(1), gy.to(torch.float32).unsqueeze(1)


@_nograd
def image_gradients(left_u8):
    """gx, gy of the dataset (us3d_.py:98-109): uint8 [B,H,W,3] (or [H,W,3]) -> two float32 [B,1,H,W] (or [1,H,W])."""
    if left_u8.dim() == 3:
        gx, gy = image_gradients(left_u8.unsqueeze(0))
        return gx[0], gy[0]
    assert _is_views(left_u8), "the view is [B,H,W,3]"
    B, H, W, _ = left_u8.shape
    if (left_u8.dtype == torch.uint8 and _hip(left_u8) and H * W <= MAX_STAT_PIXELS and B <= 65535 and left_u8.numel() < _MAX_ELEMENTS):
        count("data_hip")
        dev = left_u8.device
        ws = torch.empty(workspace_bytes(B, H, W) // 8, dtype=torch.int64, device=dev)
        gx = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
        gy = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            call("ss_prep_luma_stats_fwd", ptr(left_u8), B, H, W, ptr(ws), ws.numel() * 8)
            call("ss_prep_gradients_fwd", ptr(ws), ws.numel() * 8, B, H, W, ptr(gx), ptr(gy))
        return gx, gy
    count("data_torch")
    return _gradients_torch(left_u8 if left_u8.dtype == torch.uint8 else left_u8.clamp(0, 255).to(torch.uint8))


# ------------------------------------------------------------------------------------------------ the right view
def _disp_range(maxdisp, disp_range):
    """(lo, hi) as the float32 values both paths compare against."""
    assert (maxdisp is None) != (disp_range is None), "give exactly one of maxdisp (the signed range) and disp_range=(lo, hi)"
    lo, hi = (-maxdisp, maxdisp) if disp_range is None else disp_range
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    assert lo < hi, "the disparity range is lo < hi"
    return lo, hi


def _label_for_kernel(label, disparity):
    """(code, row stride, image stride) where the kernels read `label` in place, else None."""
    if not (label.is_cuda and label.device == disparity.device and label.dtype in LABEL_CODES):
        return None
    B, H, W = label.shape
    if label.stride(2) != 1 or label.stride(1) < W or (B > 1 and label.stride(0) < (H - 1) * label.stride(1) + W):
        return None
    return LABEL_CODES[label.dtype], label.stride(1), max(label.stride(0), (H - 1) * label.stride(1) + W)


def _targets(d, lo, hi):
    """(lands bool [B,H,W], target column int64 [B,H,W] with W where the pixel does not land, x int64 [1,1,W])."""
    W = d.shape[-1]
    x = torch.arange(W, device=d.device).view(1, 1, W)
    t = torch.round(x.to(torch.float32) - d)
    lands = (d >= lo) & (d < hi) & (t >= 0) & (t < W)
    return lands, torch.where(lands, t, torch.full_like(t, W)).long(), x


def _right_view_torch(d, label, lo, hi, fill_disparity, fill_label, want):
    B, H, W = d.shape
    lands, t, x = _targets(d, lo, hi)
    owner = torch.full((B, H, W + 1), -1, dtype=torch.int64, device=d.device)       # the last slot collects what does not land
    owner.scatter_reduce_(2, t, x.expand(B, H, W), "amax", include_self=True)
    out = {}
    if "right_disparity" in want or "right_label" in want:
        own = owner[..., :W]
        has, src = own >= 0, own.clamp(min=0)
        if "right_disparity" in want:
            out["right_disparity"] = torch.where(has, d.gather(2, src), torch.full_like(d, fill_disparity))
        if "right_label" in want:
            y = label.to(torch.float32)
            out["right_label"] = torch.where(has, y.gather(2, src), torch.full_like(y, fill_label))
    if "left_visible" in want:
        out["left_visible"] = lands & (owner.gather(2, t) == x)
    return out


@_nograd
def right_view(disparity, label=None, maxdisp=None, disp_range=None, fill_disparity=-999.0, fill_label=5.0,
               want=RIGHT_VIEW_KEYS):
    """The ground truth as the right camera sees it, and what of the left view it sees at all: the forward warp the reference left as
    a commented-out per-pixel loop (us3d_.py:115-133, `"label_r"` at :193).  `disparity` [B,H,W] (or [H,W]) of the left view, float32
    (anything else is converted first), a left pixel x matching right column x - d; `label` [B,H,W] of any dtype.  Exactly one of
    `maxdisp` (valid: -maxdisp <= d < maxdisp, the range masks of main_us3d.py:199) and `disp_range=(lo, hi)` (valid: lo <= d < hi;
    (0, maxdisp) for the unsigned variant).  Row by row:
      * x LANDS on t = round(float(x) - d) (fp32, half to even) if d is valid and 0 <= t < W;
      * the owner of a right column is the LARGEST x that lands on it -- the last writer of a raster-order loop and, the pixel further
        right having the larger disparity up to the rounding step, the surface nearer the sensor;
      * "right_disparity" = d[owner] and "right_label" = float(label[owner]), `fill_disparity` (-999, the dataset's no-data value)
        and `fill_label` (5, the ignored class) where nothing lands; "left_visible" (bool) = x lands and owns its column -- the
        non-occluded mask that disparity_metrics(mask_img=) and joint_metrics(mask=) take.
    Nothing is interpolated, so the kernel (csrc/right_view.hip) and the composition agree bit for bit.  `want` names the entries to
    compute; "right_label" needs a label.  Returns a dictionary of tensors on the input's device; nothing waits on the host."""
    want = tuple(want)
    assert want and set(want) <= set(RIGHT_VIEW_KEYS), f"want names some of {RIGHT_VIEW_KEYS}"
    assert "right_label" not in want or label is not None, "right_label needs a label"
    lo, hi = _disp_range(maxdisp, disp_range)
    squeeze = disparity.dim() == 2
    if squeeze:
        disparity, label = disparity.unsqueeze(0), None if label is None else label.unsqueeze(0)
    assert disparity.dim() == 3 and (label is None or label.shape == disparity.shape), "maps are [B,H,W]"
    if "right_label" not in want:
        label = None
    B, H, W = disparity.shape
    fill_disparity, fill_label = float(np.float32(fill_disparity)), float(np.float32(fill_label))
    how = None if label is None else _label_for_kernel(label, disparity)
    if (disparity.dtype == torch.float32 and _hip(disparity) and W <= MAX_RIGHT_VIEW_WIDTH and 0 < disparity.numel() < _MAX_ELEMENTS
            and (label is None or how is not None)):
        count("data_hip")
        dev = disparity.device
        out = {k: torch.empty((B, H, W), dtype=torch.bool if k == "left_visible" else torch.float32, device=dev) for k in want}
        code, row, img = how if how is not None else (0, W, H * W)
        with torch.cuda.device(dev):
            call("ss_right_view_fwd", ptr(disparity), ptr(label), code, row, img, B, H, W, lo, hi, fill_disparity, fill_label,
                 ptr(out.get("right_disparity")), ptr(out.get("right_label")), ptr(out.get("left_visible")))
    else:
        count("data_torch")
        out = _right_view_torch(disparity.to(torch.float32), label, lo, hi, fill_disparity, fill_label, want)
    out = {k: out[k] for k in want}
    return {k: v[0] for k, v in out.items()} if squeeze else out


@_nograd
def lr_consistency(disp_left, disp_right, threshold=1.0, maxdisp=None, disp_range=None, return_diff=False):
    """The left-right consistency check of two estimates, for inference without ground truth.  `disp_left` [B,H,W] (or [H,W]) in the
    convention of right_view; `disp_right[r]` is the disparity of RIGHT pixel r, its left match at r + disp_right[r] -- the form
    "right_disparity" has, and minus what the model returns for the swapped pair, `-model(right, left)`.  With t(x) as in right_view:
    diff[x] = |disp_left[x] - disp_right[t(x)]| in fp32 where x lands and disp_right[t(x)] is valid, +inf elsewhere; the result is
    the bool map diff <= threshold, or with `return_diff` the pair (that map, diff).  The range as in right_view."""
    lo, hi = _disp_range(maxdisp, disp_range)
    threshold = float(np.float32(threshold))
    assert threshold >= 0, "the threshold is not negative"
    squeeze = disp_left.dim() == 2
    if squeeze:
        disp_left, disp_right = disp_left.unsqueeze(0), disp_right.unsqueeze(0)
    assert disp_left.dim() == 3 and disp_right.shape == disp_left.shape, "maps are [B,H,W]"
    B, H, W = disp_left.shape
    if (disp_left.dtype == torch.float32 and disp_right.dtype == torch.float32 and _hip(disp_left, disp_right)
            and 0 < disp_left.numel() < _MAX_ELEMENTS):
        count("data_hip")
        dev = disp_left.device
        ok = torch.empty((B, H, W), dtype=torch.bool, device=dev)
        diff = torch.empty((B, H, W), dtype=torch.float32, device=dev) if return_diff else None
        with torch.cuda.device(dev):
            call("ss_lr_consistency_fwd", ptr(disp_left), ptr(disp_right), B, H, W, lo, hi, threshold, ptr(ok), ptr(diff))
    else:
        count("data_torch")
        dl, dr = disp_left.to(torch.float32), disp_right.to(torch.float32)
        lands, t, _ = _targets(dl, lo, hi)
        m = dr.gather(2, t.clamp(max=W - 1))
        found = lands & (m >= lo) & (m < hi)
        diff = torch.where(found, (dl - m).abs(), torch.full_like(dl, float("inf")))
        ok = diff <= threshold
    if squeeze:
        ok, diff = ok[0], None if diff is None else diff[0]
    return (ok, diff) if return_diff else ok


# ------------------------------------------------------------------------------------------------ the sample dictionary
@_nograd
def prepare_sample(raw, training, keys=None, disp_scale=None, maxdisp=None, disp_range=None):
    """The dictionary of the reference's `__getitem__` after the collate, from the raw arrays: `raw` holds "left_u8" and "right_u8"
    (uint8 [B,H,W,3]), "disparity" ([B,H,W] float32, or int32 as WHU's 16-bit files decode) and, for US3D, "label" ([B,H,W]); without a
    label the WHU key set is returned.  The training branch has the pyramids, the test branch "top_pad", "right_pad" (0 where `raw` has
    none) and "left_filename" (where `raw` has one), passed through.  `keys` selects a subset, and only what it names is computed: a
    training script reads "left", "right", "disparity", "disparity_4" and "label".  `disp_scale`: None = 1 / 256 for an integer
    disparity (whu_dataset.py:36) and 1 for a floating one.  `keys` may also name RIGHT_VIEW_KEYS -- "right_label" (US3D only),
    "right_disparity", "left_visible": right_view of the float32 `disparity` entry (WHU: the scaled map) and the label, which needs
    `maxdisp` or `disp_range`; they follow the reference's keys and are never part of the default dictionary."""
    kind = "us3d" if raw.get("label") is not None else "whu"
    names = KEYS[(kind, bool(training))]
    want = names if keys is None else tuple(k for k in names if k in set(keys))
    views = ()
    if keys is not None:                                                         # (a name of the other branch is no error: one list serves both)
        unknown = set(keys) - {k for v in KEYS.values() for k in v} - set(RIGHT_VIEW_KEYS)
        assert not unknown, f"not keys of any sample: {sorted(unknown)}"
        views = tuple(k for k in RIGHT_VIEW_KEYS if k in set(keys) and (kind == "us3d" or k != "right_label"))
        assert not views or (maxdisp is None) != (disp_range is None), f"{views} need exactly one of maxdisp and disp_range"
    disparity = raw["disparity"]
    if disp_scale is None:
        disp_scale = 1.0 if disparity.is_floating_point() else 1.0 / 256.0
    out = {}
    if "left" in want and "right" in want:
        out["left"], out["right"] = normalize_views(raw["left_u8"], raw["right_u8"])
    elif "left" in want:
        out["left"] = normalize_views(raw["left_u8"])
    elif "right" in want:
        out["right"] = normalize_views(raw["right_u8"])
    maps = [k for k in want if k.startswith(("disparity", "label"))]
    if maps:
        labels = [k for k in maps if k.startswith("label")]
        pyr = nearest_pyramid(disparity, raw["label"] if labels else None,
                              disp_levels=[int(k.split("_")[1]) for k in maps if k.startswith("disparity_")],
                              label_levels=[int(k.split("_")[1]) for k in labels if "_" in k], disp_scale=disp_scale)
        out.update({k: pyr[k] for k in maps})
    if views:
        d = out["disparity"] if "disparity" in out else _scaled(disparity, float(disp_scale))
        out.update(right_view(d, raw["label"] if "right_label" in views else None, maxdisp=maxdisp, disp_range=disp_range, want=views))
        want = want + views
    if "gx" in want or "gy" in want:
        gx, gy = image_gradients(raw["left_u8"])
        out.update({k: v for k, v in (("gx", gx), ("gy", gy)) if k in want})
    for k in _PASS_THROUGH:
        if k in want:
            if k in raw:
                out[k] = raw[k]
            elif k != "left_filename":
                out[k] = 0
    return {k: out[k] for k in want if k in out}


# ------------------------------------------------------------------------------------------------ the raw dataset and the loader
class RawStereoDataset(torch.utils.data.Dataset):
    """The reference's Us3dDataset / WhuDataset without their arithmetic: the same list files (left, right, disparity and, for US3D,
    label path per line, relative to `datapath`), decoded with PIL, returned as they are -- "left_u8", "right_u8" uint8 [H,W,3],
    "disparity" float32 [H,W] (US3D) or int32 [H,W] (WHU: the 16-bit file's integers; prepare_sample scales them by 1 / 256),
    "label" uint8 [H,W] (US3D), and in the test branch "top_pad", "right_pad" (0) and "left_filename"."""

    def __init__(self, datapath, list_filename, training, kind="us3d"):
        assert kind in ("us3d", "whu")
        self.datapath, self.training, self.kind = datapath, bool(training), kind
        with open(list_filename) as f:
            rows = [line.split() for line in (ln.rstrip() for ln in f.readlines()) if line]
        self.left_filenames = [r[0] for r in rows]
        self.right_filenames = [r[1] for r in rows]
        self.disp_filenames = [r[2] for r in rows]
        self.label_filenames = [r[3] for r in rows] if kind == "us3d" else None

    def __len__(self):
        return len(self.left_filenames)

    def _open(self, name):
        from PIL import Image
        return Image.open(os.path.join(self.datapath, name))

    def _view(self, name):
        return torch.from_numpy(np.array(self._open(name).convert("RGB"), dtype=np.uint8))

    def __getitem__(self, index):
        item = {"left_u8": self._view(self.left_filenames[index]), "right_u8": self._view(self.right_filenames[index])}
        disp = self._open(self.disp_filenames[index])
        item["disparity"] = torch.from_numpy(np.array(disp, dtype=np.float32 if self.kind == "us3d" else np.int32))
        if self.kind == "us3d":
            label = np.array(self._open(self.label_filenames[index]))
            item["label"] = torch.from_numpy(label if label.dtype == np.uint8 else label.astype(np.float32))
        if not self.training:
            item.update(top_pad=0, right_pad=0, left_filename=self.left_filenames[index])
        return item


class DeviceLoader:
    """Iterates `loader` (a DataLoader over a RawStereoDataset, or any iterable of collated raw batches) and yields prepared sample
    dictionaries on `device`.  On a CUDA device the raw batch is copied from pinned memory on a side stream and prepare_sample runs
    there, one batch ahead of the consumer; a batch is handed to the caller's current stream behind an event, with record_stream on
    every tensor handed out, so `sample['left'].cuda()` in the reference's train_sample is a no-op and the function runs as written.
    `training`: None = the dataset's own flag; `keys`, `disp_scale`, `maxdisp` and `disp_range` are prepare_sample's.  `augment`: an
    augment.Augmentation -- the training branch then draws a batch's parameters on the host and runs augment.augment_sample in place of
    prepare_sample (crops, so `keys` may not name gx, gy or RIGHT_VIEW_KEYS; without a range of its own the loader hands the swap the
    Augmentation's maxdisp); the test branch is never augmented."""

    def __init__(self, loader, device=None, keys=None, training=None, disp_scale=None, maxdisp=None, disp_range=None, augment=None):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.loader, self.device, self.keys, self.disp_scale = loader, torch.device(device), keys, disp_scale
        self.range = {"maxdisp": maxdisp, "disp_range": disp_range}             # for the RIGHT_VIEW_KEYS that `keys` names
        if training is None:
            training = getattr(getattr(loader, "dataset", None), "training", True)
        self.training = bool(training)
        self.augment = augment if self.training else None
        if self.augment is not None and maxdisp is None and disp_range is None:
            self.range["maxdisp"] = getattr(augment, "maxdisp", None)
        self._stream = None
        if self.device.type == "cuda":
            _const("view_table", self.device, view_table)                        # (on the caller's stream, before the side stream exists)

    def __len__(self):
        return len(self.loader)

    def _upload(self, v):
        if not isinstance(v, torch.Tensor) or v.dim() < 3:                       # pads and file names stay where they are
            return v
        if not v.is_cuda and not v.is_pinned():
            v = v.pin_memory()
        return v.to(self.device, non_blocking=True)

    def _sample(self, raw):
        if self.augment is None:
            return prepare_sample(raw, self.training, self.keys, self.disp_scale, **self.range)
        from .augment import augment_sample
        B, H, W, _ = raw["left_u8"].shape
        return augment_sample(raw, self.augment.draw(B, H, W), self.keys, self.disp_scale, **self.range)

    def _prepare(self, raw):
        if self.device.type != "cuda":
            return self._sample(raw), None
        if self._stream is None:
            self._stream = torch.cuda.Stream(self.device)
            self._stream.wait_stream(torch.cuda.current_stream(self.device))    # (once: the table's upload is on the caller's stream)
        with torch.cuda.stream(self._stream):
            sample = self._sample({k: self._upload(v) for k, v in raw.items()})
            done = torch.cuda.Event()
            done.record(self._stream)
        return sample, done

    def _hand_over(self, sample, done):
        if done is not None:
            current = torch.cuda.current_stream(self.device)
            current.wait_event(done)
            for v in sample.values():
                if isinstance(v, torch.Tensor) and v.is_cuda:
                    v.record_stream(current)
        return sample

    def __iter__(self):
        ahead = None
        for raw in self.loader:
            nxt = self._prepare(raw)
            if ahead is not None:
                yield self._hand_over(*ahead)
            ahead = nxt
        if ahead is not None:
            yield self._hand_over(*ahead)
