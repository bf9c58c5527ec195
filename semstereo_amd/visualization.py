"""The evaluation step's image outputs of the reference (main_us3d.py:252, :265-268; main_whu.py:242, :250-251) under its own names.

  gen_error_colormap / error_colormap   utils/visualization.py:11-27   the ten-row table {lo, hi, r, g, b}, float64 arithmetic cast to float32
  disp_error_image_func                 utils/visualization.py:30-55   the D1-style error map, `.apply(est, gt)` as the scripts call it
  feature_vis                           utils/mask_vis.py:5-31         argmax of the logits in the six-colour palette
  label_vis                             main_us3d.py:266               the same picture straight from a label map: no one-hot tensor
  normalize_image                       utils/experiment.py:98         make_grid(normalize=True, scale_each=True) of save_images
  eval_images                           main_us3d.py:252, :266-268     the image_outputs dictionary of test_sample, device tensors

CUDA fp32 inputs run csrc/vis.hip: one streaming launch per picture (three for a normalisation), every result staying on the device.
Everything else (CPU tensors, float64, more than six channels, SS_VIS_HIP=0) takes the PyTorch composition below, written without
boolean indexing and without `.cpu()`, so it does not wait on the host either.  modules.PATH_COUNTS["vis_hip"] / ["vis_torch"] count
the pictures made on each path.

Departures from the reference, on both paths:
  * `feature_vis` returns a torch tensor on the input's device (float32, or `dtype=torch.uint8`), not a float64 numpy array on the
    host; the values are the same 0 / 255.  `tensor2numpy` and `save_images` of utils/experiment.py accept it.
  * a label outside [0, 6), and a predicted class above 5 of logits with more than six channels, is black; the reference raises (one_hot
    a RuntimeError, the palette lookup an IndexError).
  * `disp_error_image_func` returns its float32 picture on the inputs' device, not on the host.  `legend=False` leaves the colour key
    out; `signed=True` is the honest variant for US3D's signed disparities -- valid where lo <= gt < hi and gt != 0 with
    (lo, hi) = `valid_range`, the relative error over |gt| as in metrics.D1_metric.  The default reproduces the reference, where every
    negative ground truth is black.
  * `normalize_image` is (clamp(x, lo, hi) - lo) / max(hi - lo, 1e-5) in fp32 throughout.  make_grid forms `hi - lo` in double before
    it divides; the divisor differs by at most one ulp.
"""
import numpy as np
import torch

from . import _lib
from . import engine as E
from ._host import LABEL_CODES, _c, _const, _label_classes, _nograd, argmax_first, count
from ._lib import call, ptr

NCLS = 6                                   # classes of the palette and channels the kernel takes
NAMES = ("disp_error_image_func", "feature_vis")        # what install_visualization rebinds
_OUT_CODES = {torch.float32: 0, torch.uint8: 1}
_MAX_QUADS = 2 ** 31 - 1
#: utils/mask_vis.py:10-15
PALETTE = ((0, 0, 0), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255))


def gen_error_colormap():
    """utils/visualization.py:11-24: rows {lo, hi, r, g, b}; the bounds are float64 quotients cast to float32, the colours float32
    quotients by 255."""
    edges = [0.0, 0.1875, 0.375, 0.75, 1.5, 3.0, 6.0, 12.0, 24.0, 48.0]
    rgb = [(49, 54, 149), (69, 117, 180), (116, 173, 209), (171, 217, 233), (224, 243, 248), (254, 224, 144), (253, 174, 97),
           (244, 109, 67), (215, 48, 39), (165, 0, 38)]
    rows = [[edges[i] / 3.0, edges[i + 1] / 3.0 if i + 1 < len(edges) else np.inf, *rgb[i]] for i in range(len(rgb))]
    cols = np.array(rows, dtype=np.float32)
    cols[:, 2:5] /= 255.
    return cols


error_colormap = gen_error_colormap()


def workspace_bytes():
    """Scratch of ss_image_minmax_fwd."""
    return _lib.query_bytes("ss_vis_workspace_bytes", 0)


def _fits(B, H, W):
    return 0 < B * H * ((W + 3) // 4) < _MAX_QUADS


# ------------------------------------------------------------------------------------------------ error map
# the table both paths read: the one of this module, fixed at import (the kernel gets it by value, the composition uploads it once)
_TABLE = np.ascontiguousarray(error_colormap, dtype=np.float32).copy()
assert _TABLE.shape == (10, 5) and all(_TABLE[i + 1, 0] == _TABLE[i, 1] for i in range(9))


def _error_image_torch(est, gt, abs_thres, rel_thres, legend, signed, lo, hi):
    """The composition.  The bins of the table are half-open and adjoining (lo of a row is hi of the one before, asserted above), so
    the row of a pixel is the number of lower bounds it reaches, less one."""
    cols = _TABLE
    dev, dt = gt.device, gt.dtype
    B, H, W = gt.shape
    scalar = lambda v: torch.full((), v, dtype=dt, device=dev)                  # noqa: E731  (a device divisor: a true division per element)
    if signed:
        valid, den = (gt >= lo) & (gt < hi) & (gt != 0), gt.abs()
    else:
        valid, den = gt > 0, gt
    err = (gt - est).abs()
    e = torch.minimum(err / scalar(abs_thres), (err / den) / scalar(rel_thres))                     # NaN in either gives NaN
    bounds = _const(("err_lo", dt), dev, lambda: torch.from_numpy(cols[:, 0].copy()).to(dt))
    colours = _const("err_rgb", dev, lambda: torch.from_numpy(cols[:, 2:5].copy()))
    row = (e.unsqueeze(-1) >= bounds).sum(-1) - 1                                                  # -1: below the table or NaN
    ok = valid & (row >= 0) & (e < float(cols[9, 1]))
    img = colours[row.clamp(min=0)]                                                                # [B,H,W,3]
    img = torch.where(ok.unsqueeze(-1), img, torch.zeros((), dtype=torch.float32, device=dev)).permute(0, 3, 1, 2).contiguous()
    if legend:
        hh, ww = min(10, H), min(200, W)
        key = colours[torch.arange(ww, device=dev) // 20]                                          # [ww, 3]
        img[:, :, :hh, :ww] = key.t().reshape(1, 3, 1, ww)
    return img


def supported_error_image(est, gt):
    """CUDA fp32 [B,H,W] estimate and ground truth of one shape on one device, fewer than 2^31 four-pixel groups."""
    return (isinstance(est, torch.Tensor) and isinstance(gt, torch.Tensor) and gt.is_cuda and gt.dtype == torch.float32 and gt.dim() == 3
            and est.dtype == torch.float32 and est.device == gt.device and est.shape == gt.shape and _fits(*gt.shape))


@_nograd
def disp_error_image(D_est_tensor, D_gt_tensor, abs_thres=3., rel_thres=0.05, dilate_radius=1, legend=True, signed=False,
                     valid_range=(-float("inf"), float("inf"))):
    """utils/visualization.py:30-55: float32 [B,3,H,W] on the inputs' device.  e = min(|gt - est| / abs_thres, (|gt - est| / gt) /
    rel_thres); a pixel takes the colour of the table row with lo <= e < hi; black where gt <= 0 and where no row matches (NaN or
    +inf); the colour key in the top-left corner, clipped to the picture.  `dilate_radius` is accepted and unused, as in the reference."""
    est, gt = D_est_tensor, D_gt_tensor
    assert gt.dim() == 3 and est.shape == gt.shape
    lo, hi = float(valid_range[0]), float(valid_range[1])
    if E.VIS_HIP and supported_error_image(est, gt):
        count("vis_hip")
        est, gt = _c(est), _c(gt)
        B, H, W = gt.shape
        out = torch.empty((B, 3, H, W), dtype=torch.float32, device=gt.device)
        with torch.cuda.device(gt.device):
            call("ss_disp_error_image_fwd", ptr(est), ptr(gt), _TABLE.ctypes.data, B, H, W, float(abs_thres), float(rel_thres), int(bool(legend)),
                 int(bool(signed)), lo, hi, ptr(out))
        return out
    count("vis_torch")
    if est.dtype != gt.dtype:
        est = est.to(gt.dtype)
    return _error_image_torch(est, gt, float(abs_thres), float(rel_thres), legend, signed, lo, hi)


class disp_error_image_func(object):
    """The reference's name and call form: `disp_error_image_func.apply(est, gt)` (main_us3d.py:268), with the keywords of its forward."""

    apply = staticmethod(disp_error_image)

    def forward(self, D_est_tensor, D_gt_tensor, abs_thres=3., rel_thres=0.05, dilate_radius=1, **kwargs):
        return disp_error_image(D_est_tensor, D_gt_tensor, abs_thres, rel_thres, dilate_radius, **kwargs)

    __call__ = forward

    def backward(self, grad_output):
        return None


# ------------------------------------------------------------------------------------------------ class colours
def _palette(device, dtype):
    return _const(("palette", dtype), device, lambda: torch.tensor(PALETTE + ((0, 0, 0),), dtype=dtype))      # row 6: no class


def _colours_torch(cls, dtype):
    """[B,3,H,W] from a class map int64 [B,H,W] with 6 standing for "no class"."""
    return _palette(cls.device, dtype)[cls].permute(0, 3, 1, 2).contiguous()


def _color_hip(src, code, B, C, H, W, row, img, dtype):
    out = torch.empty((B, 3, H, W), dtype=dtype, device=src.device)
    with torch.cuda.device(src.device):
        call("ss_class_color_fwd", ptr(src), code, B, C, H, W, row, img, ptr(out), _OUT_CODES[dtype])
    return out


@_nograd
def feature_vis(feats, dtype=torch.float32):
    """utils/mask_vis.py:5-31: the first maximum over the channels of `feats` [B,C,H,W] (a NaN counts as the maximum) in the palette
    black, red, green, blue, yellow, cyan, values 0 and 255: a tensor [B,3,H,W] of `dtype` (float32 or uint8) on the input's device."""
    assert feats.dim() == 4 and dtype in _OUT_CODES
    B, C, H, W = feats.shape
    if E.VIS_HIP and feats.is_cuda and feats.dtype == torch.float32 and C <= NCLS and _fits(B, H, W):
        count("vis_hip")
        return _color_hip(_c(feats), -1, B, C, H, W, W, H * W, dtype)
    count("vis_torch")
    cls = argmax_first(feats)
    return _colours_torch(torch.where(cls < NCLS, cls, torch.full_like(cls, NCLS)), dtype)


@_nograd
def label_vis(labels, dtype=torch.float32):
    """What the scripts get from feature_vis(F.one_hot(label.to(torch.int64), 6).permute(0, 3, 1, 2).float()) (main_us3d.py:266),
    from the label map [B,H,W] itself (any integer or floating dtype, any strides with a unit stride along a row)."""
    assert labels.dim() == 3 and dtype in _OUT_CODES
    B, H, W = labels.shape
    if E.VIS_HIP and labels.is_cuda and not labels.is_complex() and _fits(B, H, W):
        count("vis_hip")
        y = labels if labels.dtype in LABEL_CODES else labels.to(torch.int64)
        if y.stride(2) != 1 or y.stride(1) < W or (B > 1 and y.stride(0) < (H - 1) * y.stride(1) + W):
            y = y.contiguous()
        image_stride = max(y.stride(0), (H - 1) * y.stride(1) + W)                 # (the stride of a batch of one is arbitrary)
        return _color_hip(y, LABEL_CODES[y.dtype], B, NCLS, H, W, y.stride(1), image_stride, dtype)
    count("vis_torch")
    return _colours_torch(_label_classes(labels, NCLS), dtype)


# ------------------------------------------------------------------------------------------------ normalisation
def _normalize_torch(x):
    B, C = x.shape[:2]
    flat = x.reshape(B, -1)
    lo, hi = flat.amin(1).view(B, 1, 1, 1), flat.amax(1).view(B, 1, 1, 1)
    out = (torch.maximum(torch.minimum(x, hi), lo) - lo) / (hi - lo).clamp(min=1e-5)
    return out.expand(B, 3, *x.shape[2:]).contiguous() if C == 1 else out


@_nograd
def normalize_image(x):
    """The normalisation save_images asks of make_grid (utils/experiment.py:90-98), per image: `x` [B,C,H,W] or [B,H,W] (one channel)
    -> (clamp(x, lo, hi) - lo) / max(hi - lo, 1e-5) with lo, hi the image's minimum and maximum; a one-channel image comes back with
    three equal channels, as make_grid returns it.  Finite input only: nothing is promised for NaN or inf."""
    if x.dim() == 3:
        x = x.unsqueeze(1)
    assert x.dim() == 4
    B, C, H, W = x.shape
    if E.VIS_HIP and x.is_cuda and x.dtype == torch.float32 and 0 < B <= 1024 and x[0].numel() > 0:
        count("vis_hip")
        x = _c(x)
        minmax = torch.empty((B, 2), dtype=torch.float32, device=x.device)
        ws = torch.empty(workspace_bytes() // 4, dtype=torch.float32, device=x.device)
        out = torch.empty((B, 3 if C == 1 else C, H, W), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            call("ss_image_minmax_fwd", ptr(x), B, C * H * W, ptr(minmax), ptr(ws), ws.numel() * 4)
            call("ss_image_normalize_fwd", ptr(x), ptr(minmax), ptr(out), B, C, H * W)
        return out
    count("vis_torch")
    return _normalize_torch(x if x.is_floating_point() else x.float())


# ------------------------------------------------------------------------------------------------ the evaluation step
@_nograd
def eval_images(disp_ests, label_est, disp_gt, label_true, imgL=None, first=1, normalize=True):
    """The image_outputs dictionary of test_sample (main_us3d.py:252, :266-268): "disp_est" and "errormap" (a list with one picture per
    estimate), "disp_gt", "imgL" (if given), "label" and "label_est" (lists of one; left out where `label_true` / `label_est` is None,
    which gives the dictionary of main_whu.py:242, :250-251), computed for the first `first` images of the batch
    only -- save_images logs `value[:1]`, so the default does a quarter of the reference's work at batch 4; `first=None`: the whole
    batch.  With `normalize` every entry is the [first,3,H,W] picture in [0, 1] that save_images hands to the logger; without it the
    entries are what the script stores (disparities [first,H,W], colours 0 / 255).  `disp_gt` is taken as it is: the script's
    disp_gt[disp_gt < -871] = 0 (:248) comes before.  Everything stays on the device and nothing waits on the host."""
    cut = (lambda t: t) if first is None else (lambda t: t[:first])
    fin = normalize_image if normalize else (lambda t: t)
    ests, gt = [cut(e) for e in disp_ests], cut(disp_gt)
    out = {"disp_est": [fin(e) for e in ests], "disp_gt": fin(gt)}
    if imgL is not None:
        out["imgL"] = fin(cut(imgL))
    if label_true is not None:
        out["label"] = [fin(label_vis(cut(label_true)))]
    if label_est is not None:
        out["label_est"] = [fin(feature_vis(cut(label_est)))]
    out["errormap"] = [fin(disp_error_image(e, gt)) for e in ests]
    return out
