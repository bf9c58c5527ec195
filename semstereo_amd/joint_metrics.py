"""The joint stereo-semantic evaluation: disparity error per semantic class, and mIoU-3 -- IoU in which a pixel is a true positive only
if its class is right AND its disparity error is below `tau` = 3 px, the joint score of the pairwise semantic-stereo track US3D was
released for.  The reference started on the per-class table and left it as comments (datasets/us3d_.py:76-96 builds
label_disparity_dict and never fills it); the definitions here are this project's and are written out in `joint_metrics`.

  joint_metrics        the record of one batch, per image: one launch of csrc/joint_metrics.hip plus its finish
  JointMetric          the record accumulated over an epoch on the device, and the scores derived from it
  eval_metrics_joint   the per-batch dictionary in test_sample's shape, for EvalAverager("valid")

CUDA fp32 inputs run the kernel: every tensor eval_metrics reads is read once, nothing waits on the host.  Everything else (CPU
tensors, float64, other channel counts, SS_JOINT_METRICS_HIP=0) takes the PyTorch composition below, written without boolean indexing
and without `.cpu()`.  modules.PATH_COUNTS["joint_metrics_hip"] / ["joint_metrics_torch"] count the calls of each path.

Across ranks: `JointMetric.state()` is plain sums, so a torch.distributed.all_reduce of its tensors adds ranks.
"""
import torch

from . import _lib
from . import engine as E
from ._host import LABEL_CODES, _c, _label_classes, _nograd, argmax_first, count
from ._lib import call, ptr
from .metrics import NCLS, _as_bool, _check_shapes, supported_confusion, supported_disparity

FLAG_FIELDS = ("n_d1", "n_thr0", "n_thr1", "n_thr2", "n_thr3")        # record["cls_counts"][..., i]
RECORD_KEYS = ("image", "cls_sel", "cls_counts", "cls_sums", "joint_all", "joint_out", "joint_good")


def scratch_bytes(n_est, B):
    """Scratch of ss_joint_metrics_fwd."""
    return _lib.query_bytes("ss_joint_metrics_scratch", n_est, B)


def _bins(index, weight, n):
    out = torch.zeros(n, dtype=torch.int64, device=index.device)
    out.index_add_(0, index.reshape(-1), weight.reshape(-1).to(torch.int64))
    return out


def _joint_torch(ests, logits, gt, labels, mask, rng, thresholds, tau, C):
    """The composition: the record of `joint_metrics` for logits of C channels (C + 1 label classes)."""
    B, H, W = gt.shape
    dev = gt.device
    inmask = _as_bool(mask) if mask is not None else (gt >= rng[0]) & (gt < rng[1])
    g = _label_classes(labels[:, :H, :W], C)
    img = torch.arange(B, device=dev).view(B, 1, 1)
    row = img * (C + 1) + g                                        # (image, class)
    rec = {"image": torch.stack([inmask.sum((1, 2)), (gt > 0).sum((1, 2))], dim=1),
           "cls_sel": _bins(row, inmask, B * (C + 1)).view(B, C + 1)}
    cell = None
    if logits is not None:
        cell = row * C + argmax_first(logits)                      # (image, class, prediction)
        rec["joint_all"] = _bins(cell, torch.ones_like(inmask), B * (C + 1) * C).view(B, C + 1, C)
        rec["joint_out"] = _bins(cell, ~inmask, B * (C + 1) * C).view(B, C + 1, C)
    else:
        rec["joint_all"] = rec["joint_out"] = None
    counts, sums, good = [], [], []
    for est in ests:
        err = (gt - est).abs()
        flags = [inmask & (err > 3) & (err / gt.abs() > 0.05)] + [inmask & (err > t) for t in thresholds]
        flags += [torch.zeros_like(inmask)] * (5 - len(flags))
        counts.append(torch.stack([_bins(row, f, B * (C + 1)).view(B, C + 1) for f in flags], dim=2))
        # the sum of each class as disparity_metrics forms it over mask & class: one float64 reduction per image
        sums.append(torch.stack([torch.where(inmask & (g == c), err, torch.zeros_like(err)).sum((1, 2), dtype=torch.float64)
                                 for c in range(C + 1)], dim=1))
        if cell is not None:
            good.append(_bins(cell, inmask & (err < tau), B * (C + 1) * C).view(B, C + 1, C))
    rec["cls_counts"], rec["cls_sums"] = torch.stack(counts), torch.stack(sums)
    rec["joint_good"] = torch.stack(good) if cell is not None else None
    return rec


def supported_joint(ests, logits, gt, labels, mask):
    """The conditions of metrics.supported_disparity and metrics.supported_confusion together: one to four CUDA fp32 estimates [B,H,W],
    a ground truth and (or None) a bool mask of that shape, fp32 logits [B,6,H,W] (or None), labels [B,>=H,>=W], all on one device."""
    if not supported_disparity(ests, gt, mask, None):
        return False
    B, H, W = gt.shape
    if logits is not None and not (supported_confusion(logits, labels) and logits.device == gt.device
                                   and tuple(logits.shape) == (B, NCLS, H, W)):
        return False
    return (isinstance(labels, torch.Tensor) and labels.device == gt.device and labels.dim() == 3 and labels.shape[0] == B
            and labels.shape[1] >= H and labels.shape[2] >= W and not labels.is_complex())


def _joint_hip(ests, logits, gt, labels, mask, rng, thresholds, tau):
    dev, (B, H, W), n, T = gt.device, gt.shape, len(ests), len(thresholds)
    ests, gt = [_c(e) for e in ests], _c(gt)
    mask = None if mask is None else _c(mask)
    logits = None if logits is None else _c(logits)
    if labels.dtype not in LABEL_CODES:
        labels = labels.to(torch.int64)
    if labels.stride(2) != 1 or labels.stride(1) < W or (B > 1 and labels.stride(0) < (H - 1) * labels.stride(1) + W):
        labels = labels[:, :H, :W].contiguous()
    image_stride = max(labels.stride(0), (H - 1) * labels.stride(1) + W)                 # (the stride of a batch of one is arbitrary)
    i64 = dict(dtype=torch.int64, device=dev)
    rec = {"image": torch.empty((B, 2), **i64), "cls_sel": torch.empty((B, NCLS + 1), **i64),
           "cls_counts": torch.empty((n, B, NCLS + 1, 5), **i64),
           "cls_sums": torch.empty((n, B, NCLS + 1), dtype=torch.float64, device=dev),
           "joint_all": None, "joint_out": None, "joint_good": None}
    if logits is not None:
        rec["joint_all"], rec["joint_out"] = torch.empty((B, NCLS + 1, NCLS), **i64), torch.empty((B, NCLS + 1, NCLS), **i64)
        rec["joint_good"] = torch.empty((n, B, NCLS + 1, NCLS), **i64)
    ws = torch.empty(scratch_bytes(n, B) // 8 + 1, **i64)
    thr = [float(t) for t in thresholds] + [0.0] * (4 - T)
    with torch.cuda.device(dev):
        call("ss_joint_metrics_fwd", *[ptr(ests[i]) if i < n else None for i in range(4)], ptr(gt), ptr(mask), ptr(logits), ptr(labels),
             LABEL_CODES[labels.dtype], labels.stride(1), image_stride, n, B, NCLS, H, W, float(rng[0]), float(rng[1]), *thr, T,
             float(tau), *[ptr(rec[k]) for k in RECORD_KEYS], ptr(ws), ws.numel() * 8)
    return rec


@_nograd
def joint_metrics(disp_ests, label_est, disp_gt, label_true, mask=None, maxdisp=None, thresholds=(1.0, 2.0), tau=3.0):
    """The joint record of one batch, PER IMAGE, as a dict of device tensors (C = channels of the logits, 6 on the kernel path):

      image       int64 [B, 2]                 n_mask, n_pos (= pixels with gt > 0): what the skip rule reads
      cls_sel     int64 [B, C + 1]             pixels in the mask, per class
      cls_counts  int64 [n_est, B, C + 1, 5]   FLAG_FIELDS: n_d1, n_thr0..3 of the pixels in the mask, per class
      cls_sums    float64 [n_est, B, C + 1]    sum of E over them
      joint_all, joint_out  int64 [B, C + 1, C]          every pixel / the pixels outside the mask, by (class, prediction)
      joint_good  int64 [n_est, B, C + 1, C]   the good pixels; bad = all - out - good

    disp_ests: estimates [B,H,W] (at most four on the kernel path); label_est: logits [B,C,H,W], or None (the three joint tables are
    None); label_true: labels [B,>=H,>=W], cropped to the logits without a copy.

    Mask: `mask` (bool [B,H,W]) or, with `maxdisp`, the range -maxdisp <= gt < maxdisp evaluated on the UNTOUCHED ground truth (the
    caveat of metrics.disparity_metrics about disp_gt[disp_gt < -871] = 0 applies).  E = |gt - est| in fp32.  d1 = E > 3 & E / |gt| >
    0.05; thr_k = E > thresholds[k] (at most four).  Class: the label's class in [0, C), or C for "outside" (float labels truncate
    toward zero, NaN is outside).  Prediction: the first maximum over the logits, a NaN counting as the maximum.  good = in the mask
    and E < tau; E == tau and a NaN E are not good.  One launch plus its finish, no host wait, never differentiable."""
    ests = list(disp_ests)
    _check_shapes(*ests, disp_gt, *([mask] if mask is not None else []))
    if (mask is None) == (maxdisp is None):
        raise ValueError("give either `mask` or `maxdisp`")
    thresholds = tuple(float(t) for t in thresholds)
    if len(thresholds) > 4:
        raise ValueError("at most four thresholds")
    rng = (0.0, 0.0) if maxdisp is None else (-float(maxdisp), float(maxdisp))
    if E.JOINT_METRICS_HIP and supported_joint(ests, label_est, disp_gt, label_true, mask):
        count("joint_metrics_hip")
        return _joint_hip(ests, label_est, disp_gt, label_true, mask, rng, thresholds, tau)
    count("joint_metrics_torch")
    C = NCLS if label_est is None else label_est.shape[1]
    return _joint_torch([e.to(disp_gt.dtype) for e in ests], label_est, disp_gt, label_true, mask, rng, thresholds, float(tau), C)


class JointMetric(object):
    """The joint record over an epoch, int64 / float64 sums on the device of the first batch.

    addBatch adds the record of the images the skip rule keeps (an image is kept unless n_mask / n_pos < 0.1, decided from the integers
    as metrics.disparity_metrics decides it; skip_rule=False keeps every image).  scores() derives, for the first `num_classes` classes:

      pool="pixel"  EPE_c = sum of E / n_c, D1_c and Thres<t>_c = count / n_c over all kept images' pixels of class c in the mask;
                    NaN for a class without such a pixel
      pool="image"  what the reference's EPE_metric_mask(est, gt, mask, mask & (label == c)) returns: the mean over the kept images of
                    the per-image means -- NaN where a kept image lacks the class, 0 where no image is kept
      IoU3_c = good[c][c] / (row_c + col_c - diag_c) on the honest [num_classes, num_classes] top-left block (no fold, as
      SegmentationMetric(num_classes, fold=False)), row, col and diag over the pixels the policy includes: invalid="ignore" drops the
      pixels outside the mask from everything, "pass" counts them as good, "fail" as bad.  mIoU3 is the nanmean over the classes; the
      ordinary IoU / mIoU over the same included pixels come with it.

    Nothing waits on the host."""

    def __init__(self, num_classes=5, thresholds=(1.0, 2.0), tau=3.0, skip_rule=True, invalid="ignore"):
        if invalid not in ("ignore", "pass", "fail"):
            raise ValueError("invalid is 'ignore', 'pass' or 'fail'")
        self.num_classes = int(num_classes)
        self.thresholds = tuple(float(t) for t in thresholds)
        if len(self.thresholds) > 4:
            raise ValueError("at most four thresholds")
        self.tau, self.skip_rule, self.invalid = float(tau), bool(skip_rule), invalid
        self._s = None

    # ---- state
    def _fresh(self, n_est, C, device):
        i64, f64 = dict(dtype=torch.int64, device=device), dict(dtype=torch.float64, device=device)
        return {"images": torch.zeros(2, **i64),                              # seen, kept
                "cls_sel": torch.zeros(C + 1, **i64), "cls_counts": torch.zeros((n_est, C + 1, 5), **i64),
                "cls_sums": torch.zeros((n_est, C + 1), **f64),
                "joint_all": torch.zeros((C + 1, C), **i64), "joint_out": torch.zeros((C + 1, C), **i64),
                "joint_good": torch.zeros((n_est, C + 1, C), **i64),
                "image_means": torch.zeros((n_est, C + 1, 6), **f64)}         # sums over the kept images of EPE, D1, Thres0..3 per image

    @_nograd
    def addBatch(self, disp_ests, label_est, disp_gt, label_true, mask=None, maxdisp=None):
        ests = list(disp_ests)
        if label_est is None:
            raise ValueError("addBatch needs the logits")
        rec = joint_metrics(ests, label_est, disp_gt, label_true, mask=mask, maxdisp=maxdisp, thresholds=self.thresholds, tau=self.tau)
        C, dev = label_est.shape[1], disp_gt.device
        if self._s is None:
            self._s = self._fresh(len(ests), C, dev)
        s = self._s
        if s["joint_good"].shape != (len(ests), C + 1, C) or s["cls_sel"].device != dev:
            raise ValueError("addBatch: another device, channel count or number of estimates than the batches already added")
        n_mask, n_pos = rec["image"][:, 0], rec["image"][:, 1]
        keep = ~(n_mask.double() / n_pos.double() < 0.1) if self.skip_rule else torch.ones_like(n_mask, dtype=torch.bool)
        k = keep.to(torch.int64)
        s["images"] += torch.stack([torch.full_like(k.sum(), k.numel()), k.sum()])
        s["cls_sel"] += (rec["cls_sel"] * k[:, None]).sum(0)
        s["cls_counts"] += (rec["cls_counts"] * k[None, :, None, None]).sum(1)
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        s["cls_sums"] += torch.where(keep[None, :, None], rec["cls_sums"], zero).sum(1)
        s["joint_all"] += (rec["joint_all"] * k[:, None, None]).sum(0)
        s["joint_out"] += (rec["joint_out"] * k[:, None, None]).sum(0)
        s["joint_good"] += (rec["joint_good"] * k[None, :, None, None]).sum(1)
        n_c = rec["cls_sel"].double()[None, :, :, None]                                                      # 0 / 0 = NaN
        per_image = torch.cat([rec["cls_sums"][..., None], rec["cls_counts"].double()], dim=3) / n_c         # [n_est, B, C + 1, 6]
        s["image_means"] += torch.where(keep[None, :, None, None], per_image, zero).sum(1)

    def reset(self):
        if self._s is not None:
            for v in self._s.values():
                v.zero_()

    def state(self):
        """The sums as a dict of tensors (copies): int64 counts and float64 sums, every one additive over batches and ranks."""
        if self._s is None:
            raise ValueError("no batch added yet")
        return {k: v.clone() for k, v in self._s.items()}

    def load_state(self, state):
        self._s = {k: v.clone() for k, v in state.items()}

    # ---- scores
    def _included(self):
        s = self._s
        if self.invalid == "ignore":
            return s["joint_all"] - s["joint_out"], s["joint_good"]
        if self.invalid == "pass":
            return s["joint_all"], s["joint_good"] + s["joint_out"][None]
        return s["joint_all"], s["joint_good"]

    @_nograd
    def scores(self, pool="pixel"):
        """{"EPE_c", "D1_c", "Thres<t>_c": [n_est, num_classes], "n_c": [num_classes], "IoU3": [n_est, num_classes], "mIoU3": [n_est],
        "IoU": [num_classes], "mIoU": 0-dim} as float64 device tensors."""
        if pool not in ("pixel", "image"):
            raise ValueError("pool is 'pixel' or 'image'")
        if self._s is None:
            raise ValueError("no batch added yet")
        s, n = self._s, self.num_classes
        n_c = s["cls_sel"][:n].double()
        if pool == "pixel":
            vals = torch.cat([s["cls_sums"][:, :n, None], s["cls_counts"][:, :n].double()], dim=2) / n_c[None, :, None]
        else:
            kept = s["images"][1]
            vals = torch.where(kept > 0, s["image_means"][:, :n] / kept.double(), torch.zeros_like(s["image_means"][:, :n]))
        out = {"EPE_c": vals[..., 0], "D1_c": vals[..., 1], "n_c": n_c}
        for i, t in enumerate(self.thresholds):
            out[f"Thres{t:g}_c"] = vals[..., 2 + i]
        included, good = self._included()
        m = included[:n, :n].double()
        diag, union = torch.diagonal(m), m.sum(1) + m.sum(0) - torch.diagonal(m)
        out["IoU3"] = torch.diagonal(good[:, :n, :n].double(), dim1=1, dim2=2) / union[None]
        out["mIoU3"] = torch.nanmean(out["IoU3"], dim=1)
        out["IoU"] = diag / union
        out["mIoU"] = torch.nanmean(out["IoU"])
        return out


@_nograd
def eval_metrics_joint(disp_ests, label_est, disp_gt, label_true, maxdisp, num_classes=6, thresholds=(1.0, 2.0), tau=3.0):
    """The joint scores of ONE batch in test_sample's shape (main_us3d.py:254-263): lists of 0-dim device tensors under "mIoU3" (one
    value per estimate) and, for i < num_classes - 1, "EPE_c<i>", "D1_c<i>", "IoU3_<i>" (one value per estimate each).  With one
    estimate the lists hold one value, the shape of scalar_outputs2, and suit EvalAverager("valid"), which leaves out the NaN of a class
    that a batch lacks (that meter reads the FIRST entry of a list; several estimates go to EvalAverager("all"), which keeps every
    entry).  `disp_gt` is the UNTOUCHED ground truth, as for eval_metrics.

    The mean of these per-batch values over an epoch is NOT the epoch's score: IoU and the per-class errors are ratios of sums.  The
    epoch-exact figure is JointMetric's -- addBatch every batch, scores() once."""
    ests = list(disp_ests)
    metric = JointMetric(num_classes - 1, thresholds=thresholds, tau=tau)
    metric.addBatch(ests, label_est, disp_gt, label_true, maxdisp=maxdisp)
    s = metric.scores()
    out = {"mIoU3": [s["mIoU3"][e] for e in range(len(ests))]}
    for i in range(num_classes - 1):
        out[f"EPE_c{i}"] = [s["EPE_c"][e, i] for e in range(len(ests))]
        out[f"D1_c{i}"] = [s["D1_c"][e, i] for e in range(len(ests))]
        out[f"IoU3_{i}"] = [s["IoU3"][e, i] for e in range(len(ests))]
    return out
