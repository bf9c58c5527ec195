"""The evaluation step's metrics of the reference (utils/metrics.py; main_us3d.py:214-219, :225-263) under its own names and signatures.

  EPE_metric / D1_metric / Thres_metric               utils/metrics.py:16-59   per image, skipped where the mask is too small, then averaged
  EPE_metric_mask / D1_metric_mask / Thres_metric_mask  :63-89                 ... over `mask_img`, the skip rule still reading `mask`
  SegmentationMetric                                   :91-213                  confusion matrix and the five scores derived from it
  disparity_metrics                                    one launch for all values of up to four estimates, staying on the device
  eval_metrics                                         main_us3d.py:254-263     the two dictionaries of test_sample, device tensors
  EvalAverager                                         utils/experiment.py:136-217   AverageMeterDict / AverageMeterDict2 on the device

CUDA fp32 inputs run csrc/metrics.hip: a reduction launch and a small finish launch per call, every result staying on the device -- no
per-image loop, no `nonzero`, no copy of the logits to the host.  Everything else (CPU tensors, float64, other channel counts,
SS_METRICS_HIP=0) takes the PyTorch composition below, written without boolean indexing and without `.cpu()`, so it does not wait on
the host either.  modules.PATH_COUNTS["metrics_hip"] / ["metrics_torch"] count the calls of each path.

Departures from the reference, on both paths: nothing is printed for a skipped image (printing needs the host to know); a negative
label counts as "outside" like any other label that is no class, where np.bincount raises a ValueError; with float64 inputs a batch
whose images are all skipped gives a float64 0, not a float32 one.  Reproduced on purpose: SegmentationMetric(numClass) on logits of
more than numClass channels folds (label g, prediction numClass) into cell (g + 1, 0), because the reference histograms
g * numClass + prediction; `fold=False` and `jointMatrix` give the honest counts.

Across ranks: the joint matrix and the record of `disparity_metrics` are plain sums, so a torch.distributed.all_reduce of the two
buffers adds them.
"""
import numpy as np
import torch

from . import _lib
from . import engine as E
from ._host import LABEL_CODES, _c, _label_classes, _nograd, argmax_first, count          # (argmax_first: also this module's name for it)
from ._lib import call, ptr

NCLS = 6                                   # channels the confusion kernel is built for
NAMES = ("EPE_metric", "D1_metric", "Thres_metric", "EPE_metric_mask", "D1_metric_mask", "Thres_metric_mask", "SegmentationMetric")
COUNT_FIELDS = ("n_sel", "n_mask", "n_pos", "n_d1", "n_thr0", "n_thr1", "n_thr2", "n_thr3")      # record["counts"][..., i]
_MAPS = {}


def workspace_bytes(kind):
    """Scratch of the entry points: kind 0 = ss_disparity_metrics_fwd, 1 = ss_seg_confusion_fwd."""
    return _lib.query_bytes("ss_metrics_workspace_bytes", kind)


def _workspace(kind, device):
    return torch.empty(workspace_bytes(kind) // 8 + 1, dtype=torch.int64, device=device)


def _check_shapes(*ts):
    for t in ts:                           # utils/metrics.py:9-13
        assert len(t.size()) == 3
        assert t.size() == ts[0].size()


def _as_bool(m):
    return m if m.dtype == torch.bool else m != 0


# ------------------------------------------------------------------------------------------------ disparity metrics
def _disparity_torch(ests, gt, mask, mask_img, rng, thresholds):
    """The composition: (out [n_est, 2 + T] in the inputs' dtype, counts int64 [n_est, B, 8], sums float64 [n_est, B])."""
    inmask = _as_bool(mask) if mask is not None else (gt >= rng[0]) & (gt < rng[1])
    sel = _as_bool(mask_img) if mask_img is not None else inmask
    n_sel, n_mask, n_pos = sel.sum((1, 2)), inmask.sum((1, 2)), (gt > 0).sum((1, 2))
    keep = ~(n_mask.double() / n_pos.double() < 0.1)            # utils/metrics.py:25 from the integers; x / 0 and 0 / 0 keep the image
    n_kept = keep.sum()
    outs, counts, sums = [], [], []
    zero = torch.zeros((), dtype=torch.float64, device=gt.device)
    for est in ests:
        err = (gt - est).abs()
        total = torch.where(sel, err, torch.zeros_like(err)).sum((1, 2), dtype=torch.float64)
        d1 = (sel & (err > 3) & (err / gt.abs() > 0.05)).sum((1, 2))
        thr = [(sel & (err > t)).sum((1, 2)) for t in thresholds]
        thr4 = thr + [torch.zeros_like(d1)] * (4 - len(thr))
        counts.append(torch.stack([n_sel, n_mask, n_pos, d1] + thr4, dim=1))
        sums.append(total)
        # EPE in float64.  D1 and Thres as the reference forms them whatever the inputs' dtype: the mean of a float32 0 / 1 tensor per
        # image (utils/metrics.py:43, :52: an exact float32 sum and one float32 division), then a float32 mean over the kept images.
        epe = torch.where(keep, total / n_sel.double(), zero).sum() / n_kept.double()                       # 0 / 0 = NaN
        shares = torch.stack([c.float() for c in [d1] + thr], dim=0) / n_sel.float()                        # [1 + T, B]
        mean = torch.where(keep, shares, shares.new_zeros(())).sum(1) / n_kept.float()
        vals = torch.cat([epe.reshape(1), mean.double()])
        outs.append(torch.where(n_kept > 0, vals, zero))
    return torch.stack(outs).to(gt.dtype), torch.stack(counts), torch.stack(sums)


def supported_disparity(ests, gt, mask, mask_img):
    """One to four CUDA fp32 estimates [B,H,W] and a ground truth of that shape on one device, bool masks of that shape (or None), at
    most 1024 images of fewer than 2^31 pixels."""
    if not 1 <= len(ests) <= 4 or not isinstance(gt, torch.Tensor) or gt.dim() != 3 or not gt.is_cuda or gt.dtype != torch.float32:
        return False
    if not 0 < gt.shape[0] <= 1024 or not 0 < gt[0].numel() < 2 ** 31:
        return False
    for e in ests:
        if not (isinstance(e, torch.Tensor) and e.dtype == torch.float32 and e.device == gt.device and e.shape == gt.shape):
            return False
    for m in (mask, mask_img):
        if m is not None and not (isinstance(m, torch.Tensor) and m.dtype == torch.bool and m.device == gt.device and m.shape == gt.shape):
            return False
    return True


def _disparity_hip(ests, gt, mask, mask_img, rng, thresholds):
    dev, B, n, T = gt.device, gt.shape[0], gt[0].numel(), len(thresholds)
    ests, gt = [_c(e) for e in ests], _c(gt)
    mask, mask_img = (None if m is None else _c(m) for m in (mask, mask_img))
    out = torch.empty((len(ests), 2 + T), dtype=torch.float32, device=dev)
    counts = torch.empty((len(ests), B, 8), dtype=torch.int64, device=dev)
    sums = torch.empty((len(ests), B), dtype=torch.float64, device=dev)
    ws = _workspace(0, dev)
    thr = [float(t) for t in thresholds] + [0.0] * (4 - T)
    with torch.cuda.device(dev):
        call("ss_disparity_metrics_fwd", *[ptr(ests[i]) if i < len(ests) else None for i in range(4)], ptr(gt), ptr(mask), ptr(mask_img),
             len(ests), B, n, float(rng[0]), float(rng[1]), *thr, T, ptr(out), ptr(counts), ptr(sums), ptr(ws), ws.numel() * 8)
    return out, counts, sums


@_nograd
def disparity_metrics(disp_ests, disp_gt, mask=None, maxdisp=None, thresholds=(1.0, 2.0), mask_img=None, return_record=False):
    """EPE, D1 and Thres(t) of every estimate in `disp_ests` ([B,H,W] each, at most four on the kernel path) against `disp_gt`, all from
    one pass: a device tensor [n_est, 2 + len(thresholds)] with the columns EPE, D1, Thres(t_0), ... -- each the reference's value
    (per-image values, images with mean(mask) / mean(gt > 0) < 0.1 skipped, mean over the rest; 0 if none is left; NaN if a kept image
    selects nothing).  Nothing waits on the host.

    The mask is `mask` (bool [B,H,W]) or, with `maxdisp`, the range -maxdisp <= gt < maxdisp of main_us3d.py:235 evaluated inside the
    kernel: no mask tensor is built.  The scripts overwrite disp_gt[disp_gt < -871] = 0 AFTER building their mask (:248) and before the
    metric calls.  The range form must be given the UNTOUCHED ground truth: an overwritten pixel reads 0 and would count as inside the
    range.  On the untouched tensor those pixels are outside the mask and not positive, exactly as in the script, so the values are
    the script's.  `mask_img`: the selection of the *_mask variants (the skip rule still reads the mask).

    return_record: also {"counts": int64 [n_est, B, 8] (COUNT_FIELDS), "sums": float64 [n_est, B] (sum of |gt - est| over the
    selection)} per estimate and image -- plain sums, for tests and for epoch- or rank-level aggregation."""
    ests = list(disp_ests)
    _check_shapes(*ests, disp_gt, *([mask] if mask is not None else []), *([mask_img] if mask_img is not None else []))
    if (mask is None) == (maxdisp is None):
        raise ValueError("give either `mask` or `maxdisp`")
    thresholds = tuple(float(t) for t in thresholds)
    rng = (0.0, 0.0) if maxdisp is None else (-float(maxdisp), float(maxdisp))
    if E.METRICS_HIP and len(thresholds) <= 4 and supported_disparity(ests, disp_gt, mask, mask_img):
        count("metrics_hip")
        out, counts, sums = _disparity_hip(ests, disp_gt, mask, mask_img, rng, thresholds)
    else:
        count("metrics_torch")
        gt = disp_gt
        ests = [e.to(gt.dtype) for e in ests]
        out, counts, sums = _disparity_torch(ests, gt, mask, mask_img, rng, thresholds)
    return (out, {"counts": counts, "sums": sums}) if return_record else out


def _one(D_ests, D_gts, masks, column, thresholds=(), mask_img=None):
    _check_shapes(D_ests, D_gts, masks)
    return disparity_metrics([D_ests], D_gts, mask=masks, thresholds=thresholds, mask_img=mask_img)[0, column]


def EPE_metric(D_ests, D_gts, masks):
    """utils/metrics.py:55-59: mean |est - gt| over the mask, per image, averaged over the images that are not skipped."""
    return _one(D_ests, D_gts, masks, 0)


def D1_metric(D_ests, D_gts, masks):
    """utils/metrics.py:37-43: share of masked pixels with E > 3 and E / |gt| > 0.05."""
    return _one(D_ests, D_gts, masks, 1)


def Thres_metric(D_ests, D_gts, masks, thres):
    """utils/metrics.py:45-52: share of masked pixels with E > thres."""
    assert isinstance(thres, (int, float))
    return _one(D_ests, D_gts, masks, 2, (thres,))


def EPE_metric_mask(D_ests, D_gts, masks, mask_img):
    """utils/metrics.py:83-89: EPE over `mask_img`; `masks` only decides which images are skipped."""
    return _one(D_ests, D_gts, masks, 0, (), mask_img)


def D1_metric_mask(D_ests, D_gts, masks, mask_img):
    """utils/metrics.py:63-70."""
    return _one(D_ests, D_gts, masks, 1, (), mask_img)


def Thres_metric_mask(D_ests, D_gts, masks, thres, mask_img):
    """utils/metrics.py:72-80."""
    assert isinstance(thres, (int, float))
    return _one(D_ests, D_gts, masks, 2, (thres,), mask_img)


# ------------------------------------------------------------------------------------------------ confusion matrix
def _joint_torch(logits, labels):
    """int64 [C + 1, C]: label class (row C: no class of the logits) x prediction, labels cropped to the logits' H, W."""
    B, C, H, W = logits.shape
    g = _label_classes(labels[:, :H, :W], C)
    index = (g * C + argmax_first(logits)).reshape(-1)
    joint = torch.zeros((C + 1) * C, dtype=torch.int64, device=logits.device)
    joint.index_add_(0, index, torch.ones_like(index))
    return joint.view(C + 1, C)


def supported_confusion(logits, labels):
    """CUDA fp32 logits [B,6,H,W] with fewer than 2^31 elements, labels [B,>=H,>=W] on the same device."""
    if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 4):
        return False
    B, C, H, W = logits.shape
    if C != NCLS or not 0 < logits.numel() < 2 ** 31:
        return False
    return (isinstance(labels, torch.Tensor) and labels.device == logits.device and labels.dim() == 3 and labels.shape[0] == B
            and labels.shape[1] >= H and labels.shape[2] >= W and not labels.is_complex())


def _fold_map(C, numClass, fold):
    """Cell of the [numClass, numClass] matrix that joint cell (g, p) lands in; numClass^2 = nowhere.  fold: the reference's index
    g * numClass + p with index < numClass^2 kept (utils/metrics.py:157-166); else the top-left block of the joint matrix."""
    m = np.full((C + 1, C), numClass * numClass, dtype=np.int64)
    for g in range(C):
        for p in range(C):
            if fold and g * numClass + p < numClass * numClass:
                m[g, p] = g * numClass + p
            elif not fold and g < numClass and p < numClass:
                m[g, p] = g * numClass + p
    return m.reshape(-1)


def fold_joint(joint, numClass, fold=True, ignore=None):
    """float64 numpy [numClass, numClass] from a joint matrix [C + 1, C] (numpy)."""
    joint = np.asarray(joint)
    C = joint.shape[1]
    if ignore:
        joint = joint.copy()
        if 0 <= ignore < C:
            joint[ignore] = 0
    out = np.zeros(numClass * numClass + 1)
    np.add.at(out, _fold_map(C, numClass, fold), joint.reshape(-1).astype(np.float64))
    return out[:-1].reshape(numClass, numClass)


class SegmentationMetric(object):
    """utils/metrics.py:91-213 with the state on the device: `addBatch` is one launch that adds the batch's joint histogram of (label,
    argmax) to an int64 matrix there; `confusionMatrix` (float64 numpy [numClass, numClass], the reference's attribute) is read back
    on first use -- one copy of 336 bytes -- and cached until the next addBatch / reset.  Not in the reference: `jointMatrix`,
    `fold=False`, `scores()`."""

    def __init__(self, numClass, fold=True):
        self.numClass = numClass
        self.fold = bool(fold)
        self._joint = None                 # int64 [C + 1, C] on the device of the first batch
        self._cache = None
        self._map = None

    # ---- state
    def addBatch(self, imgPredict, imgLabel):
        with torch.no_grad():
            C = imgPredict.shape[1]
            if self._joint is None or self._joint.shape[1] != C or self._joint.device != imgPredict.device:
                if self._joint is not None and bool((self._joint != 0).any()):
                    raise ValueError("addBatch: logits of another device or channel count than the batches already added")
                self._joint = torch.zeros((C + 1, C), dtype=torch.int64, device=imgPredict.device)
                self._map = None
            _joint_add(imgPredict, imgLabel, self._joint)
        self._cache = None

    def reset(self):
        if self._joint is not None:
            self._joint.zero_()
        self._cache = None

    @property
    def jointMatrix(self):
        """The honest counts: int64 numpy [C + 1, C], label class (last row: no class) x prediction.  Waits on the device."""
        if self._joint is None:
            return np.zeros((NCLS + 1, NCLS), dtype=np.int64)
        return self._joint.cpu().numpy()

    @property
    def confusionMatrix(self):
        if self._cache is None:
            self._cache = (np.zeros((self.numClass,) * 2) if self._joint is None else fold_joint(self.jointMatrix, self.numClass, self.fold))
        return self._cache

    def get_confusion_matrix(self, label, pred, num_class=5, ignore=None):
        """The matrix of one batch (float64 numpy; waits on the device), with the reference's signature and fold."""
        with torch.no_grad():
            joint = torch.zeros((pred.shape[1] + 1, pred.shape[1]), dtype=torch.int64, device=pred.device)
            _joint_add(pred, label, joint)
        return fold_joint(joint.cpu().numpy(), num_class, self.fold, ignore)

    # ---- the reference's scores, on the host from the cached matrix
    def pixelAccuracy(self):
        m = self.confusionMatrix
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.diag(m).sum() / m.sum()

    def classPixelAccuracy(self):
        m = self.confusionMatrix
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.diag(m) / m.sum(axis=1)

    def meanPixelAccuracy(self):
        return _nanmean(self.classPixelAccuracy())

    def IoU(self):
        m = self.confusionMatrix
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.diag(m) / (m.sum(axis=1) + m.sum(axis=0) - np.diag(m))

    def meanIntersectionOverUnion(self):
        return _nanmean(self.IoU())

    # ---- the same on the device
    def device_matrix(self):
        """The [numClass, numClass] matrix as a float64 device tensor (no host wait)."""
        if self._joint is None:
            raise ValueError("no batch added yet")
        if self._map is None:
            key = (self._joint.shape[1], self.numClass, self.fold, self._joint.device)
            if key not in _MAPS:
                _MAPS[key] = torch.from_numpy(_fold_map(*key[:3])).to(key[3], non_blocking=True)
            self._map = _MAPS[key]
        n = self.numClass
        out = torch.zeros(n * n + 1, dtype=torch.float64, device=self._joint.device)
        out.index_add_(0, self._map, self._joint.reshape(-1).double())
        return out[:-1].view(n, n)

    def scores(self):
        """{"PA", "MPA", "mIoU": 0-dim, "CPA", "IoU": [numClass]} as float64 device tensors: what test_sample reads
        (main_us3d.py:258-263), without waiting on the host."""
        m = self.device_matrix()
        diag, rows, cols = torch.diagonal(m), m.sum(1), m.sum(0)
        cpa, iou = diag / rows, diag / (rows + cols - diag)
        return {"PA": diag.sum() / m.sum(), "MPA": torch.nanmean(cpa), "mIoU": torch.nanmean(iou), "CPA": cpa, "IoU": iou}


def _nanmean(v):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanmean(v)


def _joint_add(logits, labels, joint):
    """joint += the joint histogram of this batch, on the kernel where it applies."""
    if E.METRICS_HIP and supported_confusion(logits, labels) and joint.is_contiguous():
        count("metrics_hip")
        logits = _c(logits)
        if labels.dtype not in LABEL_CODES:
            labels = labels.to(torch.int64)
        B, C, H, W = logits.shape
        if labels.stride(2) != 1 or labels.stride(1) < W or (B > 1 and labels.stride(0) < (H - 1) * labels.stride(1) + W):
            labels = labels[:, :H, :W].contiguous()
        image_stride = max(labels.stride(0), (H - 1) * labels.stride(1) + W)             # (the stride of a batch of one is arbitrary)
        ws = _workspace(1, logits.device)
        with torch.cuda.device(logits.device):
            call("ss_seg_confusion_fwd", ptr(logits), ptr(labels), LABEL_CODES[labels.dtype], B, C, H, W, labels.stride(1), image_stride,
                 ptr(joint), 1, ptr(ws), ws.numel() * 8)
    else:
        count("metrics_torch")
        joint += _joint_torch(logits, labels)


# ------------------------------------------------------------------------------------------------ the evaluation step
@_nograd
def eval_metrics(disp_ests, label_est, disp_gt, label_true, maxdisp, num_classes=6, thresholds=(1.0, 2.0)):
    """main_us3d.py:254-263: (scalar_outputs, scalar_outputs2) with its keys -- "D1", "EPE", "Thres1", "Thres2" (a list with one value
    per estimate), "PA", "MPA", "mIoU", and "CPA<i>", "IoU<i>" for i < num_classes - 1 (lists of one) -- every value a 0-dim device
    tensor.  Two launches and their finishes in all; nothing waits on the host.  `disp_gt` must be the ground truth BEFORE the script's
    disp_gt[disp_gt < -871] = 0 (:248), because the mask is the range -maxdisp <= gt < maxdisp evaluated on it (see disparity_metrics)."""
    ests = list(disp_ests)
    vals = disparity_metrics(ests, disp_gt, maxdisp=maxdisp, thresholds=thresholds)
    out = {"D1": [vals[i, 1] for i in range(len(ests))], "EPE": [vals[i, 0] for i in range(len(ests))]}
    for k, t in enumerate(thresholds):
        out[f"Thres{t:g}"] = [vals[i, 2 + k] for i in range(len(ests))]
    metric = SegmentationMetric(num_classes - 1)                   # :228
    metric.addBatch(label_est, label_true)
    s = metric.scores()
    out["PA"], out["MPA"], out["mIoU"] = [s["PA"]], [s["MPA"]], [s["mIoU"]]
    out2 = {}
    for i in range(num_classes - 1):
        out2["CPA" + str(i)] = [s["CPA"][i]]
        out2["IoU" + str(i)] = [s["IoU"][i]]
    return out, out2


class EvalAverager(object):
    """AverageMeterDict (mode "all") and AverageMeterDict2 (mode "valid") of utils/experiment.py:136-217 with the sums on the device:
    `update` adds a dictionary of 0-dim tensors (or lists of them, or floats) into a float64 record without waiting, `mean()` makes one
    transfer.  Sums are sequential in float64 like the reference's Python `+=`, so the means are the same bits given the same values.

      "all"    a NaN adds 0 but the batch still counts; the first batch is taken as it is, NaN included (the deepcopy of :145)
      "valid"  a NaN neither adds nor counts; mean() gives, per key, (sum of the key's first entry) / (valid entries of the key), and
               leaves out keys without a valid value"""

    def __init__(self, mode="all"):
        if mode not in ("all", "valid"):
            raise ValueError("mode is 'all' or 'valid'")
        self.mode = mode
        self.count = 0
        self._layout = None                # [(key, length or None for a bare value)]
        self._sums = self._valid = None

    def _flatten(self, x):
        layout, vals = [], []
        for k, v in x.items():
            seq = list(v) if isinstance(v, (list, tuple)) else [v]
            layout.append((k, len(seq) if isinstance(v, (list, tuple)) else None))
            vals += seq
        dev = next((v.device for v in vals if isinstance(v, torch.Tensor)), torch.device("cpu"))
        if all(isinstance(v, torch.Tensor) for v in vals):
            flat = torch.stack([v.detach().reshape(()).to(torch.float64) for v in vals])
        else:
            host = torch.tensor([float("nan") if isinstance(v, torch.Tensor) else float(v) for v in vals], dtype=torch.float64)
            flat = host.to(dev, non_blocking=True)
            for i, v in enumerate(vals):
                if isinstance(v, torch.Tensor):
                    flat[i] = v.detach().reshape(()).to(torch.float64)
        return layout, flat

    @torch.no_grad()
    def update(self, x):
        layout, flat = self._flatten(x)
        if self._layout is None:
            self._layout = layout
            self._sums = torch.zeros_like(flat)
            self._valid = torch.zeros_like(flat)
            if self.mode == "all":
                self._sums = flat.clone()
                self.count = 1
                return
        elif layout != self._layout:
            raise ValueError("update: keys or list lengths differ from the first batch")
        nan = torch.isnan(flat)
        self._sums += torch.where(nan, torch.zeros_like(flat), flat)
        self._valid += (~nan).to(torch.float64)
        self.count += 1

    def mean(self):
        if self._layout is None:
            return {} if self.mode == "valid" else None
        host = torch.stack([self._sums, self._valid]).cpu().numpy()
        out, i = {}, 0
        for k, n in self._layout:
            m = 1 if n is None else n
            s, c = host[0, i:i + m], host[1, i:i + m]
            i += m
            if self.mode == "all":
                vals = [float(v) / float(self.count) for v in s]
                out[k] = vals[0] if n is None else vals
            elif c.sum() != 0:
                out[k] = float(s[0]) / int(c.sum())
        return out
