"""Closed-form inputs of the evaluation-metric fixtures (tests/golden/metrics.npz): shared by make_golden_metrics.py, which feeds them to
the reference's own utils/metrics.py and utils/experiment.py, and by the tests, which feed them to semstereo_amd.metrics.  Values come
from oracle.detdata, so they are the same bits wherever they are built.

A condition on every image of every case, asserted when the inputs are built: the skip rule's ratio n_mask / n_pos stays more than 1e-3
away from 0.1.  The reference compares it in float32 on the host, the library decides it from the integers; away from the edge both
agree."""
import numpy as np
import torch

from oracle import detdata as dd

NCLS = 6
THRESHOLDS = (1.0, 2.0, 3.0)
# (fixture name, reference function, reference function of the *_mask variant, threshold or None)
METRICS = (("EPE", "EPE_metric", "EPE_metric_mask", None), ("D1", "D1_metric", "D1_metric_mask", None),
           ("Thres1", "Thres_metric", "Thres_metric_mask", 1.0), ("Thres2", "Thres_metric", "Thres_metric_mask", 2.0),
           ("Thres3", "Thres_metric", "Thres_metric_mask", 3.0))
COLUMN = {"EPE": 0, "D1": 1, "Thres1": 2, "Thres2": 3, "Thres3": 4}        # column of disparity_metrics(..., thresholds=THRESHOLDS)

# name: batch, size, estimates, maxdisp of the range mask, label dtype, label tensor's extra rows / columns, seed
CASES = {
    "plain_b4": dict(B=4, H=32, W=48, nest=1, maxdisp=32, label_dtype=torch.int64, pad=(0, 0), seed=9100),
    "odd_23x41": dict(B=2, H=23, W=41, nest=2, maxdisp=32, label_dtype=torch.uint8, pad=(0, 0), seed=9200),
    "skips": dict(B=4, H=16, W=24, nest=1, maxdisp=32, label_dtype=torch.int64, pad=(0, 0), seed=9300),
    "nan_image": dict(B=2, H=12, W=20, nest=1, maxdisp=32, label_dtype=torch.int64, pad=(0, 0), seed=9400),
    "all_skipped": dict(B=2, H=12, W=16, nest=1, maxdisp=32, label_dtype=torch.int64, pad=(0, 0), seed=9500),
    "four_ests_mask_img": dict(B=2, H=20, W=36, nest=4, maxdisp=32, label_dtype=torch.float32, pad=(3, 5), seed=9600),
    "edges": dict(B=2, H=8, W=16, nest=1, maxdisp=32, label_dtype=torch.int64, pad=(0, 0), seed=9700),
}


def range_mask(gt, maxdisp):
    return (gt < maxdisp) & (gt >= -maxdisp)            # main_us3d.py:235


def _labels(shape, seed, top):
    """integers uniform in [0, top)"""
    return torch.from_numpy(np.minimum(np.floor(dd.uniform(shape, seed, 0.0, float(top))), top - 1).astype(np.int64))


def skip_ratio(mask, gt):
    """n_mask / n_pos per image in float64 (inf, NaN where no pixel is positive)."""
    return (mask.sum((1, 2)).double() / (gt > 0).sum((1, 2)).double()).numpy()


def inputs(name):
    """float32 `ests` (list), `gt`, bool `mask` (the range mask unless the case says otherwise), bool `mask_img` or None, `maxdisp`,
    `range_form` (the mask IS the range mask of gt), two batches of `logits` [B,6,H,W] and `labels` [B,H+,W+] for addBatch."""
    c = CASES[name]
    B, H, W, s = c["B"], c["H"], c["W"], c["seed"]
    gt = dd.t_uniform((B, H, W), s, -40.0, 40.0)
    ests = [gt + 1.5 * dd.t_normalish((B, H, W), s + 10 + i) for i in range(c["nest"])]
    mask, mask_img, range_form = None, None, True
    if name == "skips":
        range_form = False
        mask = range_mask(gt, c["maxdisp"])
        mask[0] = False
        mask[0, 0, :5] = True                                  # image 0: 5 masked pixels against ~190 positive ones: skipped
        gt[1] = -gt[1].abs() - 0.5                             # image 1: nothing positive, a mask that is not empty: ratio inf, kept
        mask[1] = gt[1] >= -20.0
        ests[0][1] = gt[1] + 1.5 * dd.t_normalish((H, W), s + 20)
    if name == "nan_image":
        range_form = False
        mask = range_mask(gt, c["maxdisp"])
        gt[1] = -gt[1].abs() - 0.5                             # image 1: nothing positive and an empty mask: 0 / 0, kept, every metric NaN
        mask[1] = False
    if name == "all_skipped":
        range_form = False
        mask = torch.zeros((B, H, W), dtype=torch.bool)
        mask[:, 1, 2:6] = True                                 # 4 masked pixels per image
    if name == "four_ests_mask_img":
        mask_img = dd.t_uniform((B, H, W), s + 30) > -0.2      # another selection than the mask, partly outside it
    if name == "edges":
        g, e = gt[0], ests[0][0]
        g[0, :4] = 0.0                                         # gt == 0 inside the mask: E / 0
        e[0, :4] = torch.tensor([0.0, 2.5, 3.5, -4.0])         # 0 / 0 (NaN: not counted), 2.5 / 0, 3.5 / 0 and 4 / 0 (inf)
        e[1, :4] = g[1, :4]                                    # est == gt
        g[2, :6] = torch.tensor([4.0, -7.0, 10.0, 16.0, -20.0, 30.0])
        e[2, :6] = g[2, :6] + torch.tensor([1.0, -1.0, 2.0, -2.0, 3.0, -3.0])      # E exactly 1, 2, 3: not above the threshold
        g[3, :6] = torch.tensor([60.0, 61.0, 70.0, 80.0, 64.0, 100.0])             # E > 3 with E / |gt| on both sides of 0.05 (and on it)
        e[3, :6] = g[3, :6] + torch.tensor([3.0, 3.05, 3.25, 4.1, 3.2, 5.0])
        ests[0][1, 3, 5] = float("nan")                        # image 1: a NaN estimate inside the mask
        gt[1, 3, 5] = 7.0
        range_form = False
        mask = range_mask(gt, c["maxdisp"])
        mask[0, 3, :6] = True                                  # (|gt| >= 32 is outside the range mask: these pixels are put in by hand)
    if mask is None:
        mask = range_mask(gt, c["maxdisp"])
    ratio = skip_ratio(mask, gt)
    assert all(not abs(r - 0.1) <= 1e-3 for r in ratio), (name, ratio)
    out = dict(ests=ests, gt=gt, mask=mask, mask_img=mask_img, maxdisp=c["maxdisp"], range_form=range_form)
    for k, off in (("", 0), ("2", 50)):
        logits = 2.0 * dd.t_normalish((B, NCLS, H, W), s + 3 + off)
        labels = _labels((B, H + c["pad"][0], W + c["pad"][1]), s + 2 + off, NCLS)
        if name == "odd_23x41":
            labels[0, :4] = _labels((4, W), s + 40 + off, 9)           # labels 6, 7, 8: no class
            labels[1, 5, :7] = 255
        if name == "four_ests_mask_img":
            labels[:, 2] = _labels((B, W + c["pad"][1]), s + 41 + off, 8)
        if name == "edges":
            logits[0, :, 0] = 0.5                                      # all six channels equal: the first wins
            logits[0, 2:4, 1] = 9.0                                    # channels 2 and 3 tie for the maximum
            logits[0, 4, 2, :8] = float("nan")                         # a NaN channel is the maximum
            logits[0, 1, 2, 4:8] = float("nan")                        # ... and of two NaNs the first
            logits[0, 5, 3] = 9.0                                      # prediction 5: folded into the next row's column 0
            labels[0, 3, :8] = 4                                       # ... or, for label 4, off the end
        if name == "nan_image":
            logits[:, 3] = -50.0                                       # class 3 absent from the prediction ...
            logits[:, 5] = -50.0                                       # (... and nothing folded into row 3)
            labels[labels == 3] = 1                                    # ... and from the labels: CPA and IoU of class 3 are 0 / 0
        labels = labels.to(c["label_dtype"])
        if labels.is_floating_point():
            labels[:, 4] += 0.7                                        # float labels truncate
        out["logits" + k], out["labels" + k] = logits, labels
    return out


def run_disparity(lib, d, dtype, device="cpu"):
    """The metric functions of `lib` (the reference's utils/metrics.py, or semstereo_amd.metrics) on the inputs `d` with their own
    signatures: {fixture name: ([batch value per estimate], [[per-image value] per estimate])}, Python floats.  Cases with a `mask_img`
    run the *_mask variants."""
    cast = lambda t: t.to(device=device, dtype=dtype)                       # noqa: E731
    gt, mask = cast(d["gt"]), d["mask"].to(device)
    mimg = None if d["mask_img"] is None else d["mask_img"].to(device)
    B = gt.shape[0]
    out = {}
    for key, plain, masked, thr in METRICS:
        fn = getattr(lib, plain if mimg is None else masked)

        def call(est, sl):
            args = [est[sl], gt[sl], mask[sl]] + ([] if thr is None else [thr]) + ([] if mimg is None else [mimg[sl]])
            return float(fn(*args))
        batch, images = [], []
        for est in d["ests"]:
            est = cast(est)
            batch.append(call(est, slice(0, B)))
            images.append([call(est, slice(i, i + 1)) for i in range(B)])
        out[key] = (batch, images)
    return out


def counts(d):
    """n_sel, n_mask, n_pos per image (int64 arrays)."""
    sel = d["mask"] if d["mask_img"] is None else d["mask_img"]
    return (sel.sum((1, 2)).numpy().astype(np.int64), d["mask"].sum((1, 2)).numpy().astype(np.int64),
            (d["gt"] > 0).sum((1, 2)).numpy().astype(np.int64))


def kept(d):
    """Which images the skip rule keeps (bool array), from the integers."""
    r = skip_ratio(d["mask"], d["gt"])
    return ~(r < 0.1)


# ---- the averaging meters: a fixed sequence of per-batch dictionaries (lists of one value, as test_sample builds them)
AVG_KEYS = ("EPE", "D1", "Thres1", "PA", "mIoU", "CPA3", "never")
AVG_BATCHES = 6


def avg_sequence():
    """float64 [AVG_BATCHES, len(AVG_KEYS)]: values that are exact in float32, NaNs in the first, a middle and the last batch, and a
    key that is NaN throughout."""
    v = dd.uniform((AVG_BATCHES, len(AVG_KEYS)), 9900, 0.0, 3.0).astype(np.float64)
    v[0, 1] = v[3, 0] = v[3, 5] = v[AVG_BATCHES - 1, 2] = v[AVG_BATCHES - 1, 5] = np.nan
    v[0, 5] = np.nan
    v[:, 6] = np.nan
    return v
