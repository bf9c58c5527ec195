"""Inputs of the joint stereo-semantic fixtures (tests/golden/joint_metrics.npz): every case of metrics_cases.py -- its estimates, ground
truth, mask, first logits and first label tensor -- and one case of this file's own, `class_gap`, in which image 0 has no pixel of
class 2 while image 1 has.  Shared by make_golden_joint_metrics.py, which feeds them to the reference's own utils/metrics.py one class,
image and estimate at a time, and by the tests, which feed them to semstereo_amd.joint_metrics.

The class map here is written apart from the library's decoding, which it checks: a label's class in [0, 6), else 6 ("outside");
float labels truncate toward zero, NaN is outside."""
import numpy as np
import torch

from golden import metrics_cases as mc
from oracle import detdata as dd

NCLS = mc.NCLS
THRESHOLDS = mc.THRESHOLDS
METRICS = mc.METRICS                       # (fixture name, _, reference function of the *_mask variant, threshold or None)
FLAG = {"D1": 0, "Thres1": 1, "Thres2": 2, "Thres3": 3}          # field of record["cls_counts"] with thresholds=THRESHOLDS

OWN = {"class_gap": dict(B=2, H=10, W=20, nest=2, maxdisp=32, label_dtype=torch.uint8, pad=(0, 4), seed=9800)}
CASES = dict(mc.CASES, **OWN)


def _class_gap():
    c = OWN["class_gap"]
    B, H, W, s = c["B"], c["H"], c["W"], c["seed"]
    gt = dd.t_uniform((B, H, W), s, -40.0, 40.0)
    ests = [gt + 1.5 * dd.t_normalish((B, H, W), s + 10 + i) for i in range(c["nest"])]
    mask = mc.range_mask(gt, c["maxdisp"])
    ratio = mc.skip_ratio(mask, gt)
    assert all(not abs(r - 0.1) <= 1e-3 for r in ratio), ratio           # metrics_cases' margin: both readings of the skip rule agree
    logits = 2.0 * dd.t_normalish((B, NCLS, H, W), s + 3)
    labels = mc._labels((B, H + c["pad"][0], W + c["pad"][1]), s + 2, NCLS)
    labels[0][labels[0] == 2] = 1                                        # image 0: no pixel of class 2
    return dict(ests=ests, gt=gt, mask=mask, mask_img=None, maxdisp=c["maxdisp"], range_form=True, logits=logits,
                labels=labels.to(c["label_dtype"]))


def inputs(name):
    """metrics_cases.inputs(name), or the same dictionary for a case of this file (one batch of logits and labels)."""
    return _class_gap() if name in OWN else mc.inputs(name)


def classes(d):
    """int64 [B,H,W]: the class of every pixel of the case's first label tensor, cropped to the ground truth's H x W."""
    H, W = d["gt"].shape[1:]
    y = d["labels"][:, :H, :W]
    if y.is_floating_point():
        v = torch.from_numpy(np.trunc(y.numpy().astype(np.float64)))
        inside = ~torch.isnan(v) & (v >= 0) & (v < NCLS)
        return torch.where(inside, torch.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0), torch.full_like(v, NCLS)).long()
    v = y.long()
    return torch.where((v >= 0) & (v < NCLS), v, torch.full_like(v, NCLS))
