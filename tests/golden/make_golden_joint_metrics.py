#!/usr/bin/env python3
"""Generate tests/golden/joint_metrics.npz: the REFERENCE's own EPE_metric_mask / D1_metric_mask / Thres_metric_mask (utils/metrics.py,
loaded by path exactly as make_golden_metrics.py loads it; nothing is copied) on the inputs of joint_metrics_cases.py, with
mask_img = mask & (class == c) for every class c in 0..6 (6 = outside), every image ALONE ([i:i+1]) and every estimate, on the CPU in
float32 and float64.  Runs only where the reference is mounted; the tests elsewhere read the committed file.

Stored, numeric arrays only:
  <case>/<metric>/image32, image64   [n_est, B, 7]   the metric of image i alone over mask & class c (0 where the image is skipped,
                                                     NaN where it has no such pixel); metric in EPE, D1, Thres1, Thres2, Thres3
  <case>/cls_sel                     [B, 7] int64    pixels of mask & class c

    python tests/golden/make_golden_joint_metrics.py      # writes tests/golden/joint_metrics.npz
"""
import contextlib
import io
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from golden import joint_metrics_cases as jc  # noqa: E402
from golden import make_golden_metrics as mg  # noqa: E402

REF = mg.REF
OUT = os.path.join(HERE, "joint_metrics.npz")


def generate(path=OUT):
    warnings.filterwarnings("ignore")
    threads = torch.get_num_threads()
    torch.set_num_threads(8)
    try:
        met, _ = mg.load_ref()
        out = {}
        with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
            for name in jc.CASES:
                d = jc.inputs(name)
                cls, mask = jc.classes(d), d["mask"]
                B = mask.shape[0]
                out[f"{name}/cls_sel"] = np.asarray([[int((mask[i] & (cls[i] == c)).sum()) for c in range(jc.NCLS + 1)] for i in range(B)],
                                                    dtype=np.int64)
                for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
                    gt = d["gt"].to(dtype)
                    for key, _plain, masked, thr in jc.METRICS:
                        fn = getattr(met, masked)
                        vals = np.zeros((len(d["ests"]), B, jc.NCLS + 1), dtype=np.float32 if tag == "32" else np.float64)
                        for e, est in enumerate(d["ests"]):
                            est = est.to(dtype)
                            for i in range(B):
                                sl = slice(i, i + 1)
                                for c in range(jc.NCLS + 1):
                                    args = [est[sl], gt[sl], mask[sl]] + ([] if thr is None else [thr]) + [mask[sl] & (cls[sl] == c)]
                                    vals[e, i, c] = float(fn(*args))
                        out[f"{name}/{key}/image{tag}"] = vals
        np.savez_compressed(path, **out)
    finally:
        torch.set_num_threads(threads)
    return out


if __name__ == "__main__":
    assert os.path.isdir(REF), "the reference is only mounted in the build container"
    res = generate()
    for k in sorted(res):
        if k.endswith("cls_sel"):
            print(k, res[k].tolist())
    print("joint_metrics.npz:", len(res), "arrays,", os.path.getsize(OUT) // 1024, "KiB")
