#!/usr/bin/env python3
"""Generate tests/golden/metrics.npz by running the REFERENCE's own utils/metrics.py and utils/experiment.py (imported by path under a
stand-in `utils` package; nothing is copied) on the closed-form inputs of metrics_cases.py, on the CPU in float32 and float64.  Runs
only where the reference is mounted (REF below, as in make_golden_loss.py); the tests elsewhere read the committed file.

`torchvision` is not needed by anything that runs here; an empty stand-in module answers utils/experiment.py's import of it.  The
reference's addBatch uses `np.int`, which numpy removed in 1.24: the generator process sets `numpy.int = int`, which is what the name
meant in the numpy the reference was written for.

Stored, numeric arrays only:
  <case>/<metric>/batch32, batch64      [n_est]     the metric of the whole batch, float32 and float64 inputs
  <case>/<metric>/image32, image64      [n_est, B]  ... of each image alone (0 where the image is skipped)
  <case>/n_sel, n_mask, n_pos           [B]         selected pixels, masked pixels, pixels with gt > 0
  <case>/confusion1, confusion2         [5, 5]      SegmentationMetric(5).confusionMatrix after one and after two addBatch calls
  <case>/scores                         [3 + 5 + 5] PA, MPA, mIoU, CPA[5], IoU[5] after the second
  avg/all, avg/valid, avg/valid_present [keys]      the means of AverageMeterDict and AverageMeterDict2 over metrics_cases.avg_sequence()

    python tests/golden/make_golden_metrics.py            # writes tests/golden/metrics.npz
"""
import contextlib
import importlib.util
import io
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from golden import metrics_cases as mc  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "metrics.npz")


def _by_path(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_ref():
    """(utils/metrics.py, utils/experiment.py) of the reference under a stand-in `utils` package."""
    saved = {k: sys.modules.get(k) for k in ("utils", "utils.experiment", "torchvision", "torchvision.utils")}
    try:
        if "torchvision" not in sys.modules:
            tv = types.ModuleType("torchvision")
            tv.utils = types.ModuleType("torchvision.utils")
            sys.modules["torchvision"], sys.modules["torchvision.utils"] = tv, tv.utils
        pkg = types.ModuleType("utils")
        pkg.__path__ = []
        sys.modules["utils"] = pkg
        exp = _by_path("utils.experiment", "utils/experiment.py")
        pkg.experiment = exp
        met = _by_path("ref_metrics", "utils/metrics.py")
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
        sys.modules.pop("ref_metrics", None)
    return met, exp


def generate(path=OUT):
    warnings.filterwarnings("ignore")
    threads = torch.get_num_threads()
    torch.set_num_threads(8)
    had_int = hasattr(np, "int")
    if not had_int:
        np.int = int
    try:
        met, exp = load_ref()
        out = {}
        with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
            for name in mc.CASES:
                d = mc.inputs(name)
                for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
                    res = mc.run_disparity(met, d, dtype)
                    for key, (batch, images) in res.items():
                        np_t = np.float32 if tag == "32" else np.float64
                        out[f"{name}/{key}/batch{tag}"] = np.asarray(batch, dtype=np_t)
                        out[f"{name}/{key}/image{tag}"] = np.asarray(images, dtype=np_t)
                out[f"{name}/n_sel"], out[f"{name}/n_mask"], out[f"{name}/n_pos"] = mc.counts(d)
                m = met.SegmentationMetric(mc.NCLS - 1)
                m.addBatch(d["logits"], d["labels"])
                out[f"{name}/confusion1"] = m.confusionMatrix.copy()
                m.addBatch(d["logits2"], d["labels2"])
                out[f"{name}/confusion2"] = m.confusionMatrix.copy()
                out[f"{name}/scores"] = np.concatenate([[m.pixelAccuracy(), m.meanPixelAccuracy(), m.meanIntersectionOverUnion()],
                                                        m.classPixelAccuracy(), m.IoU()]).astype(np.float64)
            seq = mc.avg_sequence()
            a, b = exp.AverageMeterDict(), exp.AverageMeterDict2()
            for row in seq:
                a.update({k: [float(v)] for k, v in zip(mc.AVG_KEYS, row)})
                b.update({k: [float(v)] for k, v in zip(mc.AVG_KEYS, row)})
            ma, mb = a.mean(), b.mean()
            out["avg/all"] = np.asarray([ma[k][0] for k in mc.AVG_KEYS], dtype=np.float64)
            out["avg/valid"] = np.asarray([mb.get(k, np.nan) for k in mc.AVG_KEYS], dtype=np.float64)
            out["avg/valid_present"] = np.asarray([k in mb for k in mc.AVG_KEYS])
        np.savez_compressed(path, **out)
    finally:
        if not had_int:
            del np.int
        torch.set_num_threads(threads)
    return out


if __name__ == "__main__":
    assert os.path.isdir(REF), "the reference is only mounted in the build container"
    res = generate()
    for k in sorted(res):
        if k.endswith(("batch32", "scores")) or k.startswith("avg/"):
            print(k, res[k])
    print("metrics.npz:", len(res), "arrays,", os.path.getsize(OUT) // 1024, "KiB")
