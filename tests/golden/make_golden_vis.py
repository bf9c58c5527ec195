#!/usr/bin/env python3
"""Generate tests/golden/vis.npz by running the REFERENCE's own utils/visualization.py and utils/mask_vis.py (imported by path; nothing is
copied) on the closed-form inputs of vis_cases.py, on the CPU.  Runs only where the reference is mounted (REF below, as in
make_golden_metrics.py); the tests elsewhere read the committed file.  Before anything is written the generator asserts what
vis_cases.check_error_inputs states about the inputs: every colour row populated, a pixel exactly on every finite threshold, the share of
invalid pixels, the NaN / inf / zero specials.

Stored, numeric arrays only:
  err/<case>      float32 [B,3,H,W]   disp_error_image_func.forward(est, gt)
  logits/<case>   uint8   [B,3,H,W]   feature_vis(logits); the reference returns float64 holding 0 and 255, asserted before the cast
  labels/<case>   uint8   [B,3,H,W]   feature_vis(F.one_hot(labels.to(int64), 6).permute(0, 3, 1, 2).float())   (main_us3d.py:266)
  colormap        float32 [10,5]      the reference's error_colormap

The archive is written with fixed member dates, so the same arrays give the same file.

    python tests/golden/make_golden_vis.py            # writes tests/golden/vis.npz
"""
import importlib.util
import os
import sys
import warnings
import zipfile

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from golden import vis_cases as vc  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "vis.npz")


def _by_path(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_ref():
    """(utils/visualization.py, utils/mask_vis.py) of the reference; both import only torch and numpy."""
    return _by_path("ref_visualization", "utils/visualization.py"), _by_path("ref_mask_vis", "utils/mask_vis.py")


def _as_uint8(mask):
    assert mask.dtype == np.float64 and np.array_equal(mask, mask.astype(np.uint8)) and set(np.unique(mask)) <= {0.0, 255.0}
    return mask.astype(np.uint8)


def save_deterministic(path, arrays):
    """np.savez_compressed with fixed member dates (numpy stamps the members with the current time)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, "w", force_zip64=True) as fid:
                np.lib.format.write_array(fid, np.ascontiguousarray(arrays[key]), allow_pickle=False)


def generate(path=OUT):
    warnings.filterwarnings("ignore")
    vc.check_error_inputs()
    vis, mv = load_ref()
    out = {"colormap": np.asarray(vis.error_colormap, dtype=np.float32)}
    assert np.array_equal(out["colormap"][:, 0], vc.BOUNDS)
    with np.errstate(all="ignore"):
        for name in vc.ERROR_CASES:
            d = vc.error_inputs(name)
            img = vis.disp_error_image_func.forward(None, d["est"], d["gt"])         # (forward never reads self)
            assert img.dtype == torch.float32
            out[f"err/{name}"] = img.numpy()
        for name in vc.LOGIT_CASES:
            out[f"logits/{name}"] = _as_uint8(mv.feature_vis(vc.logit_inputs(name)["logits"]))
        for name in vc.LABEL_CASES:
            y = vc.label_inputs(name)["labels"]
            out[f"labels/{name}"] = _as_uint8(mv.feature_vis(F.one_hot(y.to(torch.int64), vc.NCLS).permute(0, 3, 1, 2).float()))
    save_deterministic(path, out)
    return out


if __name__ == "__main__":
    assert os.path.isdir(REF), "the reference is only mounted in the build container"
    res = generate()
    for k in sorted(res):
        print(k, res[k].dtype, res[k].shape)
    print("vis.npz:", len(res), "arrays,", os.path.getsize(OUT) // 1024, "KiB")
