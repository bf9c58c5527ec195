#!/usr/bin/env python3
"""Generate tests/golden/loss.npz by running the REFERENCE's own models/loss.py (imported by path; nothing is copied) on the closed-form
inputs of loss_cases.py, on the CPU in float64 and float32.  Runs only where the reference is mounted (REF below, as in make_golden.py); the tests elsewhere read the
committed file.  Stored per case and function: the loss and every input gradient of the float64 run, the loss of the float32 run and,
for LRSC_loss, the warped label map of both runs.  The gradients keep 36 of float64's 52 mantissa bits (1.5e-11 relative, against the
tests' tightest bound of 1e-9): random mantissas do not compress, and with all 52 the file would pass the 1 MiB limit of a committed file.

    python tests/golden/make_golden_loss.py            # writes tests/golden/loss.npz
"""
import importlib.util
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

from golden import loss_cases  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "loss.npz")


def load_ref_losses():
    """models/loss.py with an empty stand-in for its `from utils import *` (nothing of it is used by the four functions)."""
    if "utils" not in sys.modules:
        sys.modules["utils"] = types.ModuleType("utils")
    spec = importlib.util.spec_from_file_location("ref_loss", os.path.join(REF, "models/loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def warped_labels(ref, name, dtype):
    """The label map LRSC_loss hands to its cross-entropy (models/loss.py:133), captured through the function's own `label_ce`."""
    d = loss_cases.inputs(name)
    seen, orig = [], ref.label_ce
    ref.label_ce = lambda pred, y, ignore=-1: (seen.append(y.detach().clone()), orig(pred, y, ignore=ignore))[1]
    try:
        ref.LRSC_loss(d["logits_r"].to(dtype), [d["ests"][0].to(dtype)], d["labels"])
    finally:
        ref.label_ce = orig
    return seen[0].numpy().astype(np.int64)


def keep36(a):
    """float64 array rounded to 36 mantissa bits (to nearest); non-finite values untouched."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    bits = a.view(np.uint64)
    r = ((bits + np.uint64(0x8000)) & ~np.uint64(0xFFFF)).view(np.float64)
    return np.where(np.isfinite(a), r, a)


def generate(path=OUT):
    warnings.filterwarnings("ignore")
    threads = torch.get_num_threads()
    torch.set_num_threads(8)
    try:
        ref = load_ref_losses()
        out = {}
        for name in loss_cases.CASES:
            r64 = loss_cases.run(ref, name, torch.float64)
            r32 = loss_cases.run(ref, name, torch.float32, grads=False)
            for fn in loss_cases.FUNCTIONS:
                out[f"{name}/{fn}/loss64"] = np.float64(r64[fn][0].item())
                out[f"{name}/{fn}/loss32"] = np.float32(r32[fn][0].item())
                for i, g in enumerate(r64[fn][1]):
                    out[f"{name}/{fn}/grad64/{i}"] = keep36(g.numpy())
            out[f"{name}/lrsc/warped32"] = warped_labels(ref, name, torch.float32).astype(np.int8)
            out[f"{name}/lrsc/warped64"] = warped_labels(ref, name, torch.float64).astype(np.int8)
            m = loss_cases.range_mask(loss_cases.inputs(name)["gt"], loss_cases.CASES[name]["maxdisp"])
            out[f"{name}/mask_kept"] = np.float64(m.double().mean().item())
        np.savez_compressed(path, **out)
    finally:
        torch.set_num_threads(threads)
    return out


if __name__ == "__main__":
    assert os.path.isdir(REF), "the reference is only mounted in the build container"
    res = generate()
    for k in sorted(res):
        if k.endswith(("loss64", "loss32", "mask_kept")):
            print(k, res[k])
    print("loss.npz:", len(res), "arrays,", os.path.getsize(OUT) // 1024, "KiB")
