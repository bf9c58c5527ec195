#!/usr/bin/env python3
"""Generate tests/golden/data.npz by running the REFERENCE's own datasets/us3d_.py and datasets/whu_dataset.py (imported by path;
nothing is copied): every case of data_cases.py is written to temporary TIFF / 16-bit PNG files with PIL, listed in a list file, and read
back through the real Us3dDataset / WhuDataset `__getitem__`, training branch (where the size allows one) and test branch.  Runs only where
the reference is mounted (REF below, as in make_golden_vis.py); the tests elsewhere read the committed file.

cv2 and torchvision are not installed where this runs.  Two small stand-in modules are installed before the import:
  cv2                       resize(a, (w, h), interpolation=INTER_NEAREST) as OpenCV's resizeNN forms it: source index
                            min(floor(d * ifx), size - 1), ifx = 1.0 / (double(dst) / double(src)); for sizes the factor does not divide
                            this formula is taken from OpenCV's source and is unverified
  torchvision.transforms    ToTensor (HWC uint8 -> CHW float32 `.div(255)`), Normalize (`.sub_(mean).div_(std)` with float32 mean and
                            std tensors) and Compose: their documented fp32 arithmetic
So the arrays come from two sources, kept apart in two key prefixes:
  ref/<case>/<key>      gx, gy, disparity, label           the reference's own code, on real PIL / numpy / scipy
  closed/<case>/<key>   left, right, the pyramid levels    the stand-ins
Items of a case are stacked: left, right float32 [B,3,H,W]; gx, gy float32 [B,1,H,W]; disparity, label float32 [B,H,W]; level k
[B, H // k, W // k].  Both branches must agree on every entry they share; before anything is written the generator asserts that the
constant case is NaN on every pixel of gx and gy and that no other array holds a NaN.  Numeric arrays only, fixed member dates: the same
arrays give the same file.

    python tests/golden/make_golden_data.py            # writes tests/golden/data.npz
"""
import importlib.util
import os
import sys
import tempfile
import types
import warnings
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from golden import data_cases as dc  # noqa: E402

REF = "/root/reference"
OUT = os.path.join(HERE, "data.npz")


# ------------------------------------------------------------------------------------------------ the stand-ins
def _nn_index(dst, src):
    ifx = 1.0 / (float(dst) / float(src))
    return np.minimum(np.floor(np.arange(dst, dtype=np.float64) * ifx).astype(np.int64), src - 1)


def _resize(a, dsize, interpolation=None):
    assert interpolation == 0 and a.ndim == 2
    w, h = dsize
    assert w > 0 and h > 0, "cv2.resize refuses an empty destination"
    return np.ascontiguousarray(a[_nn_index(h, a.shape[0])][:, _nn_index(w, a.shape[1])])


class _ToTensor:
    def __call__(self, pic):
        a = np.array(pic, dtype=np.uint8)
        assert a.ndim == 3
        return torch.from_numpy(a).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


class _Normalize:
    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, t):
        mean = torch.as_tensor(self.mean, dtype=t.dtype).view(-1, 1, 1)
        std = torch.as_tensor(self.std, dtype=t.dtype).view(-1, 1, 1)
        return t.clone().sub_(mean).div_(std)


class _Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


def install_stand_ins():
    cv2 = types.ModuleType("cv2")
    cv2.INTER_NEAREST, cv2.resize = 0, _resize
    tv, tr = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tr.ToTensor, tr.Normalize, tr.Compose = _ToTensor, _Normalize, _Compose
    tv.transforms = tr
    for name, mod in (("cv2", cv2), ("torchvision", tv), ("torchvision.transforms", tr)):
        assert name not in sys.modules, f"{name} is installed: use it instead of the stand-in and say so in the docstring"
        sys.modules[name] = mod


def _by_path(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_ref():
    """(datasets/us3d_.py, datasets/whu_dataset.py) of the reference, with datasets/data_io.py under the name they import it by."""
    install_stand_ins()
    sys.modules.setdefault("datasets", types.ModuleType("datasets"))
    _by_path("datasets.data_io", "datasets/data_io.py")
    return _by_path("ref_us3d", "datasets/us3d_.py"), _by_path("ref_whu", "datasets/whu_dataset.py")


def save_deterministic(path, arrays):
    """np.savez_compressed with fixed member dates (numpy stamps the members with the current time)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, "w", force_zip64=True) as fid:
                np.lib.format.write_array(fid, np.ascontiguousarray(arrays[key]), allow_pickle=False)


def _np(v):
    return v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def generate(path=OUT):
    warnings.filterwarnings("ignore")
    us3d, whu = load_ref()
    out = {}
    with tempfile.TemporaryDirectory() as folder, np.errstate(all="ignore"):
        for name, c in dc.CASES.items():
            lst = dc.write_case(name, folder)
            cls = us3d.Us3dDataset if c["kind"] == "us3d" else whu.WhuDataset
            test = cls(folder, lst, False)
            train = cls(folder, lst, True) if dc.has_training_branch(name) else None
            assert len(test) == c["B"]
            items = []
            for i in range(c["B"]):
                t = test[i]
                assert t["top_pad"] == 0 and t["right_pad"] == 0 and t["left_filename"] == f"{name}_{i}_left.tif"
                item = {k: _np(v) for k, v in t.items() if k not in ("top_pad", "right_pad", "left_filename")}
                if train is not None:
                    for k, v in train[i].items():
                        v = _np(v)
                        assert k not in item or np.array_equal(item[k], v, equal_nan=True), (name, k)
                        item[k] = v
                items.append(item)
            keep = dc.VIEW_KEYS + dc.GRAD_KEYS + ("disparity",) + (("label",) if c["kind"] == "us3d" else ()) + dc.level_keys(name)
            for k in keep:
                a = np.stack([it[k] for it in items])
                assert a.dtype == np.float32, (name, k, a.dtype)
                prefix = "ref" if k in dc.GRAD_KEYS + ("disparity", "label") else "closed"
                if name == dc.NAN_CASE and k in dc.GRAD_KEYS:
                    assert np.isnan(a).all(), (name, k)
                else:
                    assert not np.isnan(a).any(), (name, k)
                out[f"{prefix}/{name}/{k}"] = a
    save_deterministic(path, out)
    return out


if __name__ == "__main__":
    assert os.path.isdir(REF), "the reference is only mounted in the build container"
    res = generate()
    for k in sorted(res):
        print(k, res[k].dtype, res[k].shape)
    print("data.npz:", len(res), "arrays,", os.path.getsize(OUT) // 1024, "KiB")
