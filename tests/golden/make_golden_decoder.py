#!/usr/bin/env python3
"""Generate tests/golden/decoder.npz by running the REFERENCE's own 2-D decoder modules.

Runs ONLY where the reference checkout is mounted (the build container): it imports the reference's Conv2x, FeatUp and SemStereo by
path (nothing is copied, `timm` is a stand-in as in make_golden.py: the backbone never runs), fills them with the closed-form
weights and BatchNorm statistics of `decoder_cases.fill`, feeds them the closed-form inputs of `decoder_cases` and stores the
OUTPUTS: whole where small, else sum, sum of squares and sampled elements.  Deterministic: two runs give identical bytes (one
thread, a fixed-timestamp uncompressed .npz).

    python tests/golden/make_golden_decoder.py
"""
import os
import sys
import warnings
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from golden import decoder_cases as dc  # noqa: E402
from golden import make_golden as mg  # noqa: E402

warnings.filterwarnings("ignore")
torch.set_num_threads(1)


def generate():
    ms = mg.load_ref_model_module()
    import models.submodule as sub
    out = {}
    with torch.no_grad():
        for n, (B, Cin, Cout, H, W, Hr, Wr) in dc.CONV2X.items():
            mod = dc.fill(sub.Conv2x(Cin, Cout, deconv=True).eval(), dc.conv2x_salt(n))
            x, rem = dc.conv2x_inputs(n)
            out[f"conv2x/{n}"] = dc.record(mod(x, rem), 0)
        fu = dc.fill(ms.FeatUp().eval(), dc.FEATUP_SALT)
        featL, featR = dc.featup_inputs()
        L, R = fu(featL, featR)
        for side, maps in (("L", L), ("R", R)):
            for k, t in enumerate(maps):
                out[f"featup/{side}{k}"] = dc.record(t, 10 + k)
        net = ms.SemStereo(64, False, True, True, 6).eval()
        mods = {name: dc.fill(getattr(net, name), salt) for name, salt in dc.SPX_SALTS.items()}
        for k, t in enumerate(dc.run_spx(mods, dc.spx_inputs())):
            out[f"spx/{k}"] = dc.record(t, 20 + k)
    return out


def save(out, path):
    """an uncompressed .npz with fixed member order and timestamps (np.savez stamps the members with the current time)."""
    import io
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for key in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(out[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_STORED
            z.writestr(info, buf.getvalue())


if __name__ == "__main__":
    assert os.path.isdir(mg.REF), "the reference is only mounted in the build container"
    out = generate()
    path = os.path.join(HERE, "decoder.npz")
    save(out, path)
    for k in sorted(out):
        print(k, out[k].dtype, out[k].shape)
    print("decoder.npz:", len(out), "arrays,", os.path.getsize(path) // 1024, "KiB")
