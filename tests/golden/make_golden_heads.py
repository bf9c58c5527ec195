#!/usr/bin/env python3
"""Generate tests/golden/heads.npz by running the REFERENCE's own segmentation head and chal_* projections.

Runs ONLY where the reference checkout is mounted (the build container): it imports the reference's segmenthead and SemStereo by path
(nothing is copied, `timm` is a stand-in as in make_golden.py: the backbone never runs), fills them with the closed-form weights and
BatchNorm statistics of `decoder_cases.fill`, feeds them the closed-form inputs of `heads_cases` and stores the OUTPUTS: whole where
small, else sum, sum of squares and sampled elements.  Deterministic: two runs give identical bytes (one thread, a fixed-timestamp
uncompressed .npz).

    python tests/golden/make_golden_heads.py
"""
import os
import sys
import warnings

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from golden import decoder_cases as dc  # noqa: E402
from golden import heads_cases as hc  # noqa: E402
from golden import make_golden as mg  # noqa: E402
from golden import make_golden_decoder as mgd  # noqa: E402

warnings.filterwarnings("ignore")
torch.set_num_threads(1)


def generate():
    ms = mg.load_ref_model_module()
    import models.submodule as sub
    with torch.no_grad():
        net = ms.SemStereo(64, False, True, True, 6).eval()
        head = dc.fill(net.head_l, hc.HEAD_SALT)
        ragged = dc.fill(sub.segmenthead(*hc.RAGGED[0]).eval(), hc.RAGGED_SALT)
        chals = {name: dc.fill(getattr(net, name), salt) for name, salt in hc.CHAL_SALTS.items()}
        return {key: dc.record(t, salt) for key, (t, salt) in hc.run_all(head, ragged, chals).items()}


if __name__ == "__main__":
    assert os.path.isdir(mg.REF), "the reference is only mounted in the build container"
    out = generate()
    path = os.path.join(HERE, "heads.npz")
    mgd.save(out, path)
    for k in sorted(out):
        print(k, out[k].dtype, out[k].shape)
    print("heads.npz:", len(out), "arrays,", os.path.getsize(path) // 1024, "KiB")
