#!/usr/bin/env python3
"""Generate tests/golden/decoder_train.npz by running the REFERENCE's own 2-D decoder layers in train(), in float64 on the CPU.

Runs ONLY where the reference checkout is mounted (the build container): it imports the reference's Conv2x and SemStereo by path
(nothing is copied, `timm` is a stand-in as in make_golden.py: the backbone never runs), fills them with the closed-form weights and
BatchNorm statistics of `decoder_cases.fill`, feeds them the closed-form inputs of `decoder_train_cases`, back-propagates the
closed-form linear loss and stores the output, the gradients of both inputs and of every parameter, and each BatchNorm's buffers
after the call: whole where small, else sum, sum of squares and sampled elements.  Deterministic: two runs give identical bytes.

    python tests/golden/make_golden_decoder_train.py
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from golden import decoder_cases as dc  # noqa: E402
from golden import decoder_train_cases as tc  # noqa: E402
from golden import make_golden as mg  # noqa: E402
from golden import make_golden_decoder as mgd  # noqa: E402

warnings.filterwarnings("ignore")
torch.set_num_threads(1)


def _store(out, case, res):
    for key, t in res.items():
        name = f"{case}/{key}"
        if key.endswith("num_batches_tracked"):
            out[name] = np.asarray([int(t)], dtype=np.int64)
        else:
            out[name] = tc.record(t, tc.salt_of(name))


def generate():
    ms = mg.load_ref_model_module()
    import models.submodule as sub
    out = {}
    for n, (Cin, Cout, _) in tc.CONV2X.items():
        mod = dc.fill(sub.Conv2x(Cin, Cout, deconv=True), tc.SALTS[n])
        _store(out, n, tc.run(mod, tc.conv2x_inputs(n), n))
    net = ms.SemStereo(64, False, True, True, 6)
    assert tuple(net.spx2[0].weight.shape) == (tc.SPX2[0], tc.SPX2[1], 4, 4)
    _store(out, "spx2", tc.run(dc.fill(net.spx2, tc.SALTS["spx2"]), [tc.spx2_input()], "spx2"))
    return out


if __name__ == "__main__":
    assert os.path.isdir(mg.REF), "the reference is only mounted in the build container"
    out = generate()
    path = os.path.join(HERE, "decoder_train.npz")
    mgd.save(out, path)
    for k in sorted(out):
        print(k, out[k].dtype, out[k].shape)
    print("decoder_train.npz:", len(out), "arrays,", os.path.getsize(path) // 1024, "KiB")
