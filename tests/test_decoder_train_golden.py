"""CPU: the 2-D decoder twins (modules.Conv2x, Spx2) in train(), in float64 -- the stock path -- against tests/golden/decoder_train.npz:
the output, the gradients of both inputs and of every parameter and each BatchNorm's buffers after the call, as the REFERENCE's own
Conv2x and SemStereo.spx2 give them on the closed-form weights, inputs and loss of golden/decoder_train_cases.py.  Bound: 1e-9, the
float64 bound of the loss fixtures."""
import os

import numpy as np
import pytest
import torch

from golden import decoder_cases as dc
from golden import decoder_train_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "decoder_train.npz"))


def _check(case, res, fixture):
    keys = sorted(k[len(case) + 1:] for k in fixture.files if k.startswith(case + "/"))
    assert keys == sorted(res), (case, keys, sorted(res))
    for key, t in res.items():
        name = f"{case}/{key}"
        if key.endswith("num_batches_tracked"):
            assert int(t) == int(fixture[name][0]) == 1, name
            continue
        err, big, dsum, dsq = tc.compare(t, fixture[name], tc.salt_of(name))
        tol = TOL * max(1.0, big)
        assert err <= tol and dsum <= tol and dsq <= 2 * tol, (name, err, big, dsum, dsq)


@pytest.mark.parametrize("name", sorted(tc.CONV2X))
def test_conv2x_in_train(fixture, name):
    import semstereo_amd as sa
    Cin, Cout, _ = tc.CONV2X[name]
    mod = dc.fill(sa.modules.Conv2x(Cin, Cout, deconv=True), tc.SALTS[name])
    before = dict(sa.modules.PATH_COUNTS)
    res = tc.run(mod, tc.conv2x_inputs(name), name)
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"] + 2 and sa.modules.PATH_COUNTS["hip"] == before["hip"]
    _check(name, res, fixture)


def test_spx2_in_train(fixture):
    import semstereo_amd as sa
    mod = dc.fill(sa.modules.Spx2(tc.SPX2[0], tc.SPX2[1]), tc.SALTS["spx2"])
    _check("spx2", tc.run(mod, [tc.spx2_input()], "spx2"), fixture)


def test_the_fixture_is_small_and_holds_numbers_only(fixture):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "decoder_train.npz")) < 1 << 20
    assert all(fixture[k].dtype in (np.float64, np.int64) for k in fixture.files)
