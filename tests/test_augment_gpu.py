"""augment_sample on the HIP kernels (csrc/augment.hip): every case of tests/augment_cases.py against the PyTorch composition (computed
once on the CPU, where tests/test_augment.py holds it against the per-pixel restatement), the identity against prepare_sample, the
reference's recorded items, repeatability, the switch and DeviceLoader(augment=...).  Run on the MI355X box: pytest -m gpu.

Every comparison is torch.equal: table lookups, selections, exact integer sums and one non-contracted fp32 blend, so no tolerance appears."""
import os
import subprocess
import sys

import pytest
import torch

import augment_cases as ac
import test_augment_golden as tg
from golden import augment_cases as gc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return semstereo_amd


class counted:
    """The calls inside make `hip` calls on the kernels and `torch_` on the composition."""

    def __init__(self, sa, hip, torch_=0):
        self.sa, self.hip, self.torch = sa, hip, torch_

    def __enter__(self):
        self.before = dict(self.sa.modules.PATH_COUNTS)

    def __exit__(self, *exc):
        if exc[0] is None:
            torch.cuda.synchronize()
            pc = self.sa.modules.PATH_COUNTS
            assert pc.get("augment_hip", 0) == self.before.get("augment_hip", 0) + self.hip, "augment_hip"
            assert pc.get("augment_torch", 0) == self.before.get("augment_torch", 0) + self.torch, "augment_torch"
            assert pc["hip"] == self.before["hip"] and pc["torch"] == self.before["torch"]


def cuda(raw):
    return {k: v.cuda() for k, v in raw.items()}


def same(got, want, what):
    assert tuple(got) == tuple(want), what
    for k in want:
        assert got[k].is_cuda and got[k].dtype == want[k].dtype and torch.equal(got[k].cpu(), want[k].cpu()), (what, k)


# 1 - 6 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ac.GPU_CASES)
def test_cases_equal_the_composition(sa, name):
    c = ac.CASES[name]
    with counted(sa, 1):
        got = sa.augment_sample(cuda(ac.raw_of(name)), ac.params_of(name), c["keys"], maxdisp=c["maxdisp"])
    same(got, ac.composed(name), name)


def test_more_than_one_partial_per_image_is_added():
    """`several_workgroups`: 96 x 128 pixels are 3072 lane-trips of 4 pixels, 12 workgroups of 256 lanes, under the cap min(1024,
    2048 // (2 B)) = 512 of the grid rule -- so the mean of every (item, view) is the sum of 12 partials, and the occluder's colour of 12."""
    c = ac.CASES["several_workgroups"]
    assert ac.partials_per_image(*c["image"], c["B"]) == 12


def test_identity_equals_prepare_sample(sa):
    raw, B = ac.raw_of("levels_odd_origin"), 3                                  # 40 x 52, padded to 48 x 64 for the levels
    big = cuda({k: torch.nn.functional.pad(v, (0, 0, 4, 8, 0, 8) if v.dim() == 4 else (4, 8, 0, 8)).contiguous() for k, v in raw.items()})
    with counted(sa, 1):
        got = sa.augment_sample(big, sa.AugmentParams((48, 64), (48, 64), [(0, 0)] * B), ac.NINE)
    same(got, sa.prepare_sample(big, True, ac.NINE), "identity")


# the reference's own items -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(gc.CASES))
def test_kernel_equals_the_reference(sa, name):
    with counted(sa, 1):
        got = sa.augment_sample(cuda(gc.raw_of(name)), gc.params_of(name, tg.arrays()), tg.keys_of(name))
    tg.check(name, got)


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_raw_is_untouched(sa):
    name = "levels_odd_origin"
    c, raw = ac.CASES[name], cuda(ac.raw_of(name))
    before = {k: v.clone() for k, v in raw.items()}
    P = ac.params_of(name)
    with counted(sa, 2):
        a = sa.augment_sample(raw, P, c["keys"], maxdisp=c["maxdisp"])
        b = sa.augment_sample(raw, P, c["keys"], maxdisp=c["maxdisp"])
    same(a, b, "second call")
    assert all(torch.equal(raw[k], before[k]) for k in raw)
    with counted(sa, 2):                                                        # each half alone: a NULL output is skipped
        views = sa.augment_sample(raw, P, ("right",))
        maps = sa.augment_sample(raw, P, ("label_4", "disparity"), maxdisp=c["maxdisp"])
    same(views, {"right": a["right"]}, "right alone")
    same(maps, {"disparity": a["disparity"], "label_4": a["label_4"]}, "two maps alone")


# 8 ------------------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import os, sys, torch
sys.path[:0] = [os.environ["SS_ROOT"], os.path.join(os.environ["SS_ROOT"], "tests")]
import semstereo_amd as sa, augment_cases as ac
assert sa.engine.AUGMENT_HIP is False
name = "levels_odd_origin"
c = ac.CASES[name]
before = dict(sa.modules.PATH_COUNTS)
got = sa.augment_sample({k: v.cuda() for k, v in ac.raw_of(name).items()}, ac.params_of(name), c["keys"], maxdisp=c["maxdisp"])
torch.cuda.synchronize()
pc = sa.modules.PATH_COUNTS
assert pc.get("augment_torch", 0) == before.get("augment_torch", 0) + 1 and pc.get("augment_hip", 0) == before.get("augment_hip", 0)
want = ac.composed(name)
assert tuple(got) == tuple(want) and all(v.is_cuda and torch.equal(v.cpu(), want[k]) for k, v in got.items())
print("RESULT ok")
"""


def test_switch_off_takes_the_composition_on_the_device():
    env = dict(os.environ, SS_AUGMENT_HIP="0", SS_ROOT=ROOT)
    p = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "RESULT ok" in p.stdout, (p.stdout + p.stderr)[-4000:]


# 9 ------------------------------------------------------------------------------------------------------------------------------
def test_device_loader_augments_on_the_device(sa):
    keys = ("left", "right", "disparity", "disparity_4", "label")
    batches = [ac.raw_of("levels_odd_origin"), ac.raw_of("levels_odd_origin")]
    make = lambda: sa.Augmentation.us3d((32, 48), 12, p_occluder=0.5, occluder_rows=(3, 9), occluder_cols=(3, 9), seed=3)    # noqa: E731
    with counted(sa, 2):
        out = list(sa.DeviceLoader(batches, device="cuda", keys=keys, training=True, augment=make()))
    draws = make()
    assert len(out) == 2
    for got, raw in zip(out, batches):
        P = draws.draw(3, 40, 52)
        same(got, sa.augment_sample(raw, P, keys, maxdisp=12), "loader")        # (CPU tensors: the composition)
    assert not torch.equal(out[0]["left"], out[1]["left"])                      # two draws
