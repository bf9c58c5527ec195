"""The evaluation step's image outputs on the HIP kernels (csrc/vis.hip; reference utils/visualization.py, utils/mask_vis.py,
utils/experiment.py:84-99): every fixture case against the reference's record (tests/golden/vis.npz), larger inputs against the PyTorch
composition, the normalisation against its stated fp32 formula, eval_images, repeatability, routing and no host wait.
Run on the MI355X box: pytest -m gpu.

Bounds: none, every comparison is torch.equal.  The error map is a choice among ten float32 colours by comparisons of a float32 number
that the kernel forms with IEEE subtraction and division in the reference's order; the class colours are integers; fp32 min and max do
not depend on the order of the reduction, and clamp, subtraction and division are IEEE.  A mismatch is a bug in the arithmetic (an
approximate division, a fused operation), not a tolerance to widen.  The compositions that the kernels are compared with run on the CPU,
whose division is IEEE.

No host wait: the calls run under torch.cuda.set_sync_debug_mode("error"), which raises on a synchronising call of torch; the library's
own launches are outside its view, and csrc/vis.hip holds no synchronising or copying call (its entry points only launch)."""
import os
import types

import numpy as np
import pytest
import torch

from golden import vis_cases as vc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return semstereo_amd


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "vis.npz"))


def _error_inputs(B, H, W, seed):
    """est, gt on the CPU: a fifth of the ground truth not valid, the error measure log-uniform over 2^-6 .. 2^6 (all ten colours), a
    sprinkling of NaN, inf and zero."""
    g = torch.Generator().manual_seed(seed)
    gt = 60 * (torch.rand(B, H, W, generator=g) - 0.2)
    t = torch.exp2(12 * torch.rand(B, H, W, generator=g) - 6)
    sign = torch.where(torch.rand(B, H, W, generator=g) < 0.5, -1.0, 1.0)
    est = gt + sign * t * torch.clamp(0.05 * gt.abs(), min=3.0)
    flat_e, flat_g = est.view(-1), gt.view(-1)
    n = flat_e.numel()
    flat_e[torch.arange(7, n, 1009)] = float("nan")
    flat_e[torch.arange(11, n, 1013)] = float("inf")
    flat_g[torch.arange(13, n, 1019)] = float("nan")
    flat_g[torch.arange(17, n, 1021)] = 0.0
    return est, gt


@pytest.fixture(scope="module")
def big():
    """The 4 x 1024 x 1024 inputs (two trips of the grid-stride loop) with the composition's pictures, computed once on the CPU."""
    from semstereo_amd import visualization as V
    est, gt = _error_inputs(4, 1024, 1024, 4100)
    g = torch.Generator().manual_seed(4101)
    z = 4 * (torch.rand(4, 6, 1024, 1024, generator=g) - 0.5)
    z[:, 2, ::7, ::5] = z[:, 4, ::7, ::5]                              # ties
    z[:, 3, ::11, ::3] = float("nan")
    y = torch.randint(-1, 8, (4, 1024, 1024), generator=g)              # classes 0..5 and labels outside
    return {"est": est, "gt": gt, "z": z, "y": y, "err": V.disp_error_image_func.apply(est, gt), "feat": V.feature_vis(z),
            "lab": V.label_vis(y, dtype=torch.uint8)}


class counted:
    """The calls inside make `hip` pictures on the kernels and `torch_` on the composition."""

    def __init__(self, sa, hip, torch_=0):
        self.sa, self.hip, self.torch = sa, hip, torch_

    def __enter__(self):
        self.before = dict(self.sa.modules.PATH_COUNTS)

    def __exit__(self, *exc):
        if exc[0] is None:
            torch.cuda.synchronize()
            pc = self.sa.modules.PATH_COUNTS
            assert pc.get("vis_hip", 0) == self.before.get("vis_hip", 0) + self.hip, "vis_hip"
            assert pc.get("vis_torch", 0) == self.before.get("vis_torch", 0) + self.torch, "vis_torch"
            assert pc["hip"] == self.before["hip"] and pc["torch"] == self.before["torch"]


def same(got, want, what):
    assert got.is_cuda and got.dtype == want.dtype and got.shape == want.shape, what
    got = got.cpu()
    assert torch.equal(got, want), f"{what}: {(got != want).sum().item()} of {want.numel()} values differ"


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(vc.ERROR_CASES))
def test_fixture_cases_error_map(sa, fx, name):
    d = vc.error_inputs(name)
    with counted(sa, 1):
        got = sa.disp_error_image_func.apply(d["est"].cuda(), d["gt"].cuda())
    same(got, torch.from_numpy(fx[f"err/{name}"]), name)


@pytest.mark.parametrize("name", list(vc.LOGIT_CASES))
def test_fixture_cases_feature_vis(sa, fx, name):
    z = vc.logit_inputs(name)["logits"].cuda()
    with counted(sa, 2):
        got, got8 = sa.feature_vis(z), sa.feature_vis(z, dtype=torch.uint8)
    assert np.array_equal(got.cpu().numpy().astype(np.float64), fx[f"logits/{name}"].astype(np.float64))      # the reference returns float64
    same(got8, torch.from_numpy(fx[f"logits/{name}"]), name)


@pytest.mark.parametrize("name", list(vc.LABEL_CASES))
def test_fixture_cases_label_vis(sa, fx, name):
    d = vc.label_inputs(name)
    big = d["labels"]._base if d["labels"]._base is not None else d["labels"]
    c = vc.LABEL_CASES[name]
    y = big.cuda()[:, :c["H"], :c["W"]]                                # the cropped view, not a copy of it
    assert y.dtype == c["dtype"] and y.is_contiguous() == (c["pad"] == (0, 0))
    want = torch.from_numpy(fx[f"labels/{name}"])
    with counted(sa, 3):
        same(sa.label_vis(y, dtype=torch.uint8), want, name)
        same(sa.label_vis(y), want.float(), name)
        same(sa.label_vis(y[:1]), want[:1].float(), name + " first image")
    with counted(sa, 2):                                               # other dtypes and layouts are converted, not refused
        same(sa.label_vis(y.to(torch.int32)), want.float(), name + " int32")
        same(sa.label_vis(y.transpose(1, 2)), want.float().transpose(2, 3).contiguous(), name + " transposed")


def test_labels_outside_are_black(sa):
    from semstereo_amd import visualization as V
    y = torch.tensor([[[0, 5, 6, -1, 255, 3, 2 ** 40, -2 ** 40 + 1, 4]]])
    f = torch.tensor([[[float("nan"), -0.5, 5.99, 6.0, -1.0, float("inf"), float("-inf"), 1e30, 2.0]]])
    for t in (y, f, y.clamp(0, 255).to(torch.uint8)):
        same(sa.label_vis(t.cuda()), V.label_vis(t), str(t.dtype))


# 2 ------------------------------------------------------------------------------------------------------------------------------
def test_full_size_equals_the_composition(sa, big):
    with counted(sa, 3):
        err = sa.disp_error_image_func.apply(big["est"].cuda(), big["gt"].cuda())
        feat = sa.feature_vis(big["z"].cuda())
        lab = sa.label_vis(big["y"].cuda(), dtype=torch.uint8)
    same(err, big["err"], "error map 4x1024x1024")
    same(feat, big["feat"], "feature_vis 4x6x1024x1024")
    same(lab, big["lab"], "label_vis 4x1024x1024")
    assert len(torch.unique(big["err"].view(4, 3, -1)[:, 0])) == 11    # black and all ten colours are there


def test_element_offsets_past_32_bits(sa):
    """A picture of more than 2^31 floats and logits of more than 2^31 floats: the images of the batch are copies of one image, so every
    image of the result must equal the first, and the first the composition's."""
    from semstereo_amd import visualization as V
    H = W = 2048
    est, gt = _error_inputs(1, H, W, 4150)
    B = 180
    assert 3 * B * H * W > 2 ** 31
    with counted(sa, 1):
        err = sa.disp_error_image_func.apply(est.cuda().expand(B, H, W).contiguous(), gt.cuda().expand(B, H, W).contiguous())
    same(err[:1], V.disp_error_image_func.apply(est, gt), "image 0 of 180")
    assert bool((err.view(B, -1) == err[0].view(1, -1)).all()), "an image past the 32-bit offsets differs from image 0"
    del err
    z = 4 * (torch.rand(1, 6, H, W, generator=torch.Generator().manual_seed(4151)) - 0.5)
    B = 90
    assert 6 * B * H * W > 2 ** 31
    with counted(sa, 1):
        feat = sa.feature_vis(z.cuda().expand(B, 6, H, W).contiguous(), dtype=torch.uint8)
    same(feat[:1], V.feature_vis(z, dtype=torch.uint8), "image 0 of 90")
    assert bool((feat.view(B, -1) == feat[0].view(1, -1)).all()), "an image past the 32-bit offsets differs from image 0"


def test_without_the_legend_equals_the_composition(sa):
    from semstereo_amd import visualization as V
    est, gt = _error_inputs(2, 37, 205, 4200)
    with counted(sa, 1):
        got = sa.disp_error_image_func.apply(est.cuda(), gt.cuda(), legend=False)
    same(got, V.disp_error_image_func.apply(est, gt, legend=False), "legend=0")
    assert not torch.equal(got.cpu(), V.disp_error_image_func.apply(est, gt))


def test_signed_equals_the_composition(sa):
    from semstereo_amd import visualization as V
    est, gt = _error_inputs(2, 37, 205, 4300)
    gt = torch.where(torch.rand(gt.shape, generator=torch.Generator().manual_seed(1)) < 0.5, -gt, gt)        # both signs
    for kw in (dict(signed=True), dict(signed=True, valid_range=(-30.0, 30.0)), dict(signed=True, abs_thres=1.0, rel_thres=0.1)):
        with counted(sa, 1):
            got = sa.disp_error_image_func.apply(est.cuda(), gt.cuda(), **kw)
        same(got, V.disp_error_image_func.apply(est, gt, **kw), str(kw))
    neg = (gt < 0) & (gt >= -30)
    assert bool((got.cpu().sum(1)[:, 10:][neg[:, 10:]] > 0).any())     # a negative ground truth gets a colour


def test_uint8_output_equals_the_composition(sa):
    from semstereo_amd import visualization as V
    g = torch.Generator().manual_seed(4400)
    z = torch.randn(3, 5, 75, 203, generator=g)
    y = torch.randint(0, 7, (3, 75, 203), generator=g).to(torch.uint8)
    with counted(sa, 2):
        a, b = sa.feature_vis(z.cuda(), dtype=torch.uint8), sa.label_vis(y.cuda(), dtype=torch.uint8)
    same(a, V.feature_vis(z, dtype=torch.uint8), "feature_vis uint8, five channels")
    same(b, V.label_vis(y, dtype=torch.uint8), "label_vis uint8")


def test_views_are_made_contiguous_not_misread(sa):
    from semstereo_amd import visualization as V
    est, gt = _error_inputs(2, 40, 64, 4500)
    same(sa.disp_error_image_func.apply(est.cuda().transpose(1, 2), gt.cuda().transpose(1, 2)),
         V.disp_error_image_func.apply(est.transpose(1, 2), gt.transpose(1, 2)), "transposed")
    same(sa.disp_error_image_func.apply(est.cuda()[:, 3:, 1:], gt.cuda()[:, 3:, 1:]),
         V.disp_error_image_func.apply(est[:, 3:, 1:], gt[:, 3:, 1:]), "cropped")


# 3 ------------------------------------------------------------------------------------------------------------------------------
def _normalize_fp32(x):
    """The stated formula from stock calls: per image amin / amax, clamp, sub, div, all fp32; one channel -> three equal ones."""
    if x.dim() == 3:
        x = x.unsqueeze(1)
    B = x.shape[0]
    lo, hi = x.reshape(B, -1).amin(1).view(B, 1, 1, 1), x.reshape(B, -1).amax(1).view(B, 1, 1, 1)
    out = torch.div(torch.sub(torch.clamp(x, lo, hi), lo), torch.clamp(hi - lo, min=1e-5))
    return out.expand(B, 3, *x.shape[2:]).contiguous() if x.shape[1] == 1 else out


@pytest.mark.parametrize("shape", [(1, 1, 23, 41), (2, 3, 75, 203), (1, 3, 1024, 1024)])
def test_normalize_image_equals_the_fp32_formula(sa, shape):
    g = torch.Generator().manual_seed(4600 + shape[-1])
    x = 200 * torch.rand(*shape, generator=g) - 70
    with counted(sa, 1):
        got = sa.normalize_image(x.cuda())
    same(got, _normalize_fp32(x), f"normalize {shape}")
    assert float(got.min()) == 0.0 and float(got.max()) == 1.0 and got.shape[1] == 3


def test_normalize_image_constant_picture_and_three_dims(sa):
    flat = torch.full((2, 3, 23, 41), 2.5)
    flat[1] = -7.0
    same(sa.normalize_image(flat.cuda()), _normalize_fp32(flat), "constant: the 1e-5 floor")
    assert not sa.normalize_image(flat.cuda()).any()
    x = torch.rand(2, 23, 41, generator=torch.Generator().manual_seed(4700)) * 1e-6         # a range below the floor
    same(sa.normalize_image(x.cuda()), _normalize_fp32(x), "[B,H,W], range below 1e-5")


# 4 ------------------------------------------------------------------------------------------------------------------------------
def _eval_inputs(B=3, H=75, W=203, seed=4800):
    est, gt = _error_inputs(B, H, W, seed)
    est, gt = torch.nan_to_num(est, 1.0, 2.0, 3.0), torch.nan_to_num(gt, 1.0, 2.0, 3.0)    # finite: the pictures are normalised
    g = torch.Generator().manual_seed(seed + 1)
    return dict(ests=[est.cuda(), (est + 0.5).cuda()], z=torch.randn(B, 6, H, W, generator=g).cuda(), gt=gt.cuda(),
                y=torch.randint(0, 6, (B, H, W), generator=g).cuda(), img=torch.rand(B, 3, H, W, generator=g).cuda())


def _flat(d):
    return [(k, i, t) for k, v in d.items() for i, t in enumerate(v if isinstance(v, list) else [v])]


def test_eval_images_first_one_is_the_first_of_the_batch(sa):
    d = _eval_inputs()
    with counted(sa, 4 + 8):           # label, label_est, two error maps; eight normalisations
        one = sa.eval_images(d["ests"], d["z"], d["gt"], d["y"], imgL=d["img"])
    whole = sa.eval_images(d["ests"], d["z"], d["gt"], d["y"], imgL=d["img"], first=None)
    assert set(one) == {"disp_est", "disp_gt", "imgL", "label", "label_est", "errormap"} and len(one["errormap"]) == 2
    for (k, i, a), (_, _, b) in zip(_flat(one), _flat(whole)):
        assert a.shape == (1, 3, 75, 203) and b.shape == (3, 3, 75, 203) and a.is_cuda, k
        assert torch.equal(a, b[:1]), (k, i)
    raw = sa.eval_images(d["ests"], d["z"], d["gt"], d["y"], first=2, normalize=False)
    assert raw["disp_est"][0].shape == (2, 75, 203) and raw["label"][0].shape == (2, 3, 75, 203) and "imgL" not in raw
    from semstereo_amd import visualization as V
    same(raw["errormap"][1], V.disp_error_image_func.apply(d["ests"][1][:2].cpu(), d["gt"][:2].cpu()), "errormap of the second estimate")
    same(one["label_est"][0], _normalize_fp32(V.feature_vis(d["z"][:1].cpu())), "label_est, normalised")


def test_two_calls_give_the_same_bits(sa):
    d = _eval_inputs(2, 64, 96, 4900)
    a = sa.eval_images(d["ests"], d["z"], d["gt"], d["y"], imgL=d["img"], first=None)
    b = sa.eval_images(d["ests"], d["z"], d["gt"], d["y"], imgL=d["img"], first=None)
    for (k, i, s), (_, _, t) in zip(_flat(a), _flat(b)):
        assert torch.equal(s, t), (k, i)
    # outside the contract: non-finite pictures must not fault and must give the same bits twice (compared as integers: NaN != NaN)
    x = d["img"].clone()
    x[0, 0, 0, :5] = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0, 1.0])
    x[1] = float("nan")
    p, q = sa.normalize_image(x), sa.normalize_image(x)
    torch.cuda.synchronize()
    assert torch.equal(p.view(torch.int32), q.view(torch.int32))


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_routing(sa, monkeypatch):
    d = _eval_inputs(2, 23, 41, 5000)
    with counted(sa, 4):
        on = sa.eval_images(d["ests"], d["z"], d["gt"], d["y"], imgL=d["img"], normalize=False)
    monkeypatch.setattr(sa.engine, "VIS_HIP", False)
    with counted(sa, 0, 4 + 4 + 8):
        off = sa.eval_images(d["ests"], d["z"], d["gt"], d["y"], imgL=d["img"], normalize=False)
        nrm = sa.eval_images(d["ests"], d["z"], d["gt"], d["y"], imgL=d["img"], normalize=True)
    monkeypatch.setattr(sa.engine, "VIS_HIP", True)
    assert all(t.is_cuda and t.shape == (1, 3, 23, 41) for _, _, t in _flat(nrm))
    for (k, i, a), (_, _, b) in zip(_flat(on), _flat(off)):
        assert b.is_cuda and a.shape == b.shape and a.dtype == b.dtype, k
        if k in ("label", "label_est"):                               # integers: the same on any path and device
            assert torch.equal(a, b), k
    with counted(sa, 0, 3):                                            # float64 and more than six channels keep the composition
        sa.disp_error_image_func.apply(d["ests"][0].double(), d["gt"].double())
        sa.feature_vis(torch.randn(1, 8, 9, 9, device="cuda"))
        sa.normalize_image(d["img"].double())


def test_no_host_wait(sa):
    d = _eval_inputs(2, 64, 96, 5100)

    def step():
        return sa.eval_images(d["ests"], d["z"], d["gt"], d["y"], imgL=d["img"])
    step()                                                             # (library load, workspace query)
    torch.cuda.synchronize()
    with counted(sa, 4 + 8):
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(out["errormap"][0]).all())


# 6 ------------------------------------------------------------------------------------------------------------------------------
_SCRIPT = '''
import torch
import torch.nn.functional as F

def image_outputs(disp_ests, label_est, disp_gt, label_true, nums=6):
    out = {}
    out["label"] = [feature_vis(F.one_hot(label_true.to(torch.int64), nums).permute(0, 3, 1, 2).float())]
    out["label_est"] = [feature_vis(label_est)]
    out["errormap"] = [disp_error_image_func.apply(disp_est, disp_gt) for disp_est in disp_ests]
    return out
'''


def test_install_visualization_on_a_stand_in_script(sa):
    script = types.ModuleType("standin_eval_script")
    exec(_SCRIPT, script.__dict__)
    previous = sa.install_visualization(script)
    try:
        d = _eval_inputs(2, 23, 41, 5200)
        with counted(sa, 4):
            out = script.image_outputs(d["ests"], d["z"], d["gt"], d["y"])
        ours = sa.eval_images(d["ests"], d["z"], d["gt"], d["y"], first=None, normalize=False)
        for k in out:
            for a, b in zip(out[k], ours[k]):
                assert a.is_cuda and torch.equal(a, b), k
    finally:
        sa.uninstall(script, previous)
    assert not hasattr(script, "feature_vis")
