"""CPU: the image outputs' entry points (csrc/vis.hip) are declared, bound and exported with matching arities, refuse bad arguments
before any device call, CPU tensors take the PyTorch composition with the counters moving as stated, and install_visualization rebinds
the two names of the reference (no GPU needed)."""
import ctypes
import os
import types

import numpy as np
import torch

from abi import ROOT, declared, library

NAMES = ("ss_vis_workspace_bytes", "ss_disp_error_image_fwd", "ss_class_color_fwd", "ss_image_minmax_fwd", "ss_image_normalize_fwd")


def test_vis_entry_points_are_declared_bound_and_exported():
    _l, lib = library()
    decl = {name: len(params) for name, (_, params) in declared().items()}
    for name in NAMES:
        assert name in decl and name in _l._SIGNATURES and name in _l.EXPORTS, name
        assert len(_l._SIGNATURES[name]) == decl[name], (name, len(_l._SIGNATURES[name]), decl[name])
        assert hasattr(lib, name), name
    assert _l.ABI_VERSION == 20 and lib.ss_abi_version() == 20          # symbols were added, nothing changed
    assert "vis.hip" in open(os.path.join(ROOT, "semstereo_amd", "csrc", "Makefile")).read()


def test_bad_arguments_are_refused_before_any_device_call():
    _l, lib = library()
    big = 1 << 22
    n = ctypes.c_longlong(0)
    assert lib.ss_vis_workspace_bytes(0, None) == -1 and lib.ss_vis_workspace_bytes(1, ctypes.byref(n)) == -1
    assert lib.ss_vis_workspace_bytes(0, ctypes.byref(n)) == 0 and n.value > 0 and n.value % 4 == 0
    # pointers that are never followed (the colour table is host memory and IS read: a real one)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    table = np.zeros((10, 5), dtype=np.float32)
    t = table.ctypes.data
    inf = float("inf")

    def err(est=p, gt=p, tab=t, B=1, H=4, W=4, out=p):
        return lib.ss_disp_error_image_fwd(est, gt, tab, B, H, W, 3.0, 0.05, 1, 0, -inf, inf, out, None)

    def col(src=p, dtype=0, B=1, C=6, H=4, W=4, row=4, img=16, out=p, out_dtype=0):
        return lib.ss_class_color_fwd(src, dtype, B, C, H, W, row, img, out, out_dtype, None)

    def mm(x=p, B=1, n=16, out=p, ws=p, ws_bytes=big):
        return lib.ss_image_minmax_fwd(x, B, n, out, ws, ws_bytes, None)

    def norm(x=p, mmx=p, out=p, B=1, C=3, P=16):
        return lib.ss_image_normalize_fwd(x, mmx, out, B, C, P, None)
    assert err(est=None) == -1 and err(gt=None) == -1 and err(tab=None) == -1 and err(out=None) == -1
    assert err(B=0) == -1 and err(H=0) == -1 and err(W=-3) == -1
    assert err(B=1 << 15, H=1 << 15, W=8) == -2                                         # 2^31 four-pixel groups: not supported
    assert col(src=None) == -1 and col(out=None) == -1 and col(B=0) == -1 and col(H=0) == -1 and col(W=0) == -1
    assert col(dtype=3) == -1 and col(dtype=-2) == -1 and col(out_dtype=2) == -1 and col(out_dtype=-1) == -1      # unknown dtype codes
    assert col(row=3) == -1 and col(img=15) == -1                                       # label strides that would leave the tensor
    assert col(dtype=-1, C=0) == -1
    assert col(dtype=-1, C=7) == -2                                                     # more channels than the palette has colours
    assert mm(x=None) == -1 and mm(out=None) == -1 and mm(ws=None) == -1 and mm(B=0) == -1 and mm(n=0) == -1
    assert mm(ws_bytes=8) == -1                                                         # workspace too small
    assert mm(B=100000) == -2                                                           # more images than workgroups
    assert norm(x=None) == -1 and norm(mmx=None) == -1 and norm(out=None) == -1
    assert norm(B=0) == -1 and norm(C=0) == -1 and norm(P=0) == -1


def test_workspace_query():
    from semstereo_amd import visualization as V
    assert V.workspace_bytes() > 0 and V.workspace_bytes() % 4 == 0


def test_cpu_tensors_take_the_pytorch_composition():
    import semstereo_amd as sa
    g = torch.Generator().manual_seed(5)
    gt = 40 * (torch.rand(2, 12, 24, generator=g) - 0.2)
    est = gt + torch.randn(2, 12, 24, generator=g)
    z, y = torch.randn(2, 6, 12, 24, generator=g), torch.randint(0, 6, (2, 12, 24), generator=g)
    img = torch.rand(2, 3, 12, 24, generator=g)
    assert not sa.visualization.supported_error_image(est, gt)
    assert "VIS_HIP" in sa.engine.SWITCHES and isinstance(sa.engine.VIS_HIP, bool)
    before = dict(sa.modules.PATH_COUNTS)

    def moved():
        return sa.modules.PATH_COUNTS.get("vis_torch", 0) - before.get("vis_torch", 0)
    e = sa.disp_error_image_func.apply(est, gt)
    assert moved() == 1 and e.shape == (2, 3, 12, 24) and e.dtype == torch.float32
    assert torch.equal(sa.disp_error_image_func.apply(est, gt, abs_thres=3., rel_thres=0.05), e) and moved() == 2
    assert torch.equal(sa.disp_error_image_func().forward(est, gt, 3., 0.05, 1), e) and moved() == 3
    f = sa.feature_vis(z)
    assert moved() == 4 and isinstance(f, torch.Tensor) and f.dtype == torch.float32 and f.shape == (2, 3, 12, 24)
    assert set(f.unique().tolist()) <= {0.0, 255.0}
    lab = sa.label_vis(y, dtype=torch.uint8)
    assert moved() == 5 and lab.dtype == torch.uint8
    nrm = sa.normalize_image(gt)
    assert moved() == 6 and nrm.shape == (2, 3, 12, 24) and float(nrm.min()) == 0.0 and float(nrm.max()) == 1.0
    out = sa.eval_images([est, est + 1], z, gt, y, imgL=img)                             # first = 1, normalised
    # label, label_est, two error maps, and the normalisation of 2 + 1 + 1 + 1 + 1 + 2 pictures
    assert moved() == 6 + 4 + 8
    assert set(out) == {"disp_est", "disp_gt", "imgL", "label", "label_est", "errormap"}
    assert len(out["disp_est"]) == 2 and len(out["errormap"]) == 2 and len(out["label"]) == 1 and len(out["label_est"]) == 1
    for v in out["disp_est"] + out["errormap"] + out["label"] + out["label_est"] + [out["disp_gt"], out["imgL"]]:
        assert v.shape == (1, 3, 12, 24) and v.dtype == torch.float32 and 0.0 <= float(v.min()) and float(v.max()) <= 1.0
    raw = sa.eval_images([est], z, gt, y, first=None, normalize=False)
    assert raw["disp_est"][0].shape == (2, 12, 24) and raw["errormap"][0].shape == (2, 3, 12, 24) and "imgL" not in raw
    assert torch.equal(raw["label"][0], sa.label_vis(y)) and torch.equal(raw["errormap"][0], e)
    whu = sa.eval_images([est], None, gt, None, imgL=img)                                # main_whu.py:242, :250-251: no labels
    assert set(whu) == {"disp_est", "disp_gt", "imgL", "errormap"}
    assert sa.modules.PATH_COUNTS.get("vis_hip", 0) == before.get("vis_hip", 0)
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"] and sa.modules.PATH_COUNTS["hip"] == before["hip"]
    # the pictures are never differentiable; the reference's host helpers accept them
    assert not sa.disp_error_image_func.apply(est.clone().requires_grad_(True), gt).requires_grad
    assert isinstance(f.data.cpu().numpy(), np.ndarray)


def test_install_visualization_rebinds_the_two_names():
    import semstereo_amd as sa
    script = types.ModuleType("eval_script")
    script.feature_vis = marker = object()
    previous = sa.install_visualization(script)
    assert script.feature_vis is sa.visualization.feature_vis and script.disp_error_image_func is sa.visualization.disp_error_image_func
    gt = torch.full((1, 4, 8), 5.0)
    assert script.disp_error_image_func.apply(gt, gt).shape == (1, 3, 4, 8)              # the call form of main_us3d.py:268
    sa.uninstall(script, previous)
    assert script.feature_vis is marker and not hasattr(script, "disp_error_image_func")
