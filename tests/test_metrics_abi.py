"""CPU: the evaluation metrics' entry points (csrc/metrics.hip) are declared, bound and exported with matching arities, refuse bad
arguments before any device call, and CPU tensors take the PyTorch composition (no GPU needed)."""
import ctypes
import types

import torch

from abi import declared, library

NAMES = ("ss_metrics_workspace_bytes", "ss_disparity_metrics_fwd", "ss_seg_confusion_fwd")


def test_metric_entry_points_are_declared_bound_and_exported():
    _l, lib = library()
    decl = {name: len(params) for name, (_, params) in declared().items()}
    for name in NAMES:
        assert name in decl and name in _l._SIGNATURES and name in _l.EXPORTS, name
        assert len(_l._SIGNATURES[name]) == decl[name], (name, len(_l._SIGNATURES[name]), decl[name])
        assert hasattr(lib, name), name
    assert _l.ABI_VERSION == 20 and lib.ss_abi_version() == 20          # symbols were added, nothing changed


def test_bad_arguments_are_refused_before_any_device_call():
    _l, lib = library()
    big = 1 << 22
    thr = (1.0, 2.0, 3.0, 4.0)
    assert lib.ss_metrics_workspace_bytes(0, None) == -1
    n = ctypes.c_longlong(0)
    assert lib.ss_metrics_workspace_bytes(2, ctypes.byref(n)) == -1
    assert lib.ss_disparity_metrics_fwd(*([None] * 7), 1, 1, 16, -32.0, 32.0, *thr, 2, None, None, None, None, big, None) == -1
    assert lib.ss_seg_confusion_fwd(None, None, 0, 1, 6, 4, 4, 4, 16, None, 0, None, big, None) == -1
    # bad sizes, with pointers that are never followed
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def disp(n_est=1, B=1, npix=16, n_thr=2, ws=big, est0=p):
        return lib.ss_disparity_metrics_fwd(est0, None, None, None, p, None, None, n_est, B, npix, -32.0, 32.0, *thr, n_thr, p, p, p, p, ws, None)

    def conf(dtype=0, B=1, C=6, H=4, W=4, row=4, img=16, ws=big):
        return lib.ss_seg_confusion_fwd(p, p, dtype, B, C, H, W, row, img, p, 0, p, ws, None)
    assert disp(n_est=0) == -1 and disp(n_est=5) == -1 and disp(n_est=2) == -1          # (the second estimate is NULL)
    assert disp(B=0) == -1 and disp(npix=0) == -1 and disp(n_thr=5) == -1 and disp(n_thr=-1) == -1
    assert disp(ws=8) == -1 and disp(est0=None) == -1
    assert disp(B=100000) == -2                                                          # more images than workgroups: not supported
    assert conf(B=0) == -1 and conf(H=0) == -1 and conf(W=-3) == -1
    assert conf(dtype=7) == -1 and conf(dtype=-1) == -1                                  # unknown label dtype
    assert conf(ws=8) == -1                                                              # workspace too small
    assert conf(row=3) == -1 and conf(img=15) == -1                                      # label strides that would leave the tensor
    assert conf(C=5) == -2                                                               # C != 6: not supported


def test_workspace_query():
    from semstereo_amd import metrics
    for kind in (0, 1):
        assert metrics.workspace_bytes(kind) > 0 and metrics.workspace_bytes(kind) % 4 == 0


def test_cpu_tensors_take_the_pytorch_composition():
    import semstereo_amd as sa
    g = torch.Generator().manual_seed(5)
    gt = 40 * (torch.rand(2, 8, 12, generator=g) - 0.5)
    est = gt + torch.randn(2, 8, 12, generator=g)
    z, y = torch.randn(2, 6, 8, 12, generator=g), torch.randint(0, 6, (2, 8, 12), generator=g)
    mask = gt.abs() < 15
    assert not sa.metrics.supported_disparity([est], gt, mask, None) and not sa.metrics.supported_confusion(z, y)
    assert "METRICS_HIP" in sa.engine.SWITCHES and isinstance(sa.engine.METRICS_HIP, bool)
    before = dict(sa.modules.PATH_COUNTS)
    out, out2 = sa.eval_metrics([est], z, gt, y, 15)
    epe = sa.metrics.EPE_metric(est, gt, mask)
    m = sa.SegmentationMetric(5)
    m.addBatch(z, y)
    assert sa.modules.PATH_COUNTS["metrics_torch"] == before.get("metrics_torch", 0) + 4
    assert sa.modules.PATH_COUNTS.get("metrics_hip", 0) == before.get("metrics_hip", 0)
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"] and sa.modules.PATH_COUNTS["hip"] == before["hip"]
    assert epe.dim() == 0 and torch.equal(epe, out["EPE"][0]) and not epe.requires_grad
    assert float(out["mIoU"][0]) == m.meanIntersectionOverUnion() or abs(float(out["mIoU"][0]) - m.meanIntersectionOverUnion()) < 1e-14
    # the metrics are never differentiable
    assert not sa.metrics.D1_metric(est.clone().requires_grad_(True), gt, mask).requires_grad


def test_shape_assertion_of_the_reference():
    import pytest
    import semstereo_amd as sa
    gt = torch.zeros(2, 4, 4)
    with pytest.raises(AssertionError):
        sa.metrics.EPE_metric(gt[0], gt[0], gt[0] > 0)                     # not [B,H,W]
    with pytest.raises(AssertionError):
        sa.metrics.D1_metric(gt, gt[:1], gt > 0)                           # sizes differ
    with pytest.raises(AssertionError):
        sa.metrics.Thres_metric(gt, gt, gt > -1, torch.tensor(1.0))        # the threshold is a number


def test_install_metrics_rebinds_the_seven_names():
    import semstereo_amd as sa
    script = types.ModuleType("eval_script")
    script.EPE_metric = marker = object()
    previous = sa.install_metrics(script)
    for name in ("EPE_metric", "D1_metric", "Thres_metric", "EPE_metric_mask", "D1_metric_mask", "Thres_metric_mask", "SegmentationMetric"):
        assert getattr(script, name) is getattr(sa.metrics, name)
    sa.uninstall(script, previous)
    assert script.EPE_metric is marker and not hasattr(script, "SegmentationMetric") and not hasattr(script, "D1_metric")
