"""CPU: the joint-metrics entry points (csrc/joint_metrics.hip) are declared, bound and exported with matching arities, refuse bad
arguments before any device call, and CPU tensors take the PyTorch composition (no GPU needed)."""
import ctypes

import torch

from abi import declared, library

NAMES = ("ss_joint_metrics_scratch", "ss_joint_metrics_fwd")


def test_entry_points_are_declared_bound_and_exported():
    _l, lib = library()
    decl = {name: len(params) for name, (_, params) in declared().items()}
    for name in NAMES:
        assert name in decl and name in _l._SIGNATURES and name in _l.EXPORTS, name
        assert len(_l._SIGNATURES[name]) == decl[name], (name, len(_l._SIGNATURES[name]), decl[name])
        assert hasattr(lib, name), name
    assert decl["ss_joint_metrics_scratch"] == 3 and decl["ss_joint_metrics_fwd"] == 34
    assert not any(name.endswith("_workspace_bytes") for name in NAMES)
    assert _l.ABI_VERSION == 20 and lib.ss_abi_version() == 20          # symbols were added, nothing changed


def test_scratch_query():
    _l, lib = library()
    n = ctypes.c_longlong(0)
    assert lib.ss_joint_metrics_scratch(1, 1, None) == -1
    for n_est, B in ((0, 1), (5, 1), (1, 0), (1, -2)):
        assert lib.ss_joint_metrics_scratch(n_est, B, ctypes.byref(n)) == -1, (n_est, B)
    assert lib.ss_joint_metrics_scratch(1, 100000, ctypes.byref(n)) == -2               # more images than workgroups
    sizes = []
    for n_est in (1, 2, 3, 4):
        assert lib.ss_joint_metrics_scratch(n_est, 4, ctypes.byref(n)) == 0
        sizes.append(n.value)
    assert sizes[0] > 0 and sizes == sorted(sizes) and all(s % 8 == 0 for s in sizes)
    from semstereo_amd import joint_metrics as jm
    assert jm.scratch_bytes(4, 4) == sizes[3]
    assert lib.ss_metrics_workspace_bytes(2, ctypes.byref(n)) == -1                     # the older query knows no third kind


def test_bad_arguments_are_refused_before_any_device_call():
    _l, lib = library()
    big = 1 << 22
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                                # pointers that are never followed

    def fwd(est0=p, est1=None, gt=p, logits=p, labels=p, dtype=0, row=4, img=16, n_est=1, B=1, C=6, H=4, W=4, n_thr=2, out=p, joint=p,
            ws=p, ws_bytes=big):
        return lib.ss_joint_metrics_fwd(est0, est1, None, None, gt, None, logits, labels, dtype, row, img, n_est, B, C, H, W, -32.0, 32.0,
                                        1.0, 2.0, 3.0, 4.0, n_thr, 3.0, out, out, out, out, joint, joint, joint, ws, ws_bytes, None)
    assert lib.ss_joint_metrics_fwd(*([None] * 8), 0, 4, 16, 1, 1, 6, 4, 4, -32.0, 32.0, 1.0, 2.0, 3.0, 4.0, 2, 3.0, *([None] * 8),
                                    big, None) == -1
    assert fwd(est0=None) == -1 and fwd(gt=None) == -1 and fwd(labels=None) == -1 and fwd(out=None) == -1 and fwd(ws=None) == -1
    assert fwd(joint=None) == -1                                         # logits without the tables they fill
    assert fwd(n_est=0) == -1 and fwd(n_est=5) == -1 and fwd(n_est=2) == -1              # (the second estimate is NULL)
    assert fwd(n_thr=-1) == -1 and fwd(n_thr=5) == -1
    assert fwd(B=0) == -1 and fwd(H=0) == -1 and fwd(W=-3) == -1
    assert fwd(row=3) == -1 and fwd(img=15) == -1                        # label strides that would leave the tensor
    assert fwd(dtype=7) == -1 and fwd(dtype=-1) == -1                    # unknown label dtype
    assert fwd(ws_bytes=8) == -1                                         # workspace too small
    assert fwd(C=5) == -2                                                # C != 6: not supported
    assert fwd(B=100000, img=16) == -2                                   # more images than workgroups
    assert fwd(H=65536, W=32768, row=32768, img=65536 * 32768) == -2     # 2^31 pixels in an image


def test_cpu_tensors_take_the_composition_and_move_only_the_new_counters():
    import semstereo_amd as sa
    g = torch.Generator().manual_seed(5)
    gt = 40 * (torch.rand(2, 8, 12, generator=g) - 0.5)
    est = gt + torch.randn(2, 8, 12, generator=g)
    z, y = torch.randn(2, 6, 8, 12, generator=g), torch.randint(0, 6, (2, 8, 12), generator=g)
    assert not sa.joint_metrics.supported_joint([est], z, gt, y, None)
    assert "JOINT_METRICS_HIP" in sa.engine.SWITCHES and isinstance(sa.engine.JOINT_METRICS_HIP, bool)
    before = dict(sa.modules.PATH_COUNTS)
    rec = sa.joint_metrics.joint_metrics([est.clone().requires_grad_(True)], z.clone().requires_grad_(True), gt, y, maxdisp=15)
    m = sa.JointMetric()
    m.addBatch([est], z, gt, y, maxdisp=15)
    out = sa.eval_metrics_joint([est], z, gt, y, 15)
    after = sa.modules.PATH_COUNTS
    assert after["joint_metrics_torch"] == before.get("joint_metrics_torch", 0) + 3
    assert after.get("joint_metrics_hip", 0) == before.get("joint_metrics_hip", 0)
    assert {k: v for k, v in after.items() if not k.startswith("joint_metrics")} == \
        {k: v for k, v in before.items() if not k.startswith("joint_metrics")}
    assert all(not v.requires_grad for v in rec.values()) and all(not v.requires_grad for v in m.scores().values())
    assert rec["cls_sums"].dtype == torch.float64 and all(rec[k].dtype == torch.int64 for k in rec if k != "cls_sums")
    assert list(out)[0] == "mIoU3" and all(t.dim() == 0 and not t.requires_grad for v in out.values() for t in v)
    none = sa.joint_metrics.joint_metrics([est], None, gt, y, maxdisp=15)               # no logits: no joint tables
    assert none["joint_all"] is None and none["joint_good"] is None and torch.equal(none["cls_counts"], rec["cls_counts"])
