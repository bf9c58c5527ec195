"""CPU: the objective's entry points (csrc/loss.hip) are declared, bound and exported with matching arities, refuse NULL arguments
before any device call, and CPU tensors take the PyTorch composition (no GPU needed)."""
import ctypes

import torch

from abi import declared, library

NAMES = ("ss_loss_workspace_bytes", "ss_disparity_loss_fwd", "ss_disparity_loss_bwd", "ss_label_loss_fwd", "ss_label_loss_bwd",
         "ss_lrsc_loss_fwd", "ss_lrsc_loss_bwd")


def test_loss_entry_points_are_declared_bound_and_exported():
    _l, lib = library()
    decl = {name: len(params) for name, (_, params) in declared().items()}
    for name in NAMES:
        assert name in decl and name in _l._SIGNATURES and name in _l.EXPORTS, name
        assert len(_l._SIGNATURES[name]) == decl[name], (name, len(_l._SIGNATURES[name]), decl[name])
        assert hasattr(lib, name), name
    assert _l.ABI_VERSION == 20 and lib.ss_abi_version() == 20          # symbols were added, nothing changed


def test_null_arguments_are_refused_before_any_device_call():
    _l, lib = library()
    term = [None, None, None, 16]
    assert lib.ss_disparity_loss_fwd(*(term * 4), 1.0, 0.6, 0.5, 0.3, -32.0, 32.0, 4, 0, None, None, None, 1 << 20, None) == -1
    assert lib.ss_disparity_loss_bwd(*(([None] * 4 + [16]) * 4), 1.0, 0.6, 0.5, 0.3, -32.0, 32.0, 4, 0, None, None, None) == -1
    assert lib.ss_label_loss_fwd(None, None, 0, 1, 6, 4, 4, 5, 2.4, None, None, None, 1 << 20, None) == -1
    assert lib.ss_label_loss_bwd(None, None, 0, 1, 6, 4, 4, 5, 2.4, None, None, None, None) == -1
    assert lib.ss_lrsc_loss_fwd(None, None, None, 0, 1, 6, 4, 4, None, None, None, None, 1 << 20, None) == -1
    assert lib.ss_lrsc_loss_bwd(None, None, None, 0, 1, 6, 4, 4, None, None, None, None) == -1
    assert lib.ss_loss_workspace_bytes(0, None) == -1
    # non-positive sizes and term counts, with pointers that are never followed
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.ss_label_loss_fwd(p, p, 0, 0, 6, 4, 4, 5, 2.4, p, p, p, 1 << 20, None) == -1
    assert lib.ss_label_loss_fwd(p, p, 7, 1, 6, 4, 4, 5, 2.4, p, p, p, 1 << 20, None) == -1          # unknown label dtype
    assert lib.ss_label_loss_fwd(p, p, 0, 1, 6, 4, 4, 5, 2.4, p, p, p, 8, None) == -1                 # workspace too small
    assert lib.ss_label_loss_fwd(p, p, 0, 1, 5, 4, 4, 5, 2.4, p, p, p, 1 << 20, None) == -2           # C != 6: not supported
    assert lib.ss_disparity_loss_fwd(*([p, p, None, 0] * 4), 1.0, 0.6, 0.5, 0.3, -32.0, 32.0, 4, 0, p, p, p, 1 << 20, None) == -1
    assert lib.ss_disparity_loss_fwd(*([p, p, None, 16] * 4), 1.0, 0.6, 0.5, 0.3, -32.0, 32.0, 5, 0, p, p, p, 1 << 20, None) == -1


def test_workspace_query():
    from semstereo_amd import losses
    assert losses.workspace_bytes(0) > 0 and losses.workspace_bytes(1) > 0
    assert losses.workspace_bytes(0) % 8 == 0 and losses.workspace_bytes(1) % 8 == 0


def test_cpu_tensors_take_the_pytorch_composition():
    import semstereo_amd as sa
    g = torch.Generator().manual_seed(3)
    est = [torch.randn(2, 8, 12, generator=g).requires_grad_(True) for _ in range(4)]
    gt = torch.randn(2, 8, 12, generator=g)
    z, zr = (torch.randn(2, 6, 8, 12, generator=g).requires_grad_(True) for _ in range(2))
    y = torch.randint(0, 6, (2, 8, 12), generator=g)
    assert not sa.losses.supported_disparity(est, [gt] * 4, [None] * 4)
    assert not sa.losses.supported_labels(z, y) and not sa.losses.supported_labels(zr, y, est[0])
    before = dict(sa.modules.PATH_COUNTS)
    loss, dl, ll, rl = sa.train_objective(est, z, zr, gt, gt, y, 2, False)
    loss.backward()
    assert sa.modules.PATH_COUNTS["loss_torch"] == before.get("loss_torch", 0) + 3
    assert sa.modules.PATH_COUNTS.get("loss_hip", 0) == before.get("loss_hip", 0)
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"] and sa.modules.PATH_COUNTS["hip"] == before["hip"]
    assert loss.dim() == 0 and all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in est + [z, zr])


def test_install_losses_rebinds_the_four_names():
    import types
    import semstereo_amd as sa
    script = types.ModuleType("train_script")
    script.model_loss_train = marker = object()
    previous = sa.install_losses(script)
    for name in ("model_loss_train", "model_loss_test", "model_label_loss", "LRSC_loss"):
        assert getattr(script, name) is getattr(sa.losses, name)
    sa.uninstall(script, previous)
    assert script.model_loss_train is marker and not hasattr(script, "LRSC_loss")
