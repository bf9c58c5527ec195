"""CPU: the SSR_upsample training entry points (csrc/ssr_upsample_train.hip) are declared, bound and exported with matching arities,
and CPU tensors keep the PyTorch composition (no GPU needed)."""
import torch

from abi import declared, library

NAMES = ("ss_ssr_upsample_train_fwd", "ss_ssr_upsample_train_bwd")


def test_training_entry_points_are_declared_bound_and_exported():
    _lib, lib = library()
    decl = {name: len(params) for name, (_, params) in declared().items()}
    for name in NAMES:
        assert name in decl and name in _lib._SIGNATURES and name in _lib.EXPORTS, name
        assert len(_lib._SIGNATURES[name]) == decl[name], (name, len(_lib._SIGNATURES[name]), decl[name])
        assert hasattr(lib, name), name
    assert _lib.ABI_VERSION == 20 and lib.ss_abi_version() == 20
    # NULL inputs are refused before anything touches a device
    assert lib.ss_ssr_upsample_train_fwd(*([None] * 18), 1e-5, 1e-5, 1e-5, 1e-5, 0.1, 0.1, 0.1, 0.1, 1, 1, 1, 1, 6, None, 0, None) == -1
    assert lib.ss_ssr_upsample_train_bwd(*([None] * 10), 1, 1, 1, 1, 6, None, 0, None) == -1


def test_cpu_tensors_keep_the_pytorch_path():
    import semstereo_amd as sa
    from oracle import ssr as ossr
    mod = sa.modules.SSR_upsample(6)
    P = ossr.deterministic_ssr_params()
    mod.load_state_dict({k[len("ssr_upsample."):]: v for k, v in P.items()}, strict=False)
    mod.train()
    g = torch.Generator().manual_seed(5)
    d = torch.randn(2, 1, 3, 5, generator=g).requires_grad_(True)
    wt, lab = torch.rand(2, 6, 12, 20, generator=g), torch.randn(2, 6, 12, 20, generator=g)
    before = dict(sa.modules.PATH_COUNTS)
    mod(d, wt, lab).sum().backward()
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"] + 1
    assert sa.modules.PATH_COUNTS.get("ssr_train", 0) == before.get("ssr_train", 0)
    assert not sa.train_ssr.supported(mod, d, wt, lab)
    sa.modules.drop_parked_gates(mod)
