"""CPU: the entry points of the 2-D heads (csrc/proj2d_f16s.hip, csrc/seghead_f16s.hip) are declared, bound and exported with
matching arities, and refuse bad arguments before any device call (no GPU needed)."""
import ctypes
import os

from abi import ROOT, declared, library

NAMES = ("ss_conv2d_k1_f16s_fwd", "ss_conv2d_k1_f16s_pair_fwd", "ss_pack_conv2d_k1_weights_f16s", "ss_seghead_logits_fwd",
         "ss_pack_seghead_weights_f16s", "ss_bilinear_up2_fwd")
LL = ctypes.c_longlong


def test_head_entry_points_are_declared_with_the_bindings_arities():
    _l, lib = library()
    decl = {name: len(params) for name, (_, params) in declared().items()}
    for name in NAMES:
        assert name in decl and name in _l._SIGNATURES and name in _l.EXPORTS, name
        assert len(_l._SIGNATURES[name]) == decl[name], (name, len(_l._SIGNATURES[name]), decl[name])
    mk = open(os.path.join(ROOT, "semstereo_amd", "csrc", "Makefile")).read()
    assert "proj2d_f16s.hip" in mk and "seghead_f16s.hip" in mk


def test_the_library_exports_them_and_the_abi_version_is_unchanged():
    _l, lib = library()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.ss_abi_version() == _l.ABI_VERSION == 20


def test_bad_arguments_are_refused_before_any_device_call():
    _l, lib = library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                      # 16-byte aligned host memory that is never followed

    def k1(x=p, w=p, out=p, B=1, Cin=8, npos=16, Cout=8):
        return lib.ss_conv2d_k1_f16s_fwd(x, w, None, None, out, B, Cin, LL(npos), Cout, 1, None)
    assert k1(x=None) == -1 and k1(w=None) == -1 and k1(out=None) == -1
    assert k1(B=0) == -1 and k1(Cin=0) == -1 and k1(npos=0) == -1 and k1(npos=-3) == -1 and k1(Cout=0) == -1 and k1(B=-1) == -1
    assert k1(Cin=12) == -2                                      # whole channel octets only
    assert k1(Cin=1 << 10, npos=1 << 20) == -2 and k1(Cout=1 << 10, npos=1 << 20) == -2     # beyond the 32-bit offsets

    def pair(a=p, b=p, B=1):
        return lib.ss_conv2d_k1_f16s_pair_fwd(a, b, p, None, None, p, B, 8, LL(16), 8, 0, None)
    assert pair(a=None) == -1 and pair(b=None) == -1 and pair(B=0) == -1 and pair(B=1 << 15) == -1
    assert lib.ss_pack_conv2d_k1_weights_f16s(None, p, 8, 8, None) == -1 and lib.ss_pack_conv2d_k1_weights_f16s(p, None, 8, 8, None) == -1
    assert lib.ss_pack_conv2d_k1_weights_f16s(p, p, 0, 8, None) == -1 and lib.ss_pack_conv2d_k1_weights_f16s(p, p, 8, -8, None) == -1

    def head(x=p, w=p, w2=p, bias=p, out=p, B=1, Cin=8, H=4, W=4, K=6):
        return lib.ss_seghead_logits_fwd(x, w, None, None, w2, bias, out, B, Cin, H, W, K, None)
    assert head(x=None) == -1 and head(w=None) == -1 and head(w2=None) == -1 and head(bias=None) == -1 and head(out=None) == -1
    assert head(B=0) == -1 and head(Cin=0) == -1 and head(H=0) == -1 and head(W=-1) == -1 and head(K=0) == -1
    assert head(Cin=20) == -2 and head(K=9) == -2
    assert head(Cin=1 << 10, H=1 << 10, W=1 << 10) == -2         # one sample's input beyond the 32-bit offsets
    assert lib.ss_pack_seghead_weights_f16s(None, p, 8, None) == -1 and lib.ss_pack_seghead_weights_f16s(p, None, 8, None) == -1
    assert lib.ss_pack_seghead_weights_f16s(p, p, 0, None) == -1 and lib.ss_pack_seghead_weights_f16s(p, p, 12, None) == -1

    def up(x=p, out=p, B=1, C=6, H=4, W=4):
        return lib.ss_bilinear_up2_fwd(x, out, B, C, H, W, None)
    assert up(x=None) == -1 and up(out=None) == -1 and up(B=0) == -1 and up(C=0) == -1 and up(H=0) == -1 and up(W=-2) == -1


def test_switch_and_engine_surface():
    import semstereo_amd as sa
    import torch
    import torch.nn as nn
    E = sa.engine
    assert "HEADS_HIP" in E.SWITCHES and E.HEADS_HIP in ("auto", True, False)
    for name in ("pack_conv2d_k1_weight", "run_conv2d_k1", "run_seghead"):
        assert callable(getattr(E, name)), name
    cv, bn, x = nn.Conv2d(8, 8, 1), nn.BatchNorm2d(8), torch.zeros(1, 8, 4, 4)
    assert E.run_conv2d_k1(cv, "k", cv, bn, x, False) is None                     # a CPU tensor: does not apply
    assert E.run_seghead(None, sa.modules.segmenthead(8, 32, 6, 2), x) is None
    import inspect
    assert "heads" in inspect.signature(sa.accelerate).parameters
