"""CPU: the 2-D decoder's entry points (csrc/deconv2d_bf16s.hip, the concat-free form in csrc/conv3d_bf16s.hip) are declared, bound
and exported with matching arities, and refuse bad arguments before any device call (no GPU needed)."""
import ctypes
import os

from abi import ROOT, declared, library

NAMES = ("ss_deconv2d_bf16s_fwd", "ss_deconv2d_bf16s_pair_fwd", "ss_pack_deconv2d_weights_f16s", "ss_conv2d_bf16s_cat_fwd")


def test_decoder_entry_points_are_declared_with_the_bindings_arities():
    _l, lib = library()
    decl = {name: len(params) for name, (_, params) in declared().items()}
    for name in NAMES:
        assert name in decl and name in _l._SIGNATURES and name in _l.EXPORTS, name
        assert len(_l._SIGNATURES[name]) == decl[name], (name, len(_l._SIGNATURES[name]), decl[name])
    assert "deconv2d_bf16s.hip" in open(os.path.join(ROOT, "semstereo_amd", "csrc", "Makefile")).read()


def test_the_library_exports_them():
    _l, lib = library()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert lib.ss_abi_version() == _l.ABI_VERSION


def test_bad_arguments_are_refused_before_any_device_call():
    _l, lib = library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                      # 16-byte aligned host memory that is never followed

    def dec(x=p, w=p, out=p, B=1, Cin=8, H=4, W=4, Cout=8, nterms=19):
        return lib.ss_deconv2d_bf16s_fwd(x, w, None, None, out, B, Cin, H, W, Cout, 1, nterms, None)
    assert dec(x=None) == -1 and dec(w=None) == -1 and dec(out=None) == -1
    assert dec(B=0) == -1 and dec(Cin=0) == -1 and dec(H=0) == -1 and dec(W=-1) == -1 and dec(Cout=0) == -1
    assert dec(nterms=6) == -2 and dec(nterms=3) == -2          # the bf16 forms of this layer are not built
    assert dec(Cin=1 << 16, H=1 << 8, W=1 << 8) == -2           # one sample's input beyond the 32-bit offsets
    assert lib.ss_deconv2d_bf16s_pair_fwd(p, None, p, None, None, p, 1, 8, 4, 4, 8, 1, 19, None) == -1
    assert lib.ss_pack_deconv2d_weights_f16s(None, p, 8, 8, None) == -1 and lib.ss_pack_deconv2d_weights_f16s(p, p, 0, 8, None) == -1

    def cat(xa=p, ra=p, xb=None, rb=None, Cs=8, Cin=16, nterms=19):
        return lib.ss_conv2d_bf16s_cat_fwd(xa, ra, xb, rb, p, None, None, p, 1, Cs, Cin, 4, 4, 8, 1, nterms, None)
    assert cat(xa=None) == -1 and cat(ra=None) == -1 and cat(xb=p) == -1 and cat(rb=p) == -1
    assert cat(Cs=0) == -1 and cat(Cs=16) == -1 and cat(Cs=24) == -1
    assert cat(Cs=12) == -2 and cat(Cs=4, Cin=9) == -2           # a chunk of 8 channels would straddle the two tensors
    assert cat(nterms=7) == -1


def test_switch_and_engine_surface():
    import semstereo_amd as sa
    assert "DECODER_HIP" in sa.engine.SWITCHES and sa.engine.DECODER_HIP in ("auto", True, False)
    for name in ("pack_deconv2d_weight", "deconv2d_bf16s_hip", "run_deconv2d", "run_conv2d_cat"):
        assert callable(getattr(sa.engine, name)), name
    import torch
    import torch.nn as nn
    dc, x = nn.ConvTranspose2d(8, 8, 4, 2, 1, bias=False), torch.zeros(1, 8, 4, 4)
    assert sa.engine.run_deconv2d(dc, "k", dc, None, x, True) is None            # a CPU tensor: does not apply
    cv = nn.Conv2d(16, 8, 3, 1, 1, bias=False)
    assert sa.engine.run_conv2d_cat(cv, "k", cv, None, x, torch.zeros(1, 8, 4, 4), True) is None
