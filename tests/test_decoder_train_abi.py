"""CPU: the entry points of the 2-D decoder's training kernels (csrc/deconv2d_train.hip) are declared, bound and exported with matching
arities, refuse bad arguments before any device call, the workspace size is the documented formula, and the opt-in switch is listed
and off by default (no GPU needed)."""
import ctypes
import os

from abi import HEADER, ROOT, declared, library

NAMES = ("ss_conv2d_k4s2_f16s_fwd", "ss_pack_conv2d_k4s2_weights_f16s", "ss_deconv2d_k4s2_wgrad_fwd", "ss_deconv2d_k4s2_wgrad_workspace_bytes")
LL = ctypes.c_longlong


def test_entry_points_are_declared_with_the_bindings_arities():
    _l, lib = library()
    decl = {name: len(params) for name, (_, params) in declared().items()}
    for name in NAMES:
        assert name in decl and name in _l._SIGNATURES and name in _l.EXPORTS, name
        assert len(_l._SIGNATURES[name]) == decl[name], (name, len(_l._SIGNATURES[name]), decl[name])
    assert [decl[n] for n in NAMES] == [9, 5, 10, 6]
    header = open(HEADER).read()
    for cite in ("models/submodule.py:104", "136-138, 150", "models/SemStereo.py:207"):
        assert cite in header, cite
    mk = open(os.path.join(ROOT, "semstereo_amd", "csrc", "Makefile")).read()
    assert "deconv2d_train.hip" in mk


def test_the_library_exports_them_and_the_abi_version_is_unchanged():
    _l, lib = library()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert len(lib.ss_deconv2d_k4s2_wgrad_workspace_bytes.argtypes) == 6
    assert lib.ss_abi_version() == _l.ABI_VERSION == 20


def test_bad_arguments_are_refused_before_any_device_call():
    _l, lib = library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                      # 16-byte aligned host memory that is never followed

    def conv(g=p, ws=p, out=p, B=1, Cin=8, H=4, W=4, Cout=8):
        return lib.ss_conv2d_k4s2_f16s_fwd(g, ws, out, B, Cin, H, W, Cout, None)
    assert conv(g=None) == -1 and conv(ws=None) == -1 and conv(out=None) == -1
    assert conv(B=0) == -1 and conv(Cin=0) == -1 and conv(H=0) == -1 and conv(W=-2) == -1 and conv(Cout=0) == -1 and conv(B=-1) == -1
    assert conv(ws=ctypes.c_void_p(p.value + 8)) == -1          # the fragments are read 16 bytes at a time
    assert conv(H=5) == -2 and conv(W=7) == -2 and conv(H=3, W=3) == -2     # the gradient of a stride-2 transposed conv has even sizes
    assert conv(Cin=8, H=1 << 14, W=1 << 14) == -2              # one element's input beyond the 32-bit offsets
    assert conv(Cin=1, H=1 << 13, W=1 << 13, Cout=256) == -2    # ... its output

    def pack(w=p, ws=p, Cout=8, Cin=8):
        return lib.ss_pack_conv2d_k4s2_weights_f16s(w, ws, Cout, Cin, None)
    assert pack(w=None) == -1 and pack(ws=None) == -1 and pack(Cout=0) == -1 and pack(Cin=-8) == -1
    assert pack(ws=ctypes.c_void_p(p.value + 4)) == -1

    def wgrad(x=p, g=p, gw=p, ws=p, B=1, Cin=8, H=4, W=4, Cout=8):
        return lib.ss_deconv2d_k4s2_wgrad_fwd(x, g, gw, ws, B, Cin, H, W, Cout, None)
    assert wgrad(x=None) == -1 and wgrad(g=None) == -1 and wgrad(gw=None) == -1 and wgrad(ws=None) == -1
    assert wgrad(B=0) == -1 and wgrad(Cin=0) == -1 and wgrad(H=-4) == -1 and wgrad(W=0) == -1 and wgrad(Cout=0) == -1
    assert wgrad(Cin=8, H=1 << 13, W=1 << 13) == -2             # one element's input of 2 GiB
    assert wgrad(Cin=1, Cout=2, H=1 << 13, W=1 << 13) == -2     # one element's output gradient (four times the positions) of 2 GiB
    assert wgrad(Cin=1 << 14, Cout=1 << 14, H=1, W=1) == -2     # more weight tiles than a grid axis holds


def _formula(B, Cin, H, W, Cout):
    cdiv = lambda a, b: -(-a // b)
    rows, tiles = B * H, cdiv(Cin, 32) * cdiv(Cout, 32)
    cap = min(256, max(1, 1024 // tiles))
    rpp = min(rows, max(cdiv(rows, cap), cdiv(2048, W)))
    return cdiv(rows, rpp) * tiles * 65536


def test_workspace_bytes_is_the_documented_formula():
    _l, lib = library()
    n = LL(-1)
    ws = lib.ss_deconv2d_k4s2_wgrad_workspace_bytes
    assert ws(1, 8, 4, 4, 8, None) == -1
    assert ws(0, 8, 4, 4, 8, ctypes.byref(n)) == -1 and ws(1, 8, 0, 4, 8, ctypes.byref(n)) == -1 and ws(1, 8, 4, 4, -1, ctypes.byref(n)) == -1
    assert ws(1, 8, 1 << 13, 1 << 13, 8, ctypes.byref(n)) == -2
    assert n.value == -1                                         # (a refused call writes nothing)
    # ragged everything: 3 x 2 weight tiles, 7 x 23 rows of 37 positions -> 56 rows per partial, 3 partials
    assert ws(7, 70, 23, 37, 40, ctypes.byref(n)) == 0 and n.value == _formula(7, 70, 23, 37, 40) == 3 * 6 * 65536
    for shape in ((2, 16, 40, 70, 16), (1, 128, 8, 8, 6), (3, 8, 1, 1, 8), (4, 512, 32, 32, 384), (4, 256, 256, 256, 64), (1, 64, 512, 512, 32)):
        assert ws(*shape, ctypes.byref(n)) == 0 and n.value == _formula(*shape), shape
        assert 0 < n.value <= 64 << 20, shape                   # modest: at most 64 MiB up to 1024 weight tiles, the largest layer at batch 4 included
    assert ws(2, 16, 40, 70, 16, ctypes.byref(n)) == 0 and n.value == 3 * 65536      # more than one partial per weight tile
    # beyond 1024 weight tiles: one partial per tile, whatever the rows
    assert ws(4, 2048, 64, 64, 1024, ctypes.byref(n)) == 0 and n.value == _formula(4, 2048, 64, 64, 1024) == 64 * 32 * 65536


def test_the_switch_is_listed_and_off_by_default():
    import semstereo_amd as sa
    import torch
    E, M = sa.engine, sa.modules
    assert "DECODER_TRAIN_HIP" in E.SWITCHES
    if "SS_DECODER_TRAIN_HIP" not in os.environ:
        assert E.DECODER_TRAIN_HIP is False
    assert M.DECODER_TRAIN_HIP is E.DECODER_TRAIN_HIP            # (reads of modules.X are forwarded to the engine's switches)
    TD = __import__("semstereo_amd.train_decoder", fromlist=["x"])
    for name in ("conv2x_train", "spx2_train", "conv2x_train_applies", "spx2_train_applies", "_Deconv2dK4S2", "_Conv2dK3Cat", "DGRAD_HIP",
                 "WGRAD_HIP"):
        assert hasattr(TD, name), name
    c2x, spx2 = M.Conv2x(16, 8, deconv=True).train(), M.Spx2(16, 6).train()
    x, rem = torch.zeros(2, 16, 4, 4), torch.zeros(2, 8, 8, 8)
    assert not TD.conv2x_train_applies(c2x, x, rem) and not TD.spx2_train_applies(spx2, x)       # off, and CPU tensors
    before = dict(M.PATH_COUNTS)
    c2x(x, rem), spx2(x)
    assert M.PATH_COUNTS["torch"] == before["torch"] + 2 + 1      # (the stock path counts one per BasicConv)
    assert M.PATH_COUNTS.get("hip_train", 0) == before.get("hip_train", 0)
    assert M.PATH_COUNTS.get("decoder_train", 0) == before.get("decoder_train", 0)
    # ... and the switch alone does not move a CPU call
    saved, E.DECODER_TRAIN_HIP = E.DECODER_TRAIN_HIP, True
    try:
        assert not TD.conv2x_train_applies(c2x, x, rem) and not TD.spx2_train_applies(spx2, x)
        c2x(x, rem), spx2(x)
        fu = M.FeatUp().train()
        feats = [torch.zeros(2, c, 32 >> k, 32 >> k) for k, c in enumerate((64, 128, 256, 384, 512))]
        L, R = fu(feats, feats)
        assert [tuple(t.shape) for t in L] == [(2, 2 * c if k < 4 else c, 32 >> k, 32 >> k) for k, c in enumerate((64, 128, 256, 384, 512))]
        assert all(int(m.conv1.bn.num_batches_tracked) == 2 for m in (fu.deconv32_16, fu.deconv16_8, fu.deconv8_4, fu.deconv4_2))
    finally:
        E.DECODER_TRAIN_HIP = saved
    assert M.PATH_COUNTS.get("hip_train", 0) == before.get("hip_train", 0)
