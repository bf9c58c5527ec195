"""CPU: the entry points of the heads' training tail (csrc/seghead_train.hip) are declared, bound and exported with matching
arities, refuse bad arguments before any device call, and the opt-in switch is off by default (no GPU needed)."""
import ctypes
import os

from abi import ROOT, declared, library

NAMES = ("ss_seghead_tail_fwd", "ss_seghead_tail_bwd", "ss_seghead_tail_workspace_bytes")
LL = ctypes.c_longlong


def test_tail_entry_points_are_declared_with_the_bindings_arities():
    _l, lib = library()
    decl = {name: len(params) for name, (_, params) in declared().items()}
    for name in NAMES:
        assert name in decl and name in _l._SIGNATURES and name in _l.EXPORTS, name
        assert len(_l._SIGNATURES[name]) == decl[name], (name, len(_l._SIGNATURES[name]), decl[name])
    assert decl["ss_seghead_tail_fwd"] == 11 and decl["ss_seghead_tail_bwd"] == 14 and decl["ss_seghead_tail_workspace_bytes"] == 6
    mk = open(os.path.join(ROOT, "semstereo_amd", "csrc", "Makefile")).read()
    assert "seghead_train.hip" in mk


def test_the_library_exports_them_and_the_abi_version_is_unchanged():
    _l, lib = library()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert len(lib.ss_seghead_tail_workspace_bytes.argtypes) == 6
    assert lib.ss_abi_version() == _l.ABI_VERSION == 20


def test_bad_arguments_are_refused_before_any_device_call():
    _l, lib = library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                      # 16-byte aligned host memory that is never followed

    def fwd(a=p, w2=p, bias=p, out=p, B=1, K=32, C=6, H=4, W=4, up2=1):
        return lib.ss_seghead_tail_fwd(a, w2, bias, out, B, K, C, H, W, up2, None)
    assert fwd(a=None) == -1 and fwd(w2=None) == -1 and fwd(bias=None) == -1 and fwd(out=None) == -1
    assert fwd(B=0) == -1 and fwd(K=0) == -1 and fwd(C=0) == -1 and fwd(H=0) == -1 and fwd(W=-1) == -1 and fwd(B=-2) == -1
    assert fwd(K=16) == -2 and fwd(C=9) == -2
    assert fwd(H=1 << 13, W=1 << 13) == -2 and fwd(H=1 << 13, W=1 << 13, up2=0) == -2     # one element's `a` beyond the 32-bit offsets

    def bwd(g=p, a=p, w2=p, ga=p, gw=p, gb=p, ws=p, B=1, K=32, C=6, H=4, W=4, up2=1):
        return lib.ss_seghead_tail_bwd(g, a, w2, ga, gw, gb, ws, B, K, C, H, W, up2, None)
    assert bwd(g=None) == -1 and bwd(a=None) == -1 and bwd(w2=None) == -1
    assert bwd(ga=None, gw=None, gb=None) == -1                  # each gradient may be NULL, not all three
    assert bwd(ws=None) == -1 and bwd(ws=None, gw=None) == -1 and bwd(ws=None, gb=None) == -1     # the sums need their workspace
    assert bwd(B=0) == -1 and bwd(K=-32) == -1 and bwd(C=0) == -1 and bwd(H=0) == -1 and bwd(W=0) == -1
    assert bwd(K=16) == -2 and bwd(C=9) == -2 and bwd(ga=None, K=16) == -2 and bwd(gw=None, gb=None, ws=None, C=9) == -2
    assert bwd(H=1 << 13, W=1 << 13) == -2

    n = LL(-1)
    assert lib.ss_seghead_tail_workspace_bytes(1, 32, 6, 4, 4, None) == -1
    assert lib.ss_seghead_tail_workspace_bytes(0, 32, 6, 4, 4, ctypes.byref(n)) == -1
    assert lib.ss_seghead_tail_workspace_bytes(1, 32, 6, 0, 4, ctypes.byref(n)) == -1
    assert lib.ss_seghead_tail_workspace_bytes(1, 16, 6, 4, 4, ctypes.byref(n)) == -2
    assert lib.ss_seghead_tail_workspace_bytes(1, 32, 9, 4, 4, ctypes.byref(n)) == -2
    assert n.value == -1                                         # (a refused call writes nothing)
    # one partial per workgroup: 8 x 32 tiles of one element, C x (32 weight columns + the bias) floats each
    assert lib.ss_seghead_tail_workspace_bytes(3, 32, 6, 9, 33, ctypes.byref(n)) == 0 and n.value == 3 * (2 * 2) * 6 * 33 * 4


def test_the_switch_is_listed_and_off_by_default():
    import semstereo_amd as sa
    E = sa.engine
    assert "HEADS_TRAIN_HIP" in E.SWITCHES
    if "SS_HEADS_TRAIN_HIP" not in os.environ:
        assert E.HEADS_TRAIN_HIP is False
    assert sa.modules.HEADS_TRAIN_HIP is E.HEADS_TRAIN_HIP        # (reads of modules.X are forwarded to the engine's switches)
    TH = sa.train_heads if hasattr(sa, "train_heads") else __import__("semstereo_amd.train_heads", fromlist=["x"])
    for name in ("seghead_train", "proj_train", "seghead_train_applies", "proj_train_applies", "_SegheadTail", "_Proj2dK1"):
        assert hasattr(TH, name), name
    assert TH.PROJ_MIN_POSITIONS == 32768                         # (projections below it keep the stock layers: measured slower there)
    import torch
    head, proj = sa.modules.segmenthead(8, 32, 6, 2), sa.modules.ChalProjection(8, 8)
    x = torch.zeros(1, 8, 4, 4)
    assert not TH.seghead_train_applies(head, x) and not TH.proj_train_applies(proj, x)          # off, and a CPU tensor
    before = dict(sa.modules.PATH_COUNTS)
    head.train()(x), proj.train()(x)
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"] + 2
    assert sa.modules.PATH_COUNTS.get("hip_train", 0) == before.get("hip_train", 0)
