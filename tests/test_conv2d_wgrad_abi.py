"""CPU: the entry points of the 2-D 3x3 weight-gradient kernel (csrc/conv2d_wgrad.hip) are declared, bound and exported with matching
arities, refuse bad arguments before any device call, the workspace size is the documented formula, and the opt-in switch is listed
and off by default (no GPU needed)."""
import ctypes
import os

from abi import HEADER, ROOT, declared, library

NAMES = ("ss_conv2d_k3_wgrad_fwd", "ss_conv2d_k3_wgrad_workspace_bytes")
LL = ctypes.c_longlong
# (B, C0, C1, H, W, Cout) of the layers at 1024 x 1024 inputs, batch 4: the four Conv2x.conv2, concat_feature's two convs, segmenthead.conv1
MODEL_SHAPES = ((4, 384, 384, 64, 64, 768), (4, 256, 256, 128, 128, 512), (4, 128, 128, 256, 256, 256), (4, 64, 64, 512, 512, 128),
                (4, 128, 0, 256, 256, 64), (4, 64, 0, 256, 256, 32), (4, 128, 0, 512, 512, 32))


def test_entry_points_are_declared_with_the_bindings_arities():
    _l, lib = library()
    decl = {name: len(params) for name, (_, params) in declared().items()}
    for name in NAMES:
        assert name in decl and name in _l._SIGNATURES and name in _l.EXPORTS, name
    assert len(_l._SIGNATURES[NAMES[0]]) == decl[NAMES[0]] == 12
    assert len(_l._SIGNATURES[NAMES[1]]) == decl[NAMES[1]] == 7
    header = open(HEADER).read()
    for cite in ("models/submodule.py:142, 157-160", "models/SemStereo.py:221-223", "models/submodule.py:40-52"):
        assert cite in header, cite
    mk = open(os.path.join(ROOT, "semstereo_amd", "csrc", "Makefile")).read()
    assert "conv2d_wgrad.hip" in mk


def test_the_library_exports_them_and_the_abi_version_is_unchanged():
    _l, lib = library()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert len(lib.ss_conv2d_k3_wgrad_fwd.argtypes) == 12 and len(lib.ss_conv2d_k3_wgrad_workspace_bytes.argtypes) == 7
    assert lib.ss_abi_version() == _l.ABI_VERSION == 20


def test_bad_arguments_are_refused_before_any_device_call():
    _l, lib = library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                      # host memory that is never followed

    def wgrad(g=p, x=p, rem=p, gw=p, ws=p, B=1, C0=8, C1=8, H=4, W=4, Cout=8):
        return lib.ss_conv2d_k3_wgrad_fwd(g, x, rem, gw, ws, B, C0, C1, H, W, Cout, None)
    assert wgrad(g=None) == -1 and wgrad(x=None) == -1 and wgrad(gw=None) == -1 and wgrad(ws=None) == -1
    assert wgrad(rem=None) == -1 and wgrad(rem=None, C1=1) == -1      # C1 > 0 needs the second source
    for name in ("B", "C0", "H", "W", "Cout"):
        assert wgrad(**{name: 0}) == -1 and wgrad(**{name: -3}) == -1, name
    assert wgrad(C1=-1) == -1 and wgrad(C1=-1, rem=None) == -1
    assert wgrad(Cout=8, C0=1, C1=1, H=1 << 13, W=1 << 13) == -2      # one element's grad_out of 2 GiB
    assert wgrad(Cout=1, C0=8, C1=1, H=1 << 13, W=1 << 13) == -2      # ... in0
    assert wgrad(Cout=1, C0=1, C1=8, H=1 << 13, W=1 << 13) == -2      # ... in1
    assert wgrad(Cout=1, C0=8, C1=0, rem=None, H=1 << 13, W=1 << 13) == -2
    assert wgrad(B=1 << 16, H=1 << 15, W=1, C0=1, C1=0, Cout=1) == -2  # B * H beyond an int
    assert wgrad(C0=1 << 14, C1=1 << 14, Cout=1 << 11, H=1, W=1) == -2 # 1024 x 64 weight tiles: more than a grid axis holds
    assert wgrad(C0=1 << 15, C1=0, Cout=1 << 11, H=1, W=1) == -2


def _formula(B, C0, C1, H, W, Cout):
    cdiv = lambda a, b: -(-a // b)
    rows, tiles = B * H, (cdiv(C0, 32) + cdiv(C1, 32)) * cdiv(Cout, 32)
    cap = min(256, max(1, 1024 // tiles))
    rpp = min(rows, max(cdiv(rows, cap), cdiv(2048, W)))
    return cdiv(rows, rpp) * tiles * 36864


def test_workspace_bytes_is_the_documented_formula():
    _l, lib = library()
    n = LL(-1)
    ws = lib.ss_conv2d_k3_wgrad_workspace_bytes
    ref = ctypes.byref(n)
    assert ws(1, 8, 8, 4, 4, 8, None) == -1
    for bad in ((0, 8, 8, 4, 4, 8), (1, 0, 8, 4, 4, 8), (1, 8, -1, 4, 4, 8), (1, 8, 8, 0, 4, 8), (1, 8, 8, 4, -4, 8), (1, 8, 8, 4, 4, 0),
                (-1, 8, 8, 4, 4, 8)):
        assert ws(*bad, ref) == -1, bad
    for big in ((1, 8, 0, 1 << 13, 1 << 13, 1), (1, 1, 8, 1 << 13, 1 << 13, 1), (1, 1, 0, 1 << 13, 1 << 13, 8), (1 << 16, 1, 0, 1 << 15, 1, 1),
                (1, 1 << 14, 1 << 14, 1, 1, 1 << 11)):
        assert ws(*big, ref) == -2, big
    assert n.value == -1                                         # (a refused call writes nothing)
    # ragged everything: (3 + 1) x 2 weight tiles, 7 x 23 rows of 37 positions -> 56 rows per partial, 3 partials
    assert ws(7, 70, 9, 23, 37, 40, ref) == 0 and n.value == _formula(7, 70, 9, 23, 37, 40) == 3 * 8 * 36864
    # an input tile belongs to one source: 33 + 1 channels are 2 + 1 tiles, not the ceil(34 / 32) = 2 of the concatenation
    assert ws(1, 33, 1, 4, 4, 8, ref) == 0 and n.value == 3 * 36864
    for shape in ((2, 24, 16, 5, 37, 40), (3, 8, 0, 1, 1, 8), (1, 3, 5, 2, 3, 33), (1, 40, 40, 33, 64, 6), (2, 16, 0, 40, 70, 16), (1, 64, 64, 16, 16, 128)):
        assert ws(*shape, ref) == 0 and n.value == _formula(*shape) and n.value % 36864 == 0, shape
    assert ws(2, 16, 0, 40, 70, 16, ref) == 0 and n.value == 3 * 36864      # more than one partial per weight tile
    for shape in MODEL_SHAPES:
        assert ws(*shape, ref) == 0 and n.value == _formula(*shape), shape
        assert n.value % 36864 == 0 and 0 < n.value <= 64 << 20, shape
    # beyond 1024 weight tiles: one partial per tile, whatever the rows
    assert ws(4, 1024, 1024, 64, 64, 1024, ref) == 0 and n.value == _formula(4, 1024, 1024, 64, 64, 1024) == 64 * 32 * 36864


def test_the_switch_is_listed_and_off_by_default():
    import semstereo_amd as sa
    import torch
    E, M = sa.engine, sa.modules
    T = __import__("semstereo_amd.train", fromlist=["x"])
    assert "CONV2D_WGRAD_HIP" in E.SWITCHES
    if "SS_CONV2D_WGRAD_HIP" not in os.environ:
        assert E.CONV2D_WGRAD_HIP is False
    assert M.CONV2D_WGRAD_HIP is E.CONV2D_WGRAD_HIP             # (reads of modules.X are forwarded to the engine's switches)
    for name in ("conv2d_k3_wgrad_hip", "conv2d_k3_wgrad_applies", "conv2d_k3_wgrad_workspace_bytes"):
        assert hasattr(T, name), name
    assert T.conv2d_k3_wgrad_workspace_bytes(2, 16, 0, 40, 70, 16) == 3 * 36864
    g, x, rem = torch.zeros(2, 8, 4, 4), torch.zeros(2, 16, 4, 4), torch.zeros(2, 8, 4, 4)
    saved, E.CONV2D_WGRAD_HIP = E.CONV2D_WGRAD_HIP, True
    try:
        # the switch alone does not move a CPU or a float64 call
        assert not T.conv2d_k3_wgrad_applies(g, x) and not T.conv2d_k3_wgrad_applies(g, x, rem)
        assert not T.conv2d_k3_wgrad_applies(g.double(), x.double()) and not T.conv2d_k3_wgrad_applies(g.double(), x.double(), rem.double())
    finally:
        E.CONV2D_WGRAD_HIP = saved
