"""CPU: the sample-preparation entry points (csrc/sample_prep.hip) are declared, bound and exported with matching arities, refuse bad
arguments before any device call, and CPU tensors take the PyTorch composition with the counters moving as stated (no GPU needed)."""
import ctypes
import os
import re

import torch

from abi import ROOT, declared, library

NAMES = ("ss_prep_views_fwd", "ss_prep_pyramid_fwd", "ss_prep_luma_stats_fwd", "ss_prep_gradients_fwd")      # (a stream argument each)
QUERY = "ss_prep_workspace_bytes"


def test_prep_entry_points_are_declared_bound_and_exported():
    _l, lib = library()
    decl = {name: len(params) for name, (_, params) in declared().items()}
    for name in NAMES:
        assert name in decl and name in _l._SIGNATURES and name in _l.EXPORTS, name
        assert len(_l._SIGNATURES[name]) == decl[name], (name, len(_l._SIGNATURES[name]), decl[name])
        assert hasattr(lib, name), name
    assert QUERY in decl and QUERY in _l.EXPORTS and len(lib.ss_prep_workspace_bytes.argtypes) == decl[QUERY] == 4
    assert _l.ABI_VERSION == 20 and lib.ss_abi_version() == 20          # symbols were added, nothing changed
    srcs = re.search(r"^SRCS_HIP\s*:=(.*)$", open(os.path.join(ROOT, "semstereo_amd", "csrc", "Makefile")).read(), flags=re.M).group(1)
    assert "sample_prep.hip" in srcs.split()


def test_the_source_only_launches():
    text = open(os.path.join(ROOT, "semstereo_amd", "csrc", "sample_prep.hip")).read()
    for word in ("hipMemcpy", "hipMemset", "Synchronize", "hipMalloc", "hipFree", "hipEvent", "atomicAdd", "__hip_atomic", "printf"):
        assert word not in text, word


def test_bad_arguments_are_refused_before_any_device_call():
    _l, lib = library()
    n = ctypes.c_longlong(0)
    q = lib.ss_prep_workspace_bytes
    assert q(1, 4, 4, None) == -1 and q(0, 4, 4, ctypes.byref(n)) == -1 and q(1, 0, 4, ctypes.byref(n)) == -1 and q(1, 4, -1, ctypes.byref(n)) == -1
    assert q(2, 37, 53, ctypes.byref(n)) == 0 and n.value >= 2 * 16 + 2 * 37 * 53 and n.value % 8 == 0
    assert q(1, 4096, 2048, ctypes.byref(n)) == 0                      # 2^23 pixels: the last exact size
    assert q(1, 4096, 2049, ctypes.byref(n)) == -2                     # ... beyond: N S2 - S1^2 would leave 64 bits
    assert q(70000, 4, 4, ctypes.byref(n)) == -2
    # pointers that are never followed
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 40

    def views(left=p, right=p, table=p, B=1, H=4, W=4, ol=p, orr=p):
        return lib.ss_prep_views_fwd(left, right, table, B, H, W, ol, orr, None)

    def pyr(d=p, dd=0, y=p, yd=1, row=16, img=256, B=1, H=16, W=16, outs=(p,) * 7):
        return lib.ss_prep_pyramid_fwd(d, dd, 1.0, y, yd, row, img, B, H, W, *outs, None)

    def stats(left=p, B=1, H=4, W=4, ws=p, ws_bytes=big):
        return lib.ss_prep_luma_stats_fwd(left, B, H, W, ws, ws_bytes, None)

    def grad(ws=p, ws_bytes=big, B=1, H=4, W=4, gx=p, gy=p):
        return lib.ss_prep_gradients_fwd(ws, ws_bytes, B, H, W, gx, gy, None)
    assert views(left=None) == -1 and views(table=None) == -1 and views(ol=None) == -1
    assert views(right=None) == -1 and views(orr=None) == -1            # the right view and its output come together
    assert views(B=0) == -1 and views(H=0) == -1 and views(W=-2) == -1
    assert views(B=1 << 10, H=1 << 10, W=1 << 10) == -2                 # 3 * 2^30 bytes: 2^31 elements or more
    none = (None,) * 7
    assert pyr(outs=none) == -1                                          # nothing asked for
    assert pyr(d=None) == -1 and pyr(y=None) == -1 and pyr(dd=2) == -1 and pyr(dd=-1) == -1 and pyr(yd=3) == -1 and pyr(yd=-1) == -1
    assert pyr(B=0) == -1 and pyr(H=0) == -1 and pyr(W=0) == -1
    assert pyr(row=15) == -1 and pyr(img=255) == -1                      # label strides that would leave the tensor
    assert pyr(H=37, W=53, row=53, img=37 * 53) == -2 and pyr(H=24, W=16, img=24 * 16) == -2      # sizes 16 does not divide
    assert pyr(B=1 << 11, H=1 << 10, W=1 << 10, row=1 << 10, img=1 << 20) == -2
    assert stats(left=None) == -1 and stats(ws=None) == -1 and stats(B=0) == -1 and stats(H=0) == -1 and stats(W=0) == -1
    assert stats(ws_bytes=16) == -1                                      # workspace too small
    assert stats(H=4096, W=2049) == -2 and stats(B=70000) == -2
    assert grad(ws=None) == -1 and grad(gx=None) == -1 and grad(gy=None) == -1 and grad(B=0) == -1 and grad(H=0) == -1 and grad(W=0) == -1
    assert grad(ws_bytes=16) == -1 and grad(H=4096, W=2049) == -2


def test_workspace_query():
    from semstereo_amd import data as D
    assert D.workspace_bytes(4, 1024, 1024) >= 4 * 1024 * 1024 + 64


def test_cpu_tensors_take_the_pytorch_composition():
    import semstereo_amd as sa
    assert "DATA_HIP" in sa.engine.SWITCHES and isinstance(sa.engine.DATA_HIP, bool)
    g = torch.Generator().manual_seed(3)
    left = torch.randint(0, 256, (2, 16, 32, 3), generator=g, dtype=torch.uint8)
    right = torch.randint(0, 256, (2, 16, 32, 3), generator=g, dtype=torch.uint8)
    disp, label = torch.randn(2, 16, 32, generator=g), torch.randint(0, 6, (2, 16, 32), generator=g)
    before = dict(sa.modules.PATH_COUNTS)

    def moved():
        return sa.modules.PATH_COUNTS.get("data_torch", 0) - before.get("data_torch", 0)
    a, b = sa.normalize_views(left, right)
    assert moved() == 1 and a.shape == (2, 3, 16, 32) and a.dtype == torch.float32 and b.shape == a.shape
    p = sa.nearest_pyramid(disp, label)
    assert moved() == 2 and p["label"].dtype == torch.float32 and p["label_4"].shape == (2, 4, 8) and p["disparity"] is disp
    gx, gy = sa.image_gradients(left)
    assert moved() == 3 and gx.shape == (2, 1, 16, 32) and gy.dtype == torch.float32 and bool(torch.isfinite(gx).all())
    s = sa.prepare_sample({"left_u8": left, "right_u8": right, "disparity": disp, "label": label}, True)
    assert moved() == 6 and len(s) == 11
    assert sa.modules.PATH_COUNTS.get("data_hip", 0) == before.get("data_hip", 0)
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"] and sa.modules.PATH_COUNTS["hip"] == before["hip"]
    assert not sa.normalize_views(left).requires_grad
