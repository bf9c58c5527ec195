"""CPU: the training augmentation (semstereo_amd/augment.py, csrc/augment.hip) -- the PyTorch composition against a per-pixel restatement
on every case the GPU tests run, the identity against prepare_sample, the swap's convention on a constructed pair, the contrast mean on a
tie, the C ABI's declarations and refusals, and DeviceLoader(augment=...) on the CPU (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import augment_cases as ac
from abi import ROOT, declared, library

LAUNCHERS = ("ss_augment_stats_fwd", "ss_augment_occluder_fwd", "ss_augment_write_fwd")      # (a stream argument each)
QUERIES = {"ss_augment_scratch_bytes": 6, "ss_augment_param_bytes": 2}


@pytest.mark.parametrize("name", ac.GPU_CASES)
def test_composition_equals_the_restatement(name):
    want, got = ac.restated(name), ac.composed(name)
    assert tuple(got) == ac.CASES[name]["keys"]
    for k in want:
        assert got[k].dtype == torch.float32 and np.array_equal(want[k], got[k].numpy()), (name, k)


def _raw(B, H, W, seed=5, label=torch.uint8):
    g = torch.Generator().manual_seed(seed)
    return {"left_u8": torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8),
            "right_u8": torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8),
            "disparity": torch.randn(B, H, W, generator=g) * 4, "label": torch.randint(0, 6, (B, H, W), generator=g).to(label)}


def test_identity_equals_prepare_sample():
    import semstereo_amd as sa
    raw = _raw(2, 32, 48)
    before = {k: v.clone() for k, v in raw.items()}
    out = sa.augment_sample(raw, sa.AugmentParams((32, 48), (32, 48), [(0, 0)] * 2))
    ref = sa.prepare_sample(raw, True, ac.NINE)
    assert tuple(out) == tuple(ref) == ac.NINE
    for k in ref:
        assert torch.equal(out[k], ref[k]), k
    assert all(torch.equal(raw[k], before[k]) for k in raw)                     # raw is never modified


def test_swap_keeps_the_disparity_convention():
    """A constructed pair: right[y, x - d] = left[y, x] at the owners (the largest x landing on a column).  After the swap, wherever the
    new disparity d' is in range, new_right[y, x' - d'] == new_left[y, x'] -- compared through the view table, which is injective."""
    import semstereo_amd as sa
    H, W, m = 12, 40, 6
    g = torch.Generator().manual_seed(9)
    left = torch.randint(0, 256, (1, H, W, 3), generator=g, dtype=torch.uint8)
    d = torch.randint(-m, m, (1, H, W), generator=g)
    right = torch.randint(0, 256, (1, H, W, 3), generator=g, dtype=torch.uint8)
    for y in range(H):
        for x in range(W):                                                      # raster order: the last writer is the largest x
            t = x - int(d[0, y, x])
            if 0 <= t < W:
                right[0, y, t] = left[0, y, x]
    raw = {"left_u8": left, "right_u8": right, "disparity": d.to(torch.float32), "label": torch.zeros(1, H, W, dtype=torch.uint8)}
    out = sa.augment_sample(raw, sa.AugmentParams((H, W), (H, W), [(0, 0)], swap=[1]), ("left", "right", "disparity"), maxdisp=m)
    assert torch.equal(out["left"], sa.normalize_views(right.flip(2))) and torch.equal(out["right"], sa.normalize_views(left.flip(2)))
    nd = out["disparity"][0]
    valid = (nd >= -m) & (nd < m)
    assert int(valid.sum()) > H * W // 2
    x = torch.arange(W).view(1, W).expand(H, W)
    t = (x - nd.long()).clamp(0, W - 1)
    matched = out["right"][0].gather(2, t.view(1, H, W).expand(3, H, W))
    assert bool(((matched == out["left"][0]).all(0) | ~valid).all())
    assert bool((nd[~valid] == -999.0).all())


def test_contrast_mean_on_a_tie():
    """Half the pixels of luma k, half of k + 1: S / N = k + 0.5 and m = int(k + 1.0) = k + 1."""
    import semstereo_amd as sa
    k, H, W = 77, 8, 12
    grey = torch.full((1, H, W, 3), k, dtype=torch.uint8)
    grey.view(-1, 3)[::2] = k + 1
    raw = {"left_u8": grey, "right_u8": grey.clone(), "disparity": torch.zeros(1, H, W)}
    out = sa.augment_sample(raw, sa.AugmentParams((H, W), (H, W), [(0, 0)], contrast=[(0.0, 1.0)]), ("left", "right"))
    table = sa.data.view_table()
    for ch in range(3):                                                         # c = 0: every pixel is the mean itself
        assert bool((out["left"][0, ch] == table[ch][k + 1]).all())
    assert torch.equal(out["right"], sa.normalize_views(grey))


def test_parameters_are_validated():
    import semstereo_amd as sa
    P = sa.AugmentParams
    for bad in (dict(origin=[(9, 0)]), dict(origin=[(0, 17)]), dict(origin=[(-1, 0)]), dict(origin=[(0, 0)], contrast=[(-0.1, 1.0)]),
                dict(origin=[(0, 0)], gamma=[(float("nan"), 1.0)]), dict(origin=[(0, 0)], brightness=[(float("inf"), 1.0)])):
        with pytest.raises(AssertionError):
            P((24, 32), (32, 48), **bad)
    with pytest.raises(AssertionError):
        P((40, 32), (32, 48), [(0, 0)])
    raw = _raw(1, 32, 48)
    p = P((24, 32), (32, 48), [(8, 16)], swap=[1])
    for keys in (("left", "gx"), ("gy",), ("left", "right_label"), ("left_visible",)):
        with pytest.raises(AssertionError):
            sa.augment_sample(raw, p, keys, maxdisp=8)
    with pytest.raises(AssertionError):                                          # a swapped map needs right_view's range
        sa.augment_sample(raw, p, ("disparity",))
    with pytest.raises(AssertionError):
        sa.augment_sample(raw, p, ("disparity",), maxdisp=8, disp_range=(0, 8))
    assert tuple(sa.augment_sample(raw, p, ("right", "left"))) == ("left", "right")      # the views alone need none


def test_draws_are_the_reference_ranges_and_repeat_with_the_seed():
    import semstereo_amd as sa
    a, b = (sa.Augmentation(crop=(256, 512), p_occluder=0.5, seed=4).draw(16, 300, 600) for _ in range(2))
    for k in ("origin", "vflip", "swap", "occluder", "brightness", "gamma", "contrast", "saturation"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert not bool(a.vflip.any()) and not bool(a.swap.any())                   # the KITTI recipe has no flips
    assert bool(((a.brightness >= 0.5) & (a.brightness < 2.0)).all()) and bool(((a.saturation >= 0) & (a.saturation < 1.4)).all())
    assert bool(((a.gamma >= 0.8) & (a.gamma < 1.2)).all()) and bool(((a.contrast >= 0.8) & (a.contrast < 1.2)).all())
    occ = a.occluder[a.has_occluder]
    assert 0 < len(occ) < 16
    cy, sy, cx, sx = occ.unbind(1)
    assert bool(((sy >= 35) & (sy < 100) & (sx >= 25) & (sx < 75) & (cy >= sy) & (cy <= 256 - sy) & (cx >= sx) & (cx <= 512 - sx)).all())
    assert bool(((a.origin[:, 0] <= 44) & (a.origin[:, 1] <= 88) & (a.origin >= 0).all(1)).all())
    u = sa.Augmentation.us3d((64, 64), 32, p_occluder=0.0, seed=1)
    p = u.draw(64, 64, 80)
    assert u.maxdisp == 32 and 8 < int(p.vflip.sum()) < 56 and 8 < int(p.swap.sum()) < 56 and not bool(p.has_occluder.any())
    with pytest.raises(AssertionError):                                          # dim > 2 * (hi - 1)
        sa.Augmentation(crop=(128, 512)).draw(1, 128, 600)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_are_declared_bound_and_exported():
    _l, lib = library()
    decl = {name: len(params) for name, (_, params) in declared().items()}
    for name in LAUNCHERS + tuple(QUERIES):
        assert name in decl and name in _l._SIGNATURES and name in _l.EXPORTS, name
        assert len(_l._SIGNATURES[name]) == decl[name], (name, len(_l._SIGNATURES[name]), decl[name])
        assert hasattr(lib, name), name
    for name, n in QUERIES.items():
        assert decl[name] == n
    for name in LAUNCHERS:
        assert declared()[name][1][-1] == "ss_stream_t", name
    assert _l.ABI_VERSION == 20 and lib.ss_abi_version() == 20                  # symbols were added, nothing changed
    srcs = re.search(r"^SRCS_HIP\s*:=(.*)$", open(os.path.join(ROOT, "semstereo_amd", "csrc", "Makefile")).read(), flags=re.M).group(1)
    assert "augment.hip" in srcs.split()


def test_the_source_only_launches():
    text = open(os.path.join(ROOT, "semstereo_amd", "csrc", "augment.hip")).read()
    for word in ("hipMemcpy", "hipMemset", "Synchronize", "hipMalloc", "hipFree", "hipEvent", "atomicAdd", "__hip_atomic", "printf"):
        assert word not in text, word


def test_bad_arguments_are_refused_before_any_device_call():
    from semstereo_amd import augment as A
    _l, lib = library()
    n = ctypes.c_longlong(0)
    ref = ctypes.byref(n)
    q, pb = lib.ss_augment_scratch_bytes, lib.ss_augment_param_bytes
    assert pb(3, None) == -1 and pb(0, ref) == -1 and pb(70000, ref) == -2
    assert pb(3, ref) == 0 and n.value == 3 * A.RECORD_BYTES == 3 * 560
    assert q(1, 8, 8, 4, 4, None) == -1 and q(0, 8, 8, 4, 4, ref) == -1 and q(1, 0, 8, 4, 4, ref) == -1 and q(1, 8, -1, 4, 4, ref) == -1
    assert q(1, 8, 8, 0, 4, ref) == -1 and q(1, 8, 8, 9, 4, ref) == -1 and q(1, 8, 8, 4, 9, ref) == -1     # the crop lies inside the image
    assert q(70000, 8, 8, 4, 4, ref) == -2 and q(1 << 10, 1 << 10, 1 << 10, 4, 4, ref) == -2
    assert q(2, 96, 128, 96, 128, ref) == 0
    gs = ac.partials_per_image(96, 128, 2)                                       # 12 per (item, view); the occluder pass has 12 per item too
    assert gs == 12 and n.value == -(-2 * 2 * gs * 8 // 256) * 256 + 2 * 12 * 3 * 8
    # pointers that are never followed
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    big = 1 << 40

    def sums(fn, left=p, right=p, params=p, B=1, H=8, W=8, th=4, tw=4, ws=p, ws_bytes=big):
        return fn(left, right, params, B, H, W, th, tw, ws, ws_bytes, None)

    def write(left=p, right=p, params=p, table=p, d=p, dd=0, y=p, yd=1, row=16, img=256, B=1, H=16, W=16, th=16, tw=16, ws=p,
              ws_bytes=big, occ=0, outs=(p,) * 9):
        return lib.ss_augment_write_fwd(left, right, params, table, d, dd, 1.0, y, yd, row, img, None, None, B, H, W, th, tw, ws, ws_bytes,
                                        occ, *outs, None)
    for fn in (lib.ss_augment_stats_fwd, lib.ss_augment_occluder_fwd):
        assert sums(fn, left=None) == -1 and sums(fn, right=None) == -1 and sums(fn, params=None) == -1 and sums(fn, ws=None) == -1
        assert sums(fn, B=0) == -1 and sums(fn, H=0) == -1 and sums(fn, W=-3) == -1 and sums(fn, th=0) == -1 and sums(fn, tw=0) == -1
        assert sums(fn, th=9) == -1 and sums(fn, tw=9) == -1
        assert sums(fn, ws_bytes=8) == -1 and sums(fn, ws=odd) == -1             # too small; not 8-byte aligned
        assert sums(fn, B=70000) == -2 and sums(fn, B=1 << 10, H=1 << 10, W=1 << 10) == -2
    none = (None,) * 9
    assert write(outs=none) == -1                                                # nothing asked for
    assert write(left=None) == -1 and write(right=None) == -1 and write(params=None) == -1 and write(ws=None) == -1
    assert write(table=None) == -1 and write(d=None) == -1 and write(y=None) == -1
    assert write(dd=2) == -1 and write(dd=-1) == -1 and write(yd=3) == -1 and write(yd=-1) == -1
    assert write(row=15) == -1 and write(img=255) == -1                          # label strides that would leave the tensor
    assert write(B=0) == -1 and write(H=0) == -1 and write(W=0) == -1 and write(th=0) == -1 and write(tw=17) == -1 and write(th=17) == -1
    assert write(occ=2) == -1 and write(occ=-1) == -1 and write(ws_bytes=8) == -1 and write(ws=odd) == -1
    assert write(H=40, W=56, row=56, img=40 * 56, th=24, tw=32) == -2 and write(H=40, W=56, row=56, img=40 * 56, th=32, tw=40) == -2
    assert write(B=70000) == -2 and write(B=1 << 10, H=1 << 10, W=1 << 10, row=1 << 10, img=1 << 20) == -2


def test_cpu_tensors_take_the_pytorch_composition():
    import semstereo_amd as sa
    assert "AUGMENT_HIP" in sa.engine.SWITCHES and isinstance(sa.engine.AUGMENT_HIP, bool)
    raw = _raw(2, 32, 48)
    before = dict(sa.modules.PATH_COUNTS)
    p = sa.AugmentParams((16, 32), (32, 48), [(3, 5), (16, 16)], vflip=[1, 0])
    out = sa.augment_sample(raw, p)
    assert tuple(out) == ac.NINE and out["left"].shape == (2, 3, 16, 32) and out["label_4"].shape == (2, 4, 8)
    assert not out["left"].requires_grad and all(v.dtype == torch.float32 for v in out.values())
    assert sa.modules.PATH_COUNTS.get("augment_torch", 0) - before.get("augment_torch", 0) == 1
    assert sa.modules.PATH_COUNTS.get("augment_hip", 0) == before.get("augment_hip", 0)
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"] and sa.modules.PATH_COUNTS["hip"] == before["hip"]
    whu = {k: v for k, v in raw.items() if k != "label"}
    whu["disparity"] = (raw["disparity"] * 256).to(torch.int32)
    out = sa.augment_sample(whu, sa.AugmentParams((32, 48), (32, 48), [(0, 0)] * 2, swap=[1, 0]), maxdisp=8)
    assert tuple(out) == ac.WHU_SIX
    assert torch.equal(out["disparity"][1], whu["disparity"][1].to(torch.float32) * (1.0 / 256.0))


# ------------------------------------------------------------------------------------------------ the loader
def _batches(n=3, B=2, H=48, W=64):
    return [_raw(B, H, W, seed=20 + i) for i in range(n)]


def test_device_loader_augments_the_training_branch_only():
    import semstereo_amd as sa
    keys = ("left", "right", "disparity", "disparity_4", "label")
    batches = _batches()

    def run(**kw):
        return list(sa.DeviceLoader(batches, device="cpu", keys=keys, **kw))
    make = lambda: sa.Augmentation.us3d((32, 48), 16, p_occluder=0.5, occluder_rows=(3, 9), occluder_cols=(3, 9), seed=7)    # noqa: E731
    a, b = run(training=True, augment=make()), run(training=True, augment=make())
    assert len(a) == len(b) == 3
    for x, y in zip(a, b):                                                      # the same seed gives the same batches
        assert tuple(x) == keys and x["left"].shape == (2, 3, 32, 48) and all(torch.equal(x[k], y[k]) for k in keys)
    other = run(training=True, augment=sa.Augmentation.us3d((32, 48), 16, p_occluder=0.0, seed=8))
    assert not all(torch.equal(x["left"], y["left"]) for x, y in zip(a, other))
    draws = make()                                                              # ... and they are augment_sample of the same draws
    for x, raw in zip(a, batches):
        want = sa.augment_sample(raw, draws.draw(2, 48, 64), keys, maxdisp=16)
        assert all(torch.equal(x[k], want[k]) for k in keys)
    plain, today = run(training=True, augment=None), run(training=True)
    for x, y, raw in zip(plain, today, batches):                                # augment=None: today's dictionaries
        ref = sa.prepare_sample(raw, True, keys)
        assert tuple(x) == tuple(ref) and all(torch.equal(x[k], ref[k]) and torch.equal(y[k], ref[k]) for k in keys)
    for x, raw in zip(run(training=False, augment=make()), batches):            # the test branch is never augmented
        ref = sa.prepare_sample(raw, False, keys)
        assert tuple(x) == tuple(ref) and all(torch.equal(x[k], ref[k]) for k in ("left", "right", "disparity", "label"))
