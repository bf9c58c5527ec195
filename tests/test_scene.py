"""CPU: scene inference (semstereo_amd/scene.py; the kernels are csrc/scene_tiles.hip) -- the properties of TilePlan, the PyTorch
composition of blend_tiles against the sequential per-pixel restatement of tests/scene_cases.py, tile_views against normalize_views,
SceneStereo around a per-pixel stand-in callable, and the ABI of the two entry points with their refusals (no GPU needed).  The two
kinds of input and their bounds are written down in scene_cases.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import scene_cases as sc
from abi import ROOT, declared, library

NAMES = ("ss_tile_views_fwd", "ss_tile_blend_fwd")
ALL = ("disparity", "logits", "label", "spread", "count")


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    return semstereo_amd


def moved(sa, before, key):
    return sa.modules.PATH_COUNTS.get(key, 0) - before.get(key, 0)


# 1 ------------------------------------------------------------------------------------------------------------------------------
def axis_plan(sa, S, T, overlap):
    return sa.TilePlan(S, 40, tile=(T, 32), overlap=(overlap, 0))


def test_plan_properties(sa):
    checked = 0
    for T in (32, 64, 96):
        for S in range(33, 301):
            for overlap in range(0, T // 2 + 1):
                te = min(T, -(-S // 32) * 32)                           # a scene shorter than the tile: round_up(S, 32)
                if overlap > te // 2:
                    with pytest.raises(ValueError):
                        axis_plan(sa, S, T, overlap)
                    continue
                plan = axis_plan(sa, S, T, overlap)
                assert plan.size == (te, 32)
                o = plan.origin_y
                assert o[0] == 0 and all(a < b for a, b in zip(o, o[1:])), (S, T, overlap, o)
                if S <= te:
                    assert o == (0,)
                else:
                    assert o[-1] + te == S
                cover = np.zeros(S, dtype=np.int64)
                for k in o:
                    cover[k:k + te] += 1
                assert cover.min() >= 1 and cover.max() <= 3, (S, T, overlap, o)
                bands = plan.bands
                assert len(bands) == len(o) and bands[0][0] == 0 and bands[-1][1] == S
                assert all(a[1] == b[0] for a, b in zip(bands, bands[1:])) and all(b[0] < b[1] for b in bands)
                for r, (y0, y1, rows) in enumerate(bands):
                    covering = {k for k, oy in enumerate(o) if oy < y1 and oy + te > y0}
                    assert covering == set(rows) and max(rows) == r and 1 <= len(rows) <= 3, (S, T, overlap, r, rows)
                # the residency of SceneStereo: tile row r + 1 is issued before band r is blended, a row is dropped after its last band
                held, peak = set(), 0
                for r in range(len(o) + 1):
                    if r < len(o):
                        held.add(r)
                        peak = max(peak, len(held))
                    if r:
                        assert set(bands[r - 1][2]) <= held
                        held -= {k for k in held if plan.last_use[k] <= r - 1}
                assert peak <= 3 and not held, (S, T, overlap, peak)
                checked += 1
    assert checked > 10000
    plan = sa.TilePlan(150, 203, tile=(64, 96), overlap=(24, 32), ramp=(16, 8))
    assert plan.origin_y == (0, 40, 80, 86) and plan.origin_x == (0, 64, 107) and plan.size == (64, 96) and len(plan) == 12
    assert plan.origins[4] == (40, 64) and plan.ramp == (16, 8)
    assert sa.TilePlan(150, 203, tile=64, overlap=0).ramp == (1, 1) and sa.TilePlan(150, 203, tile=64, overlap=24).ramp == (24, 24)
    assert sa.TilePlan(4096, 4096).size == (1024, 1024) and sa.TilePlan(4096, 4096).origin_y == (0, 768, 1536, 2304, 3072)


def test_plan_refuses_bad_sizes(sa):
    for bad in (dict(tile=(48, 64)), dict(tile=(64, 100)), dict(tile=0), dict(tile=64, overlap=(33, 0)), dict(tile=64, overlap=(0, 40)),
                dict(tile=64, overlap=-1), dict(tile=64, overlap=8, ramp=0)):
        with pytest.raises(ValueError):
            sa.TilePlan(150, 203, **bad)
    with pytest.raises(ValueError):                                     # the effective tile size is 64, not 1024
        sa.TilePlan(40, 300, tile=1024, overlap=(40, 0))
    sa.TilePlan(40, 300, tile=1024, overlap=(32, 160))


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(sa):
    plan = sa.TilePlan(44, 57, tile=32, overlap=(8, 16), ramp=(4, 8))
    assert plan.origin_y == (0, 12) and plan.origin_x == (0, 16, 25)
    return plan


def test_blend_composition_equals_the_restatement_exactly(sa, small):
    d, lg = sc.make_tiles(small, 6, "exact", seed=1)
    before = dict(sa.modules.PATH_COUNTS)
    got = sa.blend_tiles(small, d, lg, want=ALL)
    assert moved(sa, before, "scene_torch") == 1 and moved(sa, before, "scene_hip") == 0
    assert tuple(got) == ALL and got["label"].dtype == torch.uint8 and got["count"].dtype == torch.uint8
    assert got["logits"].shape == (6, 44, 57) and got["disparity"].dtype == torch.float32
    sc.check_exact(got, sc.restate(small, d, lg, np.float32), "fp32 restatement")
    sc.check_exact(got, sc.as_f32(sc.restate(small, d, lg, np.float64)), "float64 restatement rounded to fp32")
    assert int(got["count"].max()) == 6 and int(got["count"].min()) == 1
    assert bool((got["spread"][got["count"] == 1] == 0).all()) and float(got["spread"].max()) > 0
    # a list of tiles, a tile that is not resident, a row range into a given mosaic
    tiles, logits = list(d), list(lg)
    sc.check_exact(sa.blend_tiles(small, tiles, logits, want=ALL), got, "a list")
    tiles[0:3], logits[0:3] = [None] * 3, [None] * 3                   # tile row 0 is gone
    part = sa.blend_tiles(small, tiles, logits, rows=(32, 44), want=ALL)
    sc.check_exact(part, got, "rows (32, 44) without tile row 0", rows=(32, 44))
    assert all(int(part[k][..., :32, :].abs().sum()) == 0 for k in ALL)
    want = sc.restate(small, d, lg, np.float32, rows=(12, 32), resident=[False] * 3 + [True] * 3)
    sc.check_exact(sa.blend_tiles(small, tiles, logits, rows=(12, 32), want=ALL), want, "tile row 1 alone", rows=(12, 32))
    out = {k: torch.full_like(v, 77) for k, v in got.items()}
    back = sa.blend_tiles(small, d, lg, rows=(5, 20), out=out, want=ALL)
    assert all(back[k] is out[k] for k in ALL)
    sc.check_exact(back, got, "rows (5, 20)", rows=(5, 20))
    assert all(bool((out[k][..., :5, :] == 77).all()) and bool((out[k][..., 20:, :] == 77).all()) for k in ALL)
    only = sa.blend_tiles(small, d, want=("spread", "count"))
    assert tuple(only) == ("spread", "count")
    sc.check_exact(only, got, "without logits")
    with pytest.raises(AssertionError):
        sa.blend_tiles(small, d, want=("label",))


def test_blend_composition_meets_the_bound_on_float_tiles(sa, small):
    d, lg = sc.make_tiles(small, 6, "float", seed=2)
    got = sa.blend_tiles(small, d, lg, want=ALL)
    ref = {k: torch.from_numpy(v) for k, v in sc.restate(small, d, lg, np.float64).items()}
    sc.check_float(got, ref, (d, lg), "composition")
    sc.check_exact(got, sc.restate(small, d, lg, np.float32), "fp32 restatement")          # the same operations in the same order
    wide = sa.blend_tiles(small, d.double(), lg.double(), want=ALL)                        # other dtypes take the composition, in that dtype
    assert wide["disparity"].dtype == torch.float64
    sc.check_exact(wide, ref, "the float64 composition")


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_tile_views_on_the_cpu(sa):
    g = torch.Generator().manual_seed(3)
    left = torch.randint(0, 256, (70, 93, 3), generator=g, dtype=torch.uint8)
    right = torch.randint(0, 256, (70, 93, 3), generator=g, dtype=torch.uint8)
    origins = ((0, 0), (17, 21), (3, 40), (50, 10), (60, 80))
    before = dict(sa.modules.PATH_COUNTS)
    l, r = sa.tile_views(left, right, origins, (32, 64))
    assert moved(sa, before, "scene_torch") == 1 and l.shape == r.shape == (5, 3, 32, 64) and l.dtype == torch.float32
    for i, (oy, ox) in enumerate(origins):
        h, w = min(32, 70 - oy), min(64, 93 - ox)
        for got, scene in ((l, left), (r, right)):
            assert torch.equal(got[i, :, :h, :w], sa.normalize_views(scene[oy:oy + h, ox:ox + w].contiguous()))
            assert bool((got[i, :, h:, :] == 0).all()) and bool((got[i, :, :, w:] == 0).all())
    assert sum(int((l[i] == 0).all(0).sum()) for i in range(5)) > 0
    one = sa.tile_views(left, None, origins[:2], (32, 64))
    assert isinstance(one, torch.Tensor) and torch.equal(one, l[:2])
    off = sa.tile_views(left, None, ((-5, -7), (200, 0)), (32, 32))                     # any origin: before the scene, off it
    assert torch.equal(off[0, :, 5:, 7:], sa.normalize_views(left[:27, :25].contiguous())) and bool((off[0, :, :5] == 0).all())
    assert bool((off[0, :, :, :7] == 0).all()) and bool((off[1] == 0).all())


# 4 ------------------------------------------------------------------------------------------------------------------------------
COMBOS = torch.tensor([[1.0, 0.5, -0.25], [-0.5, 1.0, 0.25], [0.25, -1.0, 0.5], [0.75, 0.25, -1.0], [-1.0, 0.5, 0.5], [0.5, -0.75, 1.0]])


def per_pixel_model(left, right):
    """A callable with the reference's eval convention whose answer at a pixel depends on that pixel alone."""
    disp = 3.0 * (left[:, 0] - right[:, 0])
    mix = torch.stack([left[:, 0], right[:, 1], left[:, 2] - right[:, 2]], dim=1)                 # [B,3,h,w]
    logits = torch.stack([sum(float(COMBOS[k, c]) * mix[:, c] for c in range(3)) for k in range(6)], dim=1)
    return [disp], logits


def test_scene_stereo_with_a_per_pixel_callable(sa):
    g = torch.Generator().manual_seed(4)
    H, W = 150, 203
    left = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    right = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    stereo = sa.SceneStereo(per_pixel_model, tile=(64, 96), overlap=(24, 32), batch=2)
    got = stereo(left, right, want=ALL)
    plan = stereo.plan
    assert plan.origin_y == (0, 40, 80, 86) and plan.origin_x == (0, 64, 107) and plan.ramp == (24, 32)
    assert 1 <= stereo.peak_resident_tile_rows <= 3
    assert all(got[k].shape[-2:] == (H, W) for k in ALL) and got["logits"].shape[0] == 6
    # the same callable on the whole padded scene: every tile holds the scene's own value at a pixel, so the blend may only round
    pl, pr = sa.tile_views(left, right, ((0, 0),), (160, 224))
    (whole,), whole_logits = per_pixel_model(pl, pr)
    err = float((got["disparity"] - whole[0, :H, :W]).abs().max())
    err_l = float((got["logits"] - whole_logits[0, :, :H, :W]).abs().max())
    print(f"disparity within {err:.3e} (bound {sc.bound(whole):.3e}), logits within {err_l:.3e} (bound {sc.bound(whole_logits):.3e})")
    assert err <= sc.bound(whole) and err_l <= sc.bound(whole_logits)
    assert bool((got["spread"][got["count"] == 1] == 0).all()) and float(got["spread"].max()) <= sc.bound(whole)
    assert int(got["count"].min()) == 1 and int(got["count"].max()) == 6
    # band by band equals one blend over all tiles resident
    tl, tr = sa.tile_views(left, right, plan.origins, plan.size)
    (d,), lg = per_pixel_model(tl, tr)
    sc.check_exact(got, sa.blend_tiles(plan, d, lg, want=ALL), "banded against one blend")
    # without a segmentation head
    plain = sa.SceneStereo(lambda a, b: per_pixel_model(a, b)[0], tile=(64, 96), overlap=(24, 32))
    out = plain(left, right, want=("disparity", "count"))
    assert torch.equal(out["disparity"], got["disparity"]) and torch.equal(out["count"], got["count"])
    with pytest.raises(AssertionError):
        plain(left, right)                                              # the default asks for a label


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported(sa):
    _l, lib = library()
    decl = declared()
    for name in NAMES:
        assert name in decl and name in _l._SIGNATURES and name in _l.EXPORTS, name
        assert len(_l._SIGNATURES[name]) == len(decl[name][1]), name
        assert hasattr(lib, name) and decl[name][1][-1] == "ss_stream_t", name
    assert len(decl["ss_tile_views_fwd"][1]) == 12 and len(decl["ss_tile_blend_fwd"][1]) == 21
    assert decl["ss_tile_blend_fwd"][1][:2] == ["const long long*", "const long long*"]
    assert _l.ABI_VERSION == 20 and lib.ss_abi_version() == 20          # symbols were added, nothing changed
    assert not [n for n in _l.EXPORTS if "tile" in n and n.endswith("_workspace_bytes")]
    srcs = re.search(r"^SRCS_HIP\s*:=(.*)$", open(os.path.join(ROOT, "semstereo_amd", "csrc", "Makefile")).read(), flags=re.M).group(1)
    assert "scene_tiles.hip" in srcs.split()
    assert "SCENE_HIP" in sa.engine.SWITCHES and isinstance(sa.engine.SCENE_HIP, bool)
    assert sa.SceneStereo is sa.scene.SceneStereo and sa.TilePlan is sa.scene.TilePlan
    assert sa.blend_tiles is sa.scene.blend_tiles and sa.tile_views is sa.scene.tile_views


def test_the_source_only_launches():
    text = open(os.path.join(ROOT, "semstereo_amd", "csrc", "scene_tiles.hip")).read()
    for word in ("hipMemcpy", "hipMemset", "Synchronize", "hipMalloc", "hipFree", "hipEvent", "atomicAdd", "atomicMax", "atomicCAS", "__hip_atomic", "printf", "assert(", "asm", "__frcp", "__fdividef"):
        assert word not in text, word
    flags = re.search(r"^CXXFLAGS\s*:=(.*)$", open(os.path.join(ROOT, "semstereo_amd", "csrc", "Makefile")).read(), flags=re.M).group(1)
    assert "fast-math" not in flags and "-Ofast" not in flags           # num / den is an IEEE division


def test_bad_arguments_are_refused_before_any_device_call():
    _l, lib = library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                               # pointers that are never followed

    def views(left=p, right=p, origins=p, table=p, n=5, th=32, tw=64, H=70, W=93, ol=p, orr=p):
        return lib.ss_tile_views_fwd(left, right, origins, table, n, th, tw, H, W, ol, orr, None)

    def blend(dt=p, lt=p, oy=p, ox=p, nty=4, ntx=3, th=64, tw=96, C=6, ry=16, rx=8, H=150, W=203, y0=0, y1=150, outs=(p, p, p, p, p)):
        return lib.ss_tile_blend_fwd(dt, lt, oy, ox, nty, ntx, th, tw, C, ry, rx, H, W, y0, y1, *outs, None)
    assert views(left=None) == -1 and views(origins=None) == -1 and views(table=None) == -1 and views(ol=None) == -1
    assert views(right=None) == -1 and views(orr=None) == -1            # the right view and its output come together
    assert views(n=0) == -1 and views(th=0) == -1 and views(tw=-1) == -1 and views(H=0) == -1 and views(W=0) == -1
    assert views(H=1 << 15, W=1 << 15) == -2                            # 3 * 2^30 bytes of scene
    assert views(n=64, th=4096, tw=4096) == -2                          # 2^31 elements of output
    assert views(n=64, th=4096, tw=4096, table=None) == -1              # -1 comes first
    assert blend(dt=None) == -1 and blend(oy=None) == -1 and blend(ox=None) == -1
    assert blend(outs=(None,) * 5) == -1                                # nothing asked for
    assert blend(lt=None) == -1 and blend(C=0) == -1                    # the logits table is NULL exactly when C is 0
    assert blend(lt=None, C=0, outs=(p, None, p, p, p)) == -1 and blend(lt=None, C=0, outs=(p, p, None, p, p)) == -1
    assert blend(th=0) == -1 and blend(tw=0) == -1 and blend(th=-64) == -1 and blend(nty=0) == -1 and blend(ntx=0) == -1
    assert blend(ry=0) == -1 and blend(rx=0) == -1 and blend(rx=-3) == -1
    assert blend(y0=10, y1=9) == -1 and blend(y0=-1) == -1 and blend(y1=151) == -1
    assert blend(C=9) == -2 and blend(nty=257) == -2 and blend(ntx=257) == -2
    assert blend(H=1 << 15, W=1 << 15, y1=1, C=2) == -2                 # 2^31 elements of logits
    assert blend(H=1 << 16, W=1 << 15, y1=1, lt=None, C=0, outs=(p, None, None, p, p)) == -2
    assert blend(th=1 << 14, tw=1 << 14, C=8) == -2                     # ... of a logit tile
    assert blend(C=9, ry=0) == -1                                       # -1 comes first
    assert blend(y0=7, y1=7) == 0                                       # an empty range: nothing to launch
