"""Scene inference on the HIP kernels (csrc/scene_tiles.hip): tile_views against the composition, ss_tile_blend_fwd against the CPU
composition on exact inputs (all five outputs bit for bit: with and without logits, tiles of a batch tensor, a row range into a
pre-filled mosaic, a tile row that is not resident) and within the bound on float inputs, repeatability, and SceneStereo end to end
around the stand-in model on a PairPipeline.  Run on the MI355X box: pytest -m gpu.  The two kinds of input, the bound and the label
rule are written down in tests/scene_cases.py; the references are computed once per module on the CPU."""
import os

import pytest
import torch

import scene_cases as sc

pytestmark = pytest.mark.gpu

ALL = ("disparity", "logits", "label", "spread", "count")
SENTINEL = 77


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return semstereo_amd


class counted:
    """The calls inside make `hip` calls on the kernels and `torch_` on the composition."""

    def __init__(self, sa, hip, torch_=0):
        self.sa, self.hip, self.torch = sa, hip, torch_

    def __enter__(self):
        self.before = dict(self.sa.modules.PATH_COUNTS)

    def __exit__(self, *exc):
        if exc[0] is None:
            pc = self.sa.modules.PATH_COUNTS
            assert pc.get("scene_hip", 0) == self.before.get("scene_hip", 0) + self.hip, "scene_hip"
            assert pc.get("scene_torch", 0) == self.before.get("scene_torch", 0) + self.torch, "scene_torch"
            assert pc["torch"] == self.before["torch"]


# 1 ------------------------------------------------------------------------------------------------------------------------------
def test_tile_views_kernel_equals_the_composition(sa):
    g = torch.Generator().manual_seed(11)
    left = torch.randint(0, 256, (70, 93, 3), generator=g, dtype=torch.uint8)       # a width that 4 does not divide: rows of 279 bytes
    right = torch.randint(0, 256, (70, 93, 3), generator=g, dtype=torch.uint8)
    origins = ((0, 0), (17, 21), (3, 40), (50, 10), (60, 80))                        # aligned, odd, over the right edge, the bottom, both
    want_l, want_r = sa.tile_views(left, right, origins, (32, 64))
    with counted(sa, 2):
        got_l, got_r = sa.tile_views(left.cuda(), right.cuda(), origins, (32, 64))
        one = sa.tile_views(right.cuda(), None, origins[1:3], (32, 64))             # one view only
    assert got_l.is_cuda and got_l.shape == (5, 3, 32, 64) and got_l.dtype == torch.float32
    assert torch.equal(got_l.cpu(), want_l) and torch.equal(got_r.cpu(), want_r)
    assert isinstance(one, torch.Tensor) and torch.equal(one.cpu(), want_r[1:3])
    assert bool((got_l[4, :, 10:, :] == 0).all()) and bool((got_l[4, :, :, 13:] == 0).all())
    sa.engine.SCENE_HIP = False
    try:
        with counted(sa, 0, 1):
            comp = sa.tile_views(left.cuda(), right.cuda(), origins, (32, 64))
    finally:
        sa.engine.SCENE_HIP = True
    assert torch.equal(comp[0], got_l) and torch.equal(comp[1], got_r)


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan(sa):
    p = sa.TilePlan(150, 203, tile=(64, 96), overlap=(24, 32), ramp=(16, 8))
    assert p.origin_y == (0, 40, 80, 86) and p.origin_x == (0, 64, 107)             # pixels under 6 tiles, windows 6 rows apart
    return p


@pytest.fixture(scope="module")
def exact(sa, plan):
    """(disparity tiles, logit tiles, the CPU composition of all five outputs) on exact inputs."""
    d, lg = sc.make_tiles(plan, 6, "exact", seed=21)
    return d, lg, sa.blend_tiles(plan, d, lg, want=ALL)


def test_blend_kernel_is_exact_on_exact_inputs(sa, plan, exact):
    d, lg, want = exact
    assert int(want["count"].max()) == 6 and int(want["count"].min()) == 1
    with counted(sa, 1):
        got = sa.blend_tiles(plan, [t.clone() for t in d.cuda()], [t.clone() for t in lg.cuda()], want=ALL)      # tiles allocated one by one
    assert all(got[k].is_cuda for k in ALL)
    sc.check_exact(got, want, "all five outputs")
    with counted(sa, 1):                                                # C = 0: the logits table is NULL
        plain = sa.blend_tiles(plan, d.cuda(), want=("disparity", "spread", "count"))
    assert tuple(plain) == ("disparity", "spread", "count")
    sc.check_exact(plain, want, "without logits")
    with counted(sa, 2):                                                # tiles of a batch tensor: the addresses sit at b * stride
        batch = sa.blend_tiles(plan, d.cuda(), lg.cuda(), want=ALL)
        single = sa.blend_tiles(plan, d.cuda(), lg.cuda(), want=("label",))      # one output alone reads the logits too
    sc.check_exact(batch, want, "tiles of a batch tensor")
    assert tuple(single) == ("label",)
    sc.check_exact(single, want, "the label alone")


def test_blend_kernel_writes_only_the_rows_of_the_range(sa, plan, exact):
    d, lg, want = exact
    out = {k: torch.full_like(v, SENTINEL).cuda() for k, v in want.items()}
    with counted(sa, 1):
        back = sa.blend_tiles(plan, d.cuda(), lg.cuda(), rows=(40, 86), out=out, want=ALL)
    assert all(back[k] is out[k] for k in ALL)
    sc.check_exact(back, want, "rows (40, 86)", rows=(40, 86))
    for k in ALL:
        assert bool((out[k][..., :40, :] == SENTINEL).all()) and bool((out[k][..., 86:, :] == SENTINEL).all()), k
    # tile row 0 covers rows 0 .. 63: it is not resident (address 0), and the range does not need it
    tiles, logits = list(d.cuda()), list(lg.cuda())
    tiles[0:3], logits[0:3] = [None] * 3, [None] * 3
    with counted(sa, 1):
        part = sa.blend_tiles(plan, tiles, logits, rows=(64, 150), want=ALL)
    sc.check_exact(part, want, "rows (64, 150) without tile row 0", rows=(64, 150))
    assert all(int(part[k][..., :64, :].abs().sum()) == 0 for k in ALL)
    # ... and a range that would need it sees the resident tiles only, as the composition does
    with counted(sa, 1):
        lower = sa.blend_tiles(plan, tiles, logits, rows=(40, 64), want=ALL)
    sc.check_exact(lower, sa.blend_tiles(plan, [None] * 3 + list(d[3:]), [None] * 3 + list(lg[3:]), rows=(40, 64), want=ALL),
                   "rows (40, 64) from tile rows 1 ..", rows=(40, 64))


def test_blend_kernel_meets_the_bound_on_float_inputs(sa, plan):
    d, lg = sc.make_tiles(plan, 6, "float", seed=22)
    ref = sa.blend_tiles(plan, d.double(), lg.double(), want=ALL)       # the float64 composition
    with counted(sa, 1):
        got = sa.blend_tiles(plan, d.cuda(), lg.cuda(), want=ALL)
    sc.check_float(got, ref, (d, lg), "kernel")
    sc.check_float(sa.blend_tiles(plan, d, lg, want=ALL), ref, (d, lg), "fp32 composition")
    with counted(sa, 1):                                                # two calls: the same bits on every output
        again = sa.blend_tiles(plan, d.cuda(), lg.cuda(), want=ALL)
    sc.check_exact(again, got, "the second call")


# 3 ------------------------------------------------------------------------------------------------------------------------------
def _standin(sa):
    import standin_model
    from oracle import detdata as dd
    net = standin_model.StandInSemStereo(64, sa.modules)
    with torch.no_grad():
        for i, (name, t) in enumerate(sorted(list(net.named_parameters()) + list(net.named_buffers()))):
            if name.endswith("num_batches_tracked") or name in ("gamma", "beta"):
                continue
            if name.endswith("running_var") or (name.endswith(".weight") and t.dim() == 1):
                t.copy_(dd.t_uniform(tuple(t.shape), 900 + i, 0.6, 1.4))
            elif t.dim() == 1:
                t.copy_(dd.t_uniform(tuple(t.shape), 900 + i, -0.1, 0.1))
            else:
                fan_in = t.shape[0] * 27 // 8 if (".conv5.0." in name or ".conv6.0." in name) else t[0].numel()
                t.copy_(dd.t_uniform(tuple(t.shape), 900 + i, -(3.0 / fan_in) ** 0.5, (3.0 / fan_in) ** 0.5))
    return net.cuda().eval(), standin_model


def test_scene_stereo_end_to_end(sa):
    net, module = _standin(sa)
    previous = sa.install(module)
    try:
        sa.accelerate(net)
        _end_to_end(sa, net)
    finally:
        sa.uninstall(module, previous)


def _end_to_end(sa, net):
    g = torch.Generator().manual_seed(31)
    H, W = 160, 224
    left = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    right = torch.roll(left, shifts=-3, dims=1)
    two = sa.SceneStereo(net, tile=128, overlap=32, lanes=2)
    one = sa.SceneStereo(net, tile=128, overlap=32, lanes=1)
    try:
        two(left, right, want=ALL)                                      # (weight packing, the lanes' allocator pools: set-up)
        one(left.cuda(), right.cuda(), want=ALL)
        lc, rc = left.cuda(), right.cuda()
        torch.cuda.synchronize()
        before = dict(sa.modules.PATH_COUNTS)
        torch.cuda.set_sync_debug_mode("error")                         # a synchronising call of torch raises from here on
        try:
            got = two(lc, rc, want=ALL)
            same = one(lc, rc, want=ALL)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        plan = two.plan
        assert plan.origin_y == (0, 32) and plan.origin_x == (0, 96) and plan.size == (128, 128) and plan.ramp == (32, 32)
        assert 1 <= two.peak_resident_tile_rows <= 3
        assert sa.modules.PATH_COUNTS["torch"] == before["torch"]
        assert sa.modules.PATH_COUNTS["scene_hip"] == before["scene_hip"] + 2 * (2 + 2) and sa.modules.PATH_COUNTS.get("scene_torch", 0) == before.get("scene_torch", 0)
        # a plain call of the model on the first window of tile_views' output
        views = sa.tile_views(lc, rc, plan.origins[:1], plan.size)
        with torch.no_grad():
            (d0,), lg0 = net(*views)
        # (the final comparison: nothing waited on the host before this line)
        sc.check_exact(same, got, "lanes = 1 against lanes = 2")
        assert all(bool(torch.isfinite(got[k]).all()) for k in ("disparity", "logits", "spread")) and int(got["label"].max()) < 6
        assert got["logits"].shape == (6, H, W) and got["disparity"].shape == (H, W)
        alone = (got["count"] == 1)[:128, :128]
        assert bool(alone[:32, :96].all()) and not bool(alone[32:, :].any()) and not bool(alone[:, 96:].any())
        assert torch.equal(got["disparity"][:32, :96], d0[0, :32, :96]) and torch.equal(got["logits"][:, :32, :96], lg0[0, :, :32, :96])
        assert bool((got["spread"][got["count"] == 1] == 0).all())
        assert int(got["count"].max()) == 4 and int(got["count"].min()) == 1
    finally:
        two.close()
        one.close()
