"""Sample preparation on the HIP kernels (csrc/sample_prep.hip; reference datasets/us3d_.py:70-215, datasets/whu_dataset.py:42-92): every
fixture case against the reference's record (tests/golden/data.npz), other shapes against the PyTorch composition on the CPU, one
full-size batch, repeatability, routing, no host wait and the stream order of DeviceLoader.  Run on the MI355X box: pytest -m gpu.

Criteria, the same as on the CPU (tests/test_data_golden.py): views, pyramid levels, `disparity` and `label` are torch.equal -- table
lookups, copies and exact widenings, no arithmetic that could round differently.  gx / gy are within 1 float32 ulp with NaN in the same
places: against the fixture because numpy's np.std is an ulp of double from the exact-integer form; against the composition because the
device's double division and square root are expected, not known, to round as the host's do.  The count of unequal pixels is in the
assertion message.

No host wait: the calls run under torch.cuda.set_sync_debug_mode("error"), which raises on a synchronising call of torch; the library's
own launches are outside its view, and csrc/sample_prep.hip holds no synchronising or copying call (tests/test_data_abi.py reads it)."""
import os

import numpy as np
import pytest
import torch

from golden import data_cases as dc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return semstereo_amd


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "data.npz"))


class counted:
    """The calls inside make `hip` calls on the kernels and `torch_` on the composition."""

    def __init__(self, sa, hip, torch_=0):
        self.sa, self.hip, self.torch = sa, hip, torch_

    def __enter__(self):
        self.before = dict(self.sa.modules.PATH_COUNTS)

    def __exit__(self, *exc):
        if exc[0] is None:
            torch.cuda.synchronize()
            pc = self.sa.modules.PATH_COUNTS
            assert pc.get("data_hip", 0) == self.before.get("data_hip", 0) + self.hip, "data_hip"
            assert pc.get("data_torch", 0) == self.before.get("data_torch", 0) + self.torch, "data_torch"
            assert pc["hip"] == self.before["hip"] and pc["torch"] == self.before["torch"]


def same(got, want, what):
    assert got.is_cuda and got.dtype == want.dtype and got.shape == want.shape, what
    got = got.cpu()
    assert torch.equal(got, want), f"{what}: {(got != want).sum().item()} of {want.numel()} values differ"


def cuda(raw):
    """The arrays on the device; pads and file names stay where they are, as in DeviceLoader."""
    return {k: v.cuda() if isinstance(v, torch.Tensor) and v.dim() >= 3 else v for k, v in raw.items()}


def _views(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8), torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8))


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(dc.CASES))
def test_fixture_cases(sa, fx, name):
    from test_data_golden import check_case
    c = dc.CASES[name]
    raw = cuda(dc.raw_inputs(name))
    training = dc.has_training_branch(name)
    divisible = c["H"] % 16 == 0 and c["W"] % 16 == 0
    with counted(sa, 3 if divisible else 2, 0 if divisible else 1):     # the pyramid of other sizes is the composition's
        sample = sa.prepare_sample(raw, training)
    assert all(v.is_cuda for v in sample.values() if isinstance(v, torch.Tensor))
    check_case(sample, fx, name)


# 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 2, 37])
@pytest.mark.parametrize("W", [1, 3, 4, 5, 53, 64])
def test_views_equal_the_composition(sa, H, W):
    left, right = _views(2, H, W, 6000 + 100 * H + W)
    want_l, want_r = sa.normalize_views(left, right)
    with counted(sa, 2):
        got_l, got_r = sa.normalize_views(left.cuda(), right.cuda())
        one = sa.normalize_views(right.cuda()[1])                      # one view, one image
    same(got_l, want_l, f"left 2x{H}x{W}")
    same(got_r, want_r, f"right 2x{H}x{W}")
    same(one, want_r[1], f"right[1] {H}x{W}")


def test_a_view_that_is_not_contiguous_takes_the_composition(sa):
    left, right = _views(2, 24, 40, 6500)
    wide = torch.cat([right, right], dim=2).cuda()
    crop = wide[:, :, 40:]                                              # the right view as a view into a wider tensor
    assert not crop.is_contiguous()
    with counted(sa, 0, 1):
        got_l, got_r = sa.normalize_views(left.cuda(), crop)
    want_l, want_r = sa.normalize_views(left, right)
    same(got_l, want_l, "left")
    same(got_r, want_r, "right, cropped")


# 3 ------------------------------------------------------------------------------------------------------------------------------
def _maps(B, H, W, seed, dtype, pad=(0, 0)):
    g = torch.Generator().manual_seed(seed)
    disp = 120 * torch.rand(B, H, W, generator=g) - 60
    big = torch.randint(0, 6, (B, H + pad[0], W + pad[1]), generator=g).to(dtype)
    return disp, big


@pytest.mark.parametrize("shape", [(16, 16), (32, 48), (64, 16)])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64, torch.float32])
def test_pyramids_equal_the_composition(sa, shape, dtype):
    H, W = shape
    disp, big = _maps(2, H, W, 6600 + H + W, dtype, pad=(3, 5))
    label = big[:, 2:2 + H, 4:4 + W]                                   # a strided crop, first pixel at an odd offset
    want = sa.nearest_pyramid(disp, label)
    with counted(sa, 1):
        got = sa.nearest_pyramid(disp.cuda(), big.cuda()[:, 2:2 + H, 4:4 + W])
    assert set(got) == set(want) == {"disparity", "disparity_4", "disparity_8", "disparity_16", "label", "label_2", "label_4"}
    for k in want:
        same(got[k], want[k], f"{k} {H}x{W} {dtype}")
    assert got["label"].dtype == torch.float32 and got["disparity_16"].shape == (2, H // 16, W // 16)


def test_pyramid_levels_left_out_and_the_whu_source(sa):
    disp, big = _maps(2, 32, 48, 6700, torch.uint8)
    d, y = disp.cuda(), big.cuda()
    with counted(sa, 3):
        a = sa.nearest_pyramid(d, y, disp_levels=(4,), label_levels=())              # null pointers for the other levels
        b = sa.nearest_pyramid(d, None, disp_levels=(16, 8))                          # no label source at all
        c = sa.nearest_pyramid(d, y, disp_levels=(), label_levels=(2,))
    assert set(a) == {"disparity", "disparity_4", "label"} and set(b) == {"disparity", "disparity_8", "disparity_16"}
    assert set(c) == {"disparity", "label", "label_2"} and a["disparity"] is d
    full = sa.nearest_pyramid(disp, big)
    for got in (a, b, c):
        for k, v in got.items():
            same(v, full[k], k)
    raw = torch.randint(0, 65536, (2, 32, 48), generator=torch.Generator().manual_seed(6701), dtype=torch.int32)
    want = sa.nearest_pyramid(raw, disp_scale=1 / 256)
    with counted(sa, 1):
        got = sa.nearest_pyramid(raw.cuda(), disp_scale=1 / 256)
    assert torch.equal(want["disparity"], raw.float() / 256)
    for k in want:
        same(got[k], want[k], f"whu {k}")


def test_sizes_sixteen_does_not_divide_take_the_composition(sa):
    disp, big = _maps(1, 37, 53, 6800, torch.uint8)
    with counted(sa, 0, 1):
        got = sa.nearest_pyramid(disp.cuda(), big.cuda())
    want = sa.nearest_pyramid(disp, big)
    for k in want:
        same(got[k], want[k], k)


# 4 ------------------------------------------------------------------------------------------------------------------------------
def _gradients_check(sa, left, what, hip=1):
    want_x, want_y = sa.image_gradients(left)
    with counted(sa, hip):
        got_x, got_y = sa.image_gradients(left.cuda())
    assert got_x.is_cuda and got_x.shape == want_x.shape and got_y.shape == want_y.shape
    n = dc.assert_gradients(got_x, want_x, what + " gx") + dc.assert_gradients(got_y, want_y, what + " gy")
    print(f"{what}: {n} of {2 * want_x.numel()} values unequal (all within 1 ulp)")
    return got_x, got_y, want_x, want_y


@pytest.mark.parametrize("shape", [(1, 5), (5, 1), (37, 53), (64, 64)])
def test_gradients_equal_the_composition(sa, shape):
    left, _ = _views(1, shape[0], shape[1], 6900 + shape[0])
    _gradients_check(sa, left, f"{shape[0]}x{shape[1]}")


def test_gradients_of_one_pixel_and_of_a_constant_image(sa):
    """std = 0: NaN on every pixel, borders included, on both paths."""
    one, _ = _views(1, 1, 1, 6950)
    flat = torch.empty(2, 16, 20, 3, dtype=torch.uint8)
    flat[0], flat[1] = 77, torch.tensor([1, 200, 30], dtype=torch.uint8)
    for left, what in ((one, "1x1"), (flat, "constant")):
        gx, gy, wx, wy = _gradients_check(sa, left, what)
        assert bool(torch.isnan(wx).all()) and bool(torch.isnan(wy).all()) and bool(torch.isnan(gx).all()) and bool(torch.isnan(gy).all())


def test_gradients_take_the_statistics_per_image(sa):
    g = torch.Generator().manual_seed(7000)
    left = torch.stack([torch.randint(20, 44, (24, 40, 3), generator=g), torch.randint(0, 256, (24, 40, 3), generator=g),
                        torch.randint(200, 256, (24, 40, 3), generator=g)]).to(torch.uint8)
    gx, gy, _, _ = _gradients_check(sa, left, "batch of 3")
    for i in range(3):                                                  # each image alone gives the image of the batch
        ax, ay = sa.image_gradients(left[i:i + 1].cuda())
        assert torch.equal(ax, gx[i:i + 1]) and torch.equal(ay, gy[i:i + 1]), i


def test_gradients_where_the_sum_of_squares_passes_32_bits(sa):
    left = torch.zeros(1, 512, 512, 3, dtype=torch.uint8)
    left[:, :, :256] = 255
    assert 255 * 255 * 512 * 256 > 2 ** 32
    gx, gy, wx, wy = _gradients_check(sa, left, "512x512 halves")
    # mean 127.5, std 127.5: z = +-1 exactly, so the step in the middle is 2 and the two borders 1 and -1
    assert gx[0, 0, 7, 255].item() == 2.0 and gx[0, 0, 7, 256].item() == 2.0 and gx[0, 0, 7, 0].item() == -1.0 and gx[0, 0, 7, 511].item() == -1.0
    assert gy[0, 0, 0, 3].item() == -1.0 and gy[0, 0, 511, 3].item() == 1.0 and not bool(gy[0, 0, 1:-1].any())


def test_two_calls_give_the_same_bits(sa):
    left, right = _views(2, 75, 203, 7050)
    raw = cuda({"left_u8": left, "right_u8": right, "disparity": torch.randn(2, 75, 203), "label": torch.randint(0, 6, (2, 75, 203))})
    a, b = sa.prepare_sample(raw, True), sa.prepare_sample(raw, True)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k


# 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """A batch of 4 at 1024 x 1024 with the composition's sample, computed once on the CPU."""
    import semstereo_amd as sa
    left, right = _views(4, 1024, 1024, 7100)
    g = torch.Generator().manual_seed(7101)
    raw = {"left_u8": left, "right_u8": right, "disparity": 120 * torch.rand(4, 1024, 1024, generator=g) - 60,
           "label": torch.randint(0, 6, (4, 1024, 1024), generator=g, dtype=torch.uint8)}
    return raw, sa.prepare_sample(raw, True)


def test_full_size_equals_the_composition(sa, big):
    raw, want = big
    with counted(sa, 3):
        got = sa.prepare_sample(cuda(raw), True)
    assert list(got) == list(want)
    for k, v in want.items():
        if k in dc.GRAD_KEYS:
            n = dc.assert_gradients(got[k], v, f"{k} 4x1024x1024")
            print(f"{k} 4x1024x1024: {n} values unequal")
        else:
            same(got[k], v, f"{k} 4x1024x1024")


# 6 ------------------------------------------------------------------------------------------------------------------------------
def _pinned_batches(n, B, H, W, seed, training=True):
    out = []
    for i in range(n):
        left, right = _views(B, H, W, seed + i)
        g = torch.Generator().manual_seed(seed + 50 + i)
        raw = {"left_u8": left, "right_u8": right, "disparity": 120 * torch.rand(B, H, W, generator=g) - 60,
               "label": torch.randint(0, 6, (B, H, W), generator=g, dtype=torch.uint8)}
        raw = {k: v.pin_memory() for k, v in raw.items()}
        if not training:
            raw.update(top_pad=torch.zeros(B, dtype=torch.int64), right_pad=torch.zeros(B, dtype=torch.int64), left_filename=[f"{i}.tif"] * B)
        out.append(raw)
    return out


def test_no_host_wait(sa):
    batches = _pinned_batches(3, 2, 64, 96, 7200)
    raw = cuda(batches[0])
    sa.prepare_sample(raw, True)                                        # (library load, the table's upload, the workspace query)
    loader = sa.DeviceLoader(batches, training=True)
    it = iter(loader)
    next(it)                                                            # (the side stream)
    torch.cuda.synchronize()
    with counted(sa, 3 + 3):
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = sa.prepare_sample(raw, True)
            step = next(it)                                             # prepares batch 2, hands out batch 1
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(out["gx"]).all()) and step["left"].is_cuda
    assert len(list(it)) == 1


def test_routing(sa, monkeypatch):
    left, right = _views(2, 32, 48, 7300)
    raw = cuda({"left_u8": left, "right_u8": right, "disparity": torch.randn(2, 32, 48), "label": torch.randint(0, 6, (2, 32, 48))})
    with counted(sa, 3):
        on = sa.prepare_sample(raw, True)
    monkeypatch.setattr(sa.engine, "DATA_HIP", False)
    with counted(sa, 0, 3):
        off = sa.prepare_sample(raw, True)
    monkeypatch.setattr(sa.engine, "DATA_HIP", True)
    for k in on:
        assert off[k].is_cuda and off[k].shape == on[k].shape and off[k].dtype == on[k].dtype, k
        if k not in dc.GRAD_KEYS:                                       # lookups and copies: the same on any path and device
            assert torch.equal(on[k], off[k]), k
    with counted(sa, 0, 2):                                             # oddly typed inputs keep the composition
        sa.normalize_views(raw["left_u8"].to(torch.int32))
        sa.nearest_pyramid(raw["disparity"].double(), raw["label"])
    with counted(sa, 2):                                                # the five keys of a training script: no gradients
        sub = sa.prepare_sample(raw, True, keys=("left", "right", "disparity", "disparity_4", "label"))
    assert tuple(sub) == ("left", "right", "disparity", "disparity_4", "label")


@pytest.mark.parametrize("training", [True, False])
def test_device_loader_hands_batches_over_in_stream_order(sa, training):
    batches = _pinned_batches(3, 2, 128, 160, 7400, training)
    want = [sa.prepare_sample(cuda(b), training) for b in batches]
    torch.cuda.synchronize()
    got = []
    for sample in sa.DeviceLoader(batches, training=training):
        got.append({k: (v * 1 if isinstance(v, torch.Tensor) and v.is_cuda else v) for k, v in sample.items()})   # consumed at once, on this stream
    assert len(got) == 3
    for a, b in zip(got, want):
        assert list(a) == list(b)
        for k, v in b.items():
            if isinstance(v, torch.Tensor) and v.is_cuda:
                assert a[k].is_cuda and torch.equal(a[k], v), k
            elif isinstance(v, torch.Tensor):
                assert torch.equal(a[k], v), k
            else:
                assert a[k] == v, k
    assert got[0]["left"].data_ptr() == got[0]["left"].cuda().data_ptr()                # `.cuda()` in train_sample is a no-op
