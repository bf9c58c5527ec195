"""Range tests of every kernel on the two-term fp16 block-floating form (semstereo_amd/csrc/split_f16.h): operands far apart in
magnitude, in a chosen order, so that a stale block exponent, an accumulator set left out of a rescale or a maximum taken over the
wrong values costs decades and not bits.  Every case against a float64 CPU layer on seeded inputs.

  * the 2-D kernels (conv2d_k1_f16s, deconv2d_bf16s, conv2d_bf16s and its concat-free form, seghead_f16s): the element-wise bound of
    tests/f16_model.py (tests/test_f16_model.py holds a numpy model of the protocol to it, and four wrong models out of it);
  * the 3-D kernels (conv3d_bf16s in its stride-1 tiles, stride-2 forms, persistent walk, gathered stem and one-pass classifier;
    deconv3d_bf16s): the criterion the project has for this engine -- the error relative to the rms of each (batch element, output
    channel) of the float64 result is at most 1.5 x that of the exact-fp32 kernel on the same inputs, + 1e-6.

Which instantiation a case reaches is asserted from the launchers' selection rules restated here (as tests/test_fill_hint_gpu.py
does), never by looking at a kernel.  Every figure is printed; set SS_F16_RANGE_ERR_OUT=<file> to keep the table (profiles/f16_range_err.txt is a copy of one run).
Run on the MI355X box: pytest -m gpu."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f16_model as fm

pytestmark = pytest.mark.gpu

ALL = sorted(fm.ALL_RANGE_CASES)
CHANNEL = list(fm.CHANNEL_CASES)
RAMPS = list(fm.RAMP_CASES)
CHANNEL_AND_TENSOR = CHANNEL + list(fm.TENSOR_CASES)

_TABLE = []


def _record(what, err, share, of):
    line = f"{what:86s} err {err:.3e}   {share:8.3f} of {of}"
    print(line)
    _TABLE.append(line)


@pytest.fixture(scope="module", autouse=True)
def _dump_table():
    yield
    path = os.environ.get("SS_F16_RANGE_ERR_OUT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(_TABLE) + "\n")


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    assert semstereo_amd.engine.CONV_ENGINE == "f16x3"
    return semstereo_amd


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _cdiv(a, b):
    return -(-a // b)


def _t(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


def _range_input(name, shape, seed, Cout):
    """-> (x fp32 of `shape` [B, Cin, ...] (B = 3 for the batch case), the weights' multipliers per output channel [Cout] float64):
    seeded normal values -- ReLU'd for one_huge_channel, so some are exactly zero -- times the case's channel and batch multipliers"""
    in_mul, w_mul, batch = fm.case_multipliers(name, shape[1], Cout)
    shape = ((3 if batch else shape[0]),) + tuple(shape[1:])
    x = torch.randn(shape, generator=_gen(seed)).double()
    if name == "one_huge_channel":
        x = F.relu(x)
    view = (1, -1) + (1,) * (len(shape) - 2)
    x = x * _t(in_mul).reshape(view)
    if batch:
        x = x * _t(batch).reshape((-1,) + (1,) * (len(shape) - 1))
    return x.float(), _t(w_mul)


def _affine_params(Cout, seed):
    g = _gen(seed)
    return torch.rand(Cout, generator=g) * 0.8 + 0.6, torch.zeros(Cout)      # (no shift: it would hide a small output behind itself)


def _check_bound(what, got, want, S, K, block):
    """element-wise: |got - want| <= f16_bound; block [B, Cout] or a full map"""
    got, want = got.double().cpu(), want.double()
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), what
    blk = _t(block) if not torch.is_tensor(block) else block
    if blk.dim() == 2:
        blk = blk[:, :, None, None]
    bound = (2.0 ** -21 + 4.0 * K ** 0.5 * 2.0 ** -24) * S + 2.0 ** -22 * want.abs() + blk
    err = (got - want).abs()
    excess = float((err - bound).max())
    _record(what, float(err.max()), float((err / bound).max()), "the bound")
    assert excess <= 0.0, (what, excess, float((err / bound).max()))


# --------------------------------------------------------------------------------------------------------------------
# conv2d_k1_f16s: chunks of 32 channels, 64-position tiles
# --------------------------------------------------------------------------------------------------------------------

K1_SHAPES = [(96, 33, 9, 70), (8, 200, 9, 70), (96, 33, 129, 127), (8, 200, 129, 127), (8, 260, 129, 127)]


def _k1_channel_tiles_per_wave(Cout, H, W):
    """proj2d_impl: maps of at least 256 position tiles keep up to 384 channels in one workgroup"""
    nmt = _cdiv(Cout, 32)
    return (3 if nmt > 8 else (2 if nmt > 4 else 1)) if _cdiv(H * W, 64) >= 256 else 1


def test_k1_shapes_reach_every_form():
    assert {_k1_channel_tiles_per_wave(co, h, w) for _ci, co, h, w in K1_SHAPES} == {1, 2, 3}
    assert _k1_channel_tiles_per_wave(200, 129, 127) == 2 and _k1_channel_tiles_per_wave(200, 9, 70) == 1


def _k1_case(name, shape):
    Cin, Cout, H, W = shape
    x, w_mul = _range_input(name, (1, Cin, H, W), 1000 + Cin + W, Cout)
    w = ((torch.rand(Cout, Cin, 1, 1, generator=_gen(Cin * 7 + Cout)) * 2 - 1) * (3.0 / Cin) ** 0.5).double() * w_mul.reshape(-1, 1, 1, 1)
    scale, shift = _affine_params(Cout, Cout)
    return x, w.float(), scale, shift


def _hip_k1(sa, x, w, scale, shift, xb=None):
    E = sa.engine
    return E.conv2d_k1_f16s_hip(x, E.pack_conv2d_k1_weight(w.cuda()), w.shape[0], scale.cuda(), shift.cuda(), False, xb=xb)


@pytest.mark.parametrize("shape", K1_SHAPES, ids=["x".join(map(str, s)) for s in K1_SHAPES])
@pytest.mark.parametrize("name", ALL)
def test_projection_ranges(sa, name, shape):
    x, w, scale, shift = _k1_case(name, shape)
    got = _hip_k1(sa, x.cuda(), w, scale, shift)
    sc = scale.double()[None, :, None, None]
    want = F.conv2d(x.double(), w.double()) * sc
    S = F.conv2d(x.double().abs(), w.double().abs()) * sc
    block = fm.block_term(x.numpy(), w.double().abs().reshape(w.shape[0], -1).numpy(), scale.numpy(), 32)
    _check_bound(f"conv2d_k1 {shape} {name}", got, want, S, shape[0], block)


@pytest.mark.parametrize("shape", K1_SHAPES, ids=["x".join(map(str, s)) for s in K1_SHAPES])
def test_projection_pair_of_views_twelve_decades_apart(sa, shape):
    x, w, scale, shift = _k1_case("tensor_1e+6", shape)
    xa, xb = x.cuda(), (x.flip(3) * 1e-12).cuda()
    one_a, one_b = _hip_k1(sa, xa, w, scale, shift), _hip_k1(sa, xb, w, scale, shift)
    pair = _hip_k1(sa, xa, w, scale, shift, xb=xb)
    assert torch.equal(pair[:1], one_a) and torch.equal(pair[1:], one_b), shape
    pair = _hip_k1(sa, xb, w, scale, shift, xb=xa)
    assert torch.equal(pair[:1], one_b) and torch.equal(pair[1:], one_a), shape


# --------------------------------------------------------------------------------------------------------------------
# deconv2d_bf16s: chunks of 8 channels
# --------------------------------------------------------------------------------------------------------------------

DECONV2D_SHAPES = [(20, 12, 5, 7), (64, 33, 11, 37), (16, 256, 121, 33)]


def _deconv2d_rows_per_wave(Cout, H, W):
    """deconv2d_impl: NT = 2 (8 input rows per workgroup) when one sample offers at least 256 such workgroups"""
    return 2 if _cdiv(W, 32) * _cdiv(H, 8) * _cdiv(Cout, 32) >= 256 else 1


def test_deconv2d_shapes_reach_both_tiles():
    assert [_deconv2d_rows_per_wave(co, h, w) for _ci, co, h, w in DECONV2D_SHAPES] == [1, 1, 2]


def _deconv2d_case(name, shape):
    Cin, Cout, H, W = shape
    x, w_mul = _range_input(name, (1, Cin, H, W), 2000 + Cin + W, Cout)
    w = ((torch.rand(Cin, Cout, 4, 4, generator=_gen(Cin * 5 + Cout)) * 2 - 1) * (3.0 / (4 * Cin)) ** 0.5).double() * w_mul.reshape(1, -1, 1, 1)
    scale, shift = _affine_params(Cout, Cout + 1)
    return x, w.float(), scale, shift


def _hip_deconv2d(sa, x, w, scale, shift, xb=None):
    E = sa.engine
    return E.deconv2d_bf16s_hip(x, E.pack_deconv2d_weight(w.cuda()), w.shape[1], scale.cuda(), shift.cuda(), False, xb=xb)


def _deconv2d_block(x, w, scale):
    """BLOCK per output parity class: output row 2 i + py reads the taps ky with ky % 2 == (py + 1) % 2 (stride 2, padding 1)"""
    B, (Cin, Cout) = x.shape[0], w.shape[:2]
    H, W = x.shape[2:]
    blk = torch.zeros(B, Cout, 2 * H, 2 * W, dtype=torch.float64)
    wa = w.double().abs()
    for py in (0, 1):
        for px in (0, 1):
            taps = wa[:, :, (py + 1) % 2::2, (px + 1) % 2::2].sum(dim=(2, 3)).t()        # [Cout, Cin]
            blk[:, :, py::2, px::2] = _t(fm.block_term(x.numpy(), taps.numpy(), scale.numpy(), 8))[:, :, None, None]
    return blk


@pytest.mark.parametrize("shape", DECONV2D_SHAPES, ids=["x".join(map(str, s)) for s in DECONV2D_SHAPES])
@pytest.mark.parametrize("name", ALL)
def test_deconv2d_ranges(sa, name, shape):
    x, w, scale, shift = _deconv2d_case(name, shape)
    got = _hip_deconv2d(sa, x.cuda(), w, scale, shift)
    sc = scale.double()[None, :, None, None]
    want = F.conv_transpose2d(x.double(), w.double(), None, 2, 1) * sc
    S = F.conv_transpose2d(x.double().abs(), w.double().abs(), None, 2, 1) * sc
    _check_bound(f"deconv2d {shape} {name}", got, want, S, 4 * shape[0], _deconv2d_block(x, w, scale))


@pytest.mark.parametrize("shape", DECONV2D_SHAPES, ids=["x".join(map(str, s)) for s in DECONV2D_SHAPES])
def test_deconv2d_pair_of_views_twelve_decades_apart(sa, shape):
    x, w, scale, shift = _deconv2d_case("tensor_1e+6", shape)
    xa, xb = x.cuda(), (x.flip(3) * 1e-12).cuda()
    one_a, one_b = _hip_deconv2d(sa, xa, w, scale, shift), _hip_deconv2d(sa, xb, w, scale, shift)
    pair = _hip_deconv2d(sa, xa, w, scale, shift, xb=xb)
    assert torch.equal(pair[:1], one_a) and torch.equal(pair[1:], one_b), shape
    pair = _hip_deconv2d(sa, xb, w, scale, shift, xb=xa)
    assert torch.equal(pair[:1], one_b) and torch.equal(pair[1:], one_a), shape


# --------------------------------------------------------------------------------------------------------------------
# conv2d_bf16s (3 x 3, nterms 19) and its concat-free form: chunks of 8 channels
# --------------------------------------------------------------------------------------------------------------------

# (B, Csplit, Crem, Cout, H, W) of CAT_IDENTITY (tests/test_decoder_gpu.py) that reach the 1 x 4, the 2 x 8 and the 4 x 16 tile
CAT_SHAPES = [(2, 8, 20, 12, 9, 33), (1, 64, 64, 128, 128, 256), (1, 64, 64, 128, 256, 256)]
CAT_CASES = CHANNEL + ["x_1e+6_rem_1e-6", "x_1e-6_rem_1e+6"]


def _conv2d_tile(B, Cout, H, W):
    """conv2d_bf16s_impl, plain and concat-free form alike: the first candidate that gives at least 512 workgroups"""
    blocks = lambda th: _cdiv(W, 32) * _cdiv(H, th) * _cdiv(Cout, 32) * B      # noqa: E731
    return 0 if blocks(16) >= 512 else (1 if blocks(8) >= 512 else 2)


def test_cat_shapes_reach_every_tile():
    assert [_conv2d_tile(c[0], c[3], c[4], c[5]) for c in CAT_SHAPES] == [2, 1, 0]


@pytest.mark.parametrize("shape", CAT_SHAPES, ids=["x".join(map(str, s)) for s in CAT_SHAPES])
@pytest.mark.parametrize("name", CAT_CASES)
def test_conv2d_and_concat_free_form_ranges(sa, name, shape):
    B, Cs, Cr, Cout, H, W = shape
    Cin = Cs + Cr
    if name in fm.ALL_RANGE_CASES:
        x, w_mul = _range_input(name, (B, Cin, H, W), 3000 + Cs + W, Cout)
    else:
        x, w_mul = torch.randn(B, Cin, H, W, generator=_gen(3000 + Cs + W)), torch.ones(Cout, dtype=torch.float64)
        first, second = (1e6, 1e-6) if name == "x_1e+6_rem_1e-6" else (1e-6, 1e6)
        x = torch.cat((x[:, :Cs] * first, x[:, Cs:] * second), 1)
    w = ((torch.rand(Cout, Cin, 3, 3, generator=_gen(300 + Cs)) * 2 - 1) * (3.0 / (9 * Cin)) ** 0.5).double() * w_mul.reshape(-1, 1, 1, 1)
    w = w.float()
    scale, shift = _affine_params(Cout, Cout + 2)
    E, p = sa.engine, sa._lib.ptr
    ws = E.pack_conv2d_weight_bf16s(w.cuda(), 19)
    sc, sh = scale.cuda(), shift.cuda()
    xd = x.cuda()
    plain = E.conv2d_bf16s_hip(xd, ws, Cout, sc, sh, False, 19)
    xa, ra = xd[:, :Cs].contiguous(), xd[:, Cs:].contiguous()
    cat = torch.empty_like(plain)
    with torch.cuda.device(xd.device):
        sa._lib.call("ss_conv2d_bf16s_cat_fwd", p(xa), p(ra), None, None, p(ws), p(sc), p(sh), p(cat), B, Cs, Cin, H, W, Cout, 0, 19)
    assert torch.equal(cat, plain), (shape, name)
    s64 = scale.double()[None, :, None, None]
    want = F.conv2d(x.double(), w.double(), None, 1, 1) * s64
    S = F.conv2d(x.double().abs(), w.double().abs(), None, 1, 1) * s64
    block = fm.block_term(x.numpy(), w.double().abs().sum(dim=(2, 3)).numpy(), scale.numpy(), 8)
    _check_bound(f"conv2d 3x3 / cat {shape} tile {_conv2d_tile(B, Cout, H, W)} {name}", plain, want, S, 9 * Cin, block)


# --------------------------------------------------------------------------------------------------------------------
# seghead_f16s through engine.run_seghead: chunks of 8 channels
# --------------------------------------------------------------------------------------------------------------------

HEAD_SHAPES = [(128, 5, 7), (16, 5, 7), (128, 37, 70), (16, 37, 70)]


def _range_head(sa, Cin, seed, w_mul):
    """segmenthead(Cin, 32, 6, 2) with seeded weights, conv1's output channels times w_mul; no shifts (they would hide a small output)"""
    head = sa.modules.segmenthead(Cin, 32, 6, 2)
    g = _gen(seed)
    with torch.no_grad():
        w1 = ((torch.rand(32, Cin, 3, 3, generator=g) * 2 - 1) * (3.0 / (9 * Cin)) ** 0.5).double() * w_mul.reshape(-1, 1, 1, 1)
        head.conv1.conv.weight.copy_(w1.float())
        head.conv1.bn.weight.copy_(torch.rand(32, generator=g) * 0.8 + 0.6)
        head.conv1.bn.running_var.copy_(torch.rand(32, generator=g) * 0.8 + 0.6)
        head.conv1.bn.bias.zero_()
        head.conv1.bn.running_mean.zero_()
        head.conv2.weight.copy_((torch.rand(6, 32, 1, 1, generator=g) * 2 - 1) * (3.0 / 32) ** 0.5)
        head.conv2.bias.zero_()
    return head.eval()


@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=["x".join(map(str, s)) for s in HEAD_SHAPES])
@pytest.mark.parametrize("name", CHANNEL_AND_TENSOR)
def test_seghead_ranges(sa, name, shape):
    """the bound of test_head_bound_against_float64 (tests/test_heads_gpu.py) with BLOCK added to its first-stage term"""
    Cin, H, W = shape
    x, w_mul = _range_input(name, (1, Cin, H, W), 4000 + Cin + W, 32)
    head = _range_head(sa, Cin, 30 + Cin + W, w_mul)
    on_dev = copy.deepcopy(head).cuda().eval()
    with torch.no_grad():
        got = sa.engine.run_seghead(on_dev, on_dev, x.cuda())
    assert got is not None
    got = got.cpu().double()
    h64 = copy.deepcopy(head).double()
    bn = h64.conv1.bn
    scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    with torch.no_grad():
        want = h64._forward_now(x.double())
        w1 = h64.conv1.conv.weight
        y1 = F.relu(bn(h64.conv1.conv(x.double())))
        S1 = F.conv2d(x.double().abs(), w1.abs(), None, 1, 1) * scale.abs()[None, :, None, None]
        blk = _t(fm.block_term(x.numpy(), w1.abs().sum(dim=(2, 3)).numpy(), scale.detach().numpy(), 8))[:, :, None, None]
        b1 = (2.0 ** -21 + 4.0 * (9 * Cin) ** 0.5 * 2.0 ** -24) * S1 + 1e-30 + 2.0 ** -22 * y1.abs() + blk
        w2 = h64.conv2.weight.abs()
        b2 = F.conv2d(b1, w2) + 32 * 2.0 ** -24 * F.conv2d(y1.abs(), w2)
        bound = F.interpolate(b2, size=(2 * H, 2 * W), mode="bilinear", align_corners=False) + 2.0 ** -22 * want.abs()
    assert got.shape == want.shape == (1, 6, 2 * H, 2 * W) and bool(torch.isfinite(got).all())
    err = (got - want).abs()
    _record(f"seghead {shape} {name}", float(err.max()), float((err / bound).max()), "the bound")
    assert float((err - bound).max()) <= 0.0, (shape, name, float((err / bound).max()))


# --------------------------------------------------------------------------------------------------------------------
# the 3-D kernels: error relative to the rms of each (batch element, output channel), against the exact-fp32 kernel's
# --------------------------------------------------------------------------------------------------------------------

def _rel_err(y, ref, region=None):
    """largest |y - ref| relative to the rms of its (batch element, channel) of the float64 result (over `region` of the depth axis)"""
    y = y.double().cpu()
    if region is not None:
        y, ref = y[:, :, region], ref[:, :, region]
    rms = ref.pow(2).mean(dim=(2, 3, 4), keepdim=True).sqrt().clamp_min(1e-300)
    return float(((y - ref) / rms).abs().max())


def _judge32(what, y, y32, ref, region=None):
    assert y.shape == ref.shape and bool(torch.isfinite(y).all()), what
    e, e32 = _rel_err(y, ref, region), _rel_err(y32, ref, region)
    _record(what, e, e / (1.5 * e32 + 1e-6), "1.5 e32 + 1e-6")
    assert e <= 1.5 * e32 + 1e-6, (what, e, e32)


def _conv3d_case(name, Cin, Cout, dhw, seed):
    x, w_mul = _range_input(name, (1, Cin) + tuple(dhw), seed, Cout)
    w = ((torch.rand(Cout, Cin, 3, 3, 3, generator=_gen(seed + 1)) * 2 - 1) * (3.0 / (Cin * 27)) ** 0.5).double() * w_mul.reshape(-1, 1, 1, 1, 1)
    return x, w.float()


def _hip_conv3d(sa, x, w, nterms=19, stride=1, partial=None):
    M = sa.modules
    Cout = w.shape[0]
    one, zero = torch.ones(Cout).cuda(), torch.zeros(Cout).cuda()
    return M.conv3d_bf16s_hip(x, M.pack_conv_weight_bf16s(w.cuda(), nterms), Cout, one, zero, False, nterms, partial=partial, stride=stride)


def _f32_conv3d(sa, x, w, stride=1):
    M = sa.modules
    Cout = w.shape[0]
    return M.conv3d_hip(x, M.pack_conv_weight(w.cuda()), torch.ones(Cout).cuda(), torch.zeros(Cout).cuda(), 3, stride, False)


# ---- stride 1: every tile, forced.  (Cin, Cout, (D, H, W)): the three stride-1 shapes of tests/test_fill_hint_gpu.py ----
S1_SHAPES = {"c64_4x16x64": (64, 64, (4, 16, 64)), "c64_6x16x40": (64, 64, (6, 16, 40)), "c128_2x8x32": (128, 128, (2, 8, 32))}
LARGE_S1 = (16, 32, (4, 128, 512))      # the cheapest layer that is not "small": 16 x 16 x 2 tiles of 2 x 8 x 32, one channel tile


def _s1_blocks(Cout, dhw, td, th, B=1):
    d, h, w = dhw
    return _cdiv(w, 32) * _cdiv(h, th) * _cdiv(d, td) * _cdiv(Cout, 32) * B


def _s1_form(Cout, dhw, tile, B=1):
    """conv3d_bf16s_impl for a forced tile: (rows per wave, planes x rows of the tile, chunk-blocked accumulation).  Chunk-blocked
    is the LAYER's property (what one batch element offers the chip); its 4-row instantiations are the two-pass ones."""
    accb = _s1_blocks(Cout, dhw, 2, 8, B) // B < 512
    if tile == 0:
        return (4, (4, 4) if dhw[0] % 4 == 0 else (2, 8), accb)
    return (2, (1, 8), accb) if tile == 1 else (1, (1, 4), accb)


def test_stride1_shapes_reach_every_form():
    forms = {(k, t): _s1_form(c[1], c[2], t) for k, c in S1_SHAPES.items() for t in (0, 1, 2)}
    assert forms["c64_4x16x64", 0] == (4, (4, 4), True)          # the 4 x 4 x 32 two-pass form
    assert forms["c64_6x16x40", 0] == (4, (2, 8), True)          # the 2 x 8 x 32 two-pass form
    assert forms["c128_2x8x32", 1] == (2, (1, 8), True)          # the 2-row form
    assert forms["c128_2x8x32", 2] == (1, (1, 4), True)
    assert _s1_form(LARGE_S1[1], LARGE_S1[2], 0) == (4, (4, 4), False)      # the single chain of large layers
    assert _s1_blocks(LARGE_S1[1], LARGE_S1[2], 2, 8) >= 512
    # ... and nothing cheaper meets that condition: the tile count is its lower bound, Cin = 16 is two chunks
    assert _s1_blocks(LARGE_S1[1], LARGE_S1[2], 2, 8) == 512


@pytest.mark.parametrize("shape", sorted(S1_SHAPES))
@pytest.mark.parametrize("name", ALL)
def test_conv3d_stride1_ranges_on_every_tile(sa, name, shape, tuning_env):
    Cin, Cout, dhw = S1_SHAPES[shape]
    x, w = _conv3d_case(name, Cin, Cout, dhw, 5000 + Cin + dhw[0])
    ref = F.conv3d(x.double(), w.double(), None, 1, 1)
    xd = x.cuda()
    y32 = _f32_conv3d(sa, xd, w)
    # a partial sum 100 x this convolution's contribution, as in test_conv3d_f16_form_block_floating_ranges
    rms = ref.pow(2).mean(dim=(2, 3, 4), keepdim=True).sqrt().clamp_min(1e-300)
    part = (torch.randn(ref.shape, generator=_gen(703)).double() * rms * 100.0).float()
    refp = ref + part.double()
    for tile in (0, 1, 2):
        tuning_env("SS_CONV_TILE", str(tile))
        _judge32(f"conv3d s1 {shape} tile {tile} {name}", _hip_conv3d(sa, xd, w), y32, ref)
        yp = _hip_conv3d(sa, xd, w, partial=part.cuda())
        y6 = _hip_conv3d(sa, xd, w, nterms=6, partial=part.cuda())
        assert bool(torch.isfinite(yp).all())
        ep = float(((yp.double().cpu() - refp) / (100.0 * rms)).abs().max())
        ep6 = float(((y6.double().cpu() - refp) / (100.0 * rms)).abs().max())
        _record(f"conv3d s1 {shape} tile {tile} {name} + partial x100", ep, ep / min(2.0 * ep6 + 1e-6, 2e-5), "min(2 e_bf16x6 + 1e-6, 2e-5)")
        assert ep <= 2.0 * ep6 + 1e-6 and ep <= 2e-5, (shape, tile, name, ep, ep6)


@pytest.mark.parametrize("name", RAMPS)
def test_conv3d_single_chain_four_row_tile_ranges(sa, name, tuning_env):
    Cin, Cout, dhw = LARGE_S1
    x, w = _conv3d_case(name, Cin, Cout, dhw, 5100)
    ref = F.conv3d(x.double(), w.double(), None, 1, 1)
    tuning_env("SS_CONV_TILE", "0")
    _judge32(f"conv3d s1 single chain {LARGE_S1} {name}", _hip_conv3d(sa, x.cuda(), w), _f32_conv3d(sa, x.cuda(), w), ref)


# ---- stride 2: the three forms on the 32 -> 64 shape of tests/test_fill_hint_gpu.py ----
S2_SHAPE = (32, 64, (4, 16, 64))


def _s2_form(Cout, dhw, hint, mt1, B=1):
    """ss::plan_conv3d (csrc/conv_plan.h), stride 2: the waves split 64 channels (count alone) / two channel tiles per wave (SS_CONV_S2_MT1=0) / one tile per wave"""
    do, ho, wo = [(n - 1) // 2 + 1 for n in dhw]
    wg2 = _cdiv(wo, 32) * _cdiv(ho, 2) * _cdiv(do, 2) * _cdiv(Cout, 64) * B * hint
    if Cout > 32 and wg2 >= 256 and mt1 < 0:
        return "split"
    return "two_tiles" if Cout > 32 and wg2 >= 256 and mt1 <= 0 else "one_tile"


def test_stride2_forms_are_the_three():
    assert _s2_form(64, S2_SHAPE[2], 64, 1) == "one_tile" and _s2_form(64, S2_SHAPE[2], 64, 0) == "two_tiles"
    assert _s2_form(64, S2_SHAPE[2], 64, -1) == "split" and _s2_form(64, S2_SHAPE[2], 1, -1) == "one_tile"


@pytest.mark.parametrize("name", CHANNEL_AND_TENSOR)
def test_conv3d_stride2_ranges_in_every_form(sa, name, tuning_env):
    Cin, Cout, dhw = S2_SHAPE
    x, w = _conv3d_case(name, Cin, Cout, dhw, 5200)
    ref = F.conv3d(x.double(), w.double(), None, 2, 1)
    xd = x.cuda()
    y32 = _f32_conv3d(sa, xd, w, stride=2)
    lib = sa._lib.load()
    prev = lib.ss_set_fill_hint(64)
    try:
        for form, mt1 in (("one_tile", "1"), ("two_tiles", "0"), ("split", "-1")):
            tuning_env("SS_CONV_S2_MT1", mt1)
            assert _s2_form(Cout, dhw, lib.ss_get_fill_hint(), int(mt1)) == form
            _judge32(f"conv3d s2 {form} {name}", _hip_conv3d(sa, xd, w, stride=2), y32, ref)
    finally:
        lib.ss_set_fill_hint(prev)


# ---- tiles walked by one workgroup: a stale exponent from the tile before ----
WALK = (16, 32, (12, 44, 64), 32)       # Cin, Cout, (D, H, W), B: one batch element repeated B times


def _walk_tiles(dhw, tile):
    td, th = _s1_form(32, dhw, tile)[1]
    return _cdiv(dhw[2], 32) * _cdiv(dhw[1], th) * _cdiv(dhw[0], td), td


def _judged_planes(D, td, slab):
    """output planes whose tile [d0, d0 + td) and its halo plane on either side lie inside one slab of the input (planes < slab / >= slab)"""
    planes = []
    for d0 in range(0, D, td):
        lo, hi = max(d0 - 1, 0), min(d0 + td, D - 1)
        if hi < slab or lo >= slab:
            planes += list(range(d0, min(d0 + td, D)))
    return planes


@pytest.mark.parametrize("order", ["1e+6_then_1e-6", "1e-6_then_1e+6"])
@pytest.mark.parametrize("tile", [0, 2])
def test_conv3d_persistent_walk_across_slabs_of_other_magnitude(sa, tile, order, tuning_env):
    """launch_conv: cap = resident workgroups / (ceil(Cout / 32) B), at most 4 workgroups on each of 256 CUs; with at least twice as
    many tiles every workgroup walks two or more (tile, tile + gridDim.x, ...), here from one depth slab into the other."""
    Cin, Cout, dhw, B = WALK
    D = dhw[0]
    groups = _cdiv(Cout, 32) * B
    ntiles, td = _walk_tiles(dhw, tile)
    assert ntiles >= 2 * 1024 // groups and ntiles * groups >= 2 * 1024
    assert _s1_blocks(Cout, dhw, 2, 8) < 512                     # chunk-blocked at every batch size
    x = torch.randn((1, Cin) + tuple(dhw), generator=_gen(5300)).double()
    w = ((torch.rand(Cout, Cin, 3, 3, 3, generator=_gen(5301)) * 2 - 1) * (3.0 / (Cin * 27)) ** 0.5).float()
    first, second = (1e6, 1e-6) if order == "1e+6_then_1e-6" else (1e-6, 1e6)
    x = torch.cat((x[:, :, :4] * first, x[:, :, 4:] * second), 2).float()
    ref = F.conv3d(x.double(), w.double(), None, 1, 1)
    planes = _judged_planes(D, td, 4)
    assert planes == ([8, 9, 10, 11] if tile == 0 else [0, 1, 2, 5, 6, 7, 8, 9, 10, 11])
    tuning_env("SS_CONV_TILE", str(tile))
    y = _hip_conv3d(sa, x.cuda().expand(B, -1, -1, -1, -1).contiguous(), w)
    assert bool((y == y[:1]).all()), "batch elements of one input differ"
    y32 = _f32_conv3d(sa, x.cuda(), w)
    for region in ([p for p in planes if p < 4], [p for p in planes if p >= 4]):
        if region:
            _judge32(f"conv3d walk tile {tile} {order} planes {region[0]}-{region[-1]}", y[:1], y32, ref, region)


# ---- deconv3d_bf16s ----
DECONV3D = (48, 40, 3, 9, 35, 16)       # the shape of test_deconv3d_f16_form_block_floating_ranges


def _deconv_form(D, H, W, Cout, B=1, nterms=19, groups=-1, stream=-1):
    """ss::plan_deconv3d (csrc/conv_plan.h) over an INPUT of (D, H, W): -> ((planes, rows) of the 32-column tile, groups, stream).
    groups 0: all 8 output parity classes in one workgroup, 1: two class groups, 2: two groups + chunk-blocked accumulation -- by
    what ONE pair offers the chip, or SS_DECONV_GROUPS; stream: nontemporal stores (groups 0 only), by the launch's output bytes or
    SS_DECONV_STREAM.  The bf16 forms have one form: (tile, 0, False)."""
    td, th = (2, 2) if D >= 2 and H < 4 else (1, 4)
    if nterms != 19:
        return (td, th), 0, False
    per_pair = _cdiv(W, 32) * _cdiv(H, th) * _cdiv(D, td) * _cdiv(Cout, 32)
    g = groups if groups in (0, 1, 2) else (2 if per_pair < 256 else 0)
    s = stream != 0 if stream >= 0 else B * Cout * 8 * D * H * W * 4 >= 192 << 20
    return (td, th), g, g == 0 and s


def _deconv_skip_orders(D, H, W, Cout):
    """the non-split forms project the skip tensor before the main loop where (unit ^ channel tile) is odd, after it elsewhere:
    -> the set of (unit ^ channel tile) & 1 over a launch's workgroups ({0, 1}: both orders run)"""
    (td, th), _, _ = _deconv_form(D, H, W, Cout)
    units = _cdiv(W, 32) * _cdiv(H, th) * _cdiv(D, td)
    return {(u ^ c) & 1 for u in range(units) for c in range(_cdiv(Cout, 32))}


def test_deconv3d_range_shape_runs_both_skip_orders():
    _cin, Cout, D, H, W, _cs = DECONV3D
    assert _deconv_form(D, H, W, Cout) == ((1, 4), 2, False)        # 2 x 3 x 3 tiles of 1 x 4 x 32, 2 channel tiles: 36 < 256
    assert (_cdiv(W, 32), _cdiv(H, 4), D, _cdiv(Cout, 32)) == (2, 3, 3, 2) and _deconv_skip_orders(D, H, W, Cout) == {0, 1}


@pytest.mark.parametrize("split", ["0", "1"])     # (SS_DECONV_SPLIT: the form of the exact-fp32 kernel that is the yardstick)
@pytest.mark.parametrize("skip_mul", [1e-6, 1.0, 1e6])
@pytest.mark.parametrize("name", CHANNEL + ["out_channels_1e-8_to_1e+8"])
def test_deconv3d_ranges_beside_the_skip_projection(sa, name, skip_mul, split, tuning_env):
    """the fp16 main loop with a growing / shrinking maximum, and the bf16 skip projection that initialises its accumulators
    (E_INIT_SHIFT: SS_DECONV_GROUPS=0, the workgroups with (unit ^ channel tile) odd) or joins them after the loop (the other
    workgroups, and all of groups 1 and 2), 12 decades below, at and 12 decades above the main term; the weights of both, per
    output channel, times the case's multipliers"""
    tuning_env("SS_DECONV_SPLIT", split)
    M = sa.modules
    Cin, Cout, D, H, W, Cs = DECONV3D
    x, w_mul = _range_input(name, (1, Cin, D, H, W), 5400, Cout)
    g = _gen(5401)
    w = (torch.rand(Cin, Cout, 3, 3, 3, generator=g) * 2 - 1) * (3.0 / (Cin * 27 / 8)) ** 0.5
    ws = (torch.rand(Cout, Cs, 1, 1, 1, generator=g) * 2 - 1) * (3.0 / Cs) ** 0.5
    w = (w.double() * w_mul.reshape(1, -1, 1, 1, 1)).float()            # a transposed conv's weight is [Cin, Cout, ...]
    ws = (ws.double() * w_mul.reshape(-1, 1, 1, 1, 1)).float()
    main = F.conv_transpose3d(x.double(), w.double(), None, stride=2, padding=1, output_padding=1)
    main_rms = float((main / w_mul.reshape(1, -1, 1, 1, 1)).pow(2).mean().sqrt())      # of the main term before the channels' multipliers
    skip = (torch.randn(1, Cs, 2 * D, 2 * H, 2 * W, generator=g).double() * main_rms * skip_mul).float()
    ref = main + F.conv3d(skip.double(), ws.double())
    wp = M.pack_conv_weight(w.cuda(), transposed=True)
    wsp = M.pack_conv_weight(ws.cuda()).reshape(Cs, Cout).contiguous()
    zero = torch.zeros(Cout).cuda()
    y32 = M.deconv3d_hip(x.cuda(), wp, zero, False, skip.cuda(), wsp)
    for groups in (0, 1, 2):
        tuning_env("SS_DECONV_GROUPS", str(groups))
        assert _deconv_form(D, H, W, Cout, groups=groups)[1] == groups
        y = M.deconv3d_bf16s_hip(x.cuda(), M.pack_deconv_weight_bf16s(wp, 19), Cout, zero, False, 19, skip.cuda(), M.pack_deconv_weight_bf16s(wsp))
        _judge32(f"deconv3d groups {groups} split {split} {name} skip x{skip_mul:g}", y, y32, ref)


# ---- the gathered stem ----
# (B, C, nd, H, W, forced tile or None) of test_stem_gathers_the_warped_half_in_its_staging (tests/test_parity_gpu.py)
STEM = [(1, 32, 24, 96, 128, None), (2, 32, 24, 64, 96, None), (1, 16, 6, 160, 160, 0)]


def _stem_form(B, C, nd, H, W, forced):
    """ss_conv3d_gather_fwd: the rules of a stride-1 layer of this output shape"""
    blocks = lambda td, th: _cdiv(W, 32) * _cdiv(H, th) * _cdiv(nd, td) * _cdiv(C, 32) * B      # noqa: E731
    tile = forced if forced is not None else (0 if blocks(2, 8) >= 512 else (1 if blocks(1, 8) >= 512 else 2))
    assert tile == 0
    return ((4, 4) if nd % 4 == 0 else (2, 8)), blocks(2, 8) // B < 512


def test_stem_shapes_reach_the_four_row_tiles():
    assert [_stem_form(*s) for s in STEM] == [((4, 4), False), ((4, 4), True), ((2, 8), True)]


@pytest.mark.parametrize("shape", STEM, ids=["x".join(map(str, s)) for s in STEM])
@pytest.mark.parametrize("name", RAMPS)
def test_gathered_stem_ranges(sa, name, shape, tuning_env):
    """the assertion of test_stem_gathers_the_warped_half_in_its_staging -- as close to the float64 convolution of the exact gather
    as the three-launch form is to its own -- with errors relative to each channel's rms, on right features whose channels ramp over
    12 decades; alone and continuing a partial sum 1e+6 / 1e-6 times the gathered term"""
    from oracle import detdata as dd
    M = sa.modules
    B, C, nd, H, W, forced = shape
    if forced is not None:
        tuning_env("SS_CONV_TILE", str(forced))
    cr, _ = _range_input(name, (B, C, H, W), 5500 + H, C)
    cr = cr * 3.0
    samples = dd.distinct_sorted_candidates(B, nd, H, W, max(nd, min(W // 2, 48)), 333)
    att = dd.t_uniform((B, 1, nd, H, W), 334, 0.0, 0.7)
    stem = M.BasicConv(2 * C, C, is_3d=True, kernel_size=3, stride=1, padding=1)
    with torch.no_grad():
        stem.conv.weight.copy_(dd.t_uniform((C, 2 * C, 3, 3, 3), 336, -1, 1) * (3.0 / (2 * C * 27)) ** 0.5)
        stem.bn.weight.copy_(dd.t_uniform((C,), 337, 0.6, 1.4)); stem.bn.bias.zero_()
        stem.bn.running_mean.zero_(); stem.bn.running_var.copy_(dd.t_uniform((C,), 340, 0.6, 1.4))
    stem = stem.cuda().eval()
    sc, sh = (t.detach() for t in M.fold_bn(stem.bn))
    w64 = stem.conv.weight.detach().cpu().double()
    idx = torch.arange(W).reshape(1, 1, 1, W) - samples.long()
    ok = (idx >= 0) & (idx < W)
    gathered = torch.gather(cr.unsqueeze(2).expand(B, C, nd, H, W), 4, idx.clamp(0, W - 1).unsqueeze(1).expand(B, C, nd, H, W))
    xg = (att * (gathered * ok.unsqueeze(1))).float()
    with torch.no_grad():
        assert M.stem_gather_applies(stem, cr.cuda(), samples.cuda())
        right = sa.ops.concat_volume_sampled(None, cr.cuda(), samples.cuda(), att.cuda())
    term_g = F.conv3d(xg.double(), w64[:, C:], None, 1, 1)
    term_3 = F.conv3d(right.cpu().double(), w64[:, C:], None, 1, 1)
    rms = term_g.pow(2).mean(dim=(2, 3, 4), keepdim=True).sqrt().clamp_min(1e-300)
    noise = torch.randn(term_g.shape, generator=_gen(341)).double()

    def finish(acc):
        return F.relu(acc * sc.cpu().double().reshape(1, -1, 1, 1, 1) + sh.cpu().double().reshape(1, -1, 1, 1, 1))
    for pmul in (None, 1e6, 1e-6):
        part = None if pmul is None else (noise * rms * pmul).float()
        p64 = 0.0 if part is None else part.double()
        pd = None if part is None else part.cuda()
        with torch.no_grad():
            y_g = M.stem_gather_half(stem, cr.cuda(), samples.cuda(), att.cuda(), pd, None)
            if part is None:
                y_3 = M.conv3d_bf16s_hip(right, sa.engine._stem_halves_params(stem, C)[2], C, sc, sh, True, 19, None, None)
            else:
                y_3 = M.stem_volume_half(stem, right, pd, None)
        ref_g, ref_3 = finish(term_g + p64), finish(term_3 + p64)
        assert y_g.shape == ref_g.shape and bool(torch.isfinite(y_g).all())
        e_g, e_3 = _rel_err(y_g, ref_g), _rel_err(y_3, ref_3)
        _record(f"stem gather {shape} {name} partial x{pmul}", e_g, e_g / max(2.0 * e_3 + 1e-6, 8e-6), "max(2 e_three_launch + 1e-6, 8e-6)")
        assert e_g <= max(2.0 * e_3 + 1e-6, 8e-6), (shape, name, pmul, e_g, e_3)


# ---- the one-pass classifier ----

@pytest.mark.parametrize("name", RAMPS)
def test_classifier_one_pass_ranges(sa, name, monkeypatch):
    """the assertions of test_classifier_one_pass_form_against_the_two_launch_form_and_float64 at its shape (1, 12, 134, 200), relative
    to the rms of the float64 result, on inputs whose channels ramp over 12 decades"""
    from oracle import detdata as dd
    B, D, H, W = 1, 12, 134, 200
    assert _s1_blocks(32, (D, H, W), 2, 8) >= 512 and D % 4 == 0        # classifier_fused_applies: the layer fills the chip, 4-plane tiles

    def classifier():
        m = sa.modules.Classifier(32).cuda().eval()
        with torch.no_grad():
            for i, p in enumerate(m.parameters()):
                p.copy_((dd.t_uniform(tuple(p.shape), 900 + i, -1, 1) * (0.05 if p.dim() > 1 else 1.0)).cuda())
            m[0][1].bias.zero_()
            m[0][1].running_mean.zero_()
            m[0][1].running_var.copy_(dd.t_uniform((32,), 911, 0.6, 1.4).cuda())
        return m
    m = classifier()
    x, _ = _range_input(name, (B, 32, D, H, W), 5600, 32)
    xd = x.cuda()
    assert sa.engine.classifier_fused_applies(xd, 19)
    outs = []
    for flag in (True, False):
        monkeypatch.setattr(sa.engine, "CLASSIFIER_FUSED", flag)
        with torch.no_grad():
            outs.append(m(xd))
    assert outs[0].shape == (B, 1, D, H, W) and bool(torch.isfinite(outs[0]).all())
    assert float((outs[0] - outs[1]).abs().max()) <= 4e-6 * float(outs[1].abs().max())
    md = classifier().double().cpu()
    with torch.no_grad():
        ref = F.conv3d(F.relu(md[0][1](F.conv3d(x.double(), md[0][0].weight, padding=1))), md[2].weight, padding=1)
    ref_rms = float(ref.pow(2).mean().sqrt())
    e = [float((o.double().cpu() - ref).pow(2).mean().sqrt()) / ref_rms for o in outs]
    _record(f"classifier one pass {name}", e[0], e[0] / (1.1 * e[1] + 1e-9), "1.1 e_two_launch + 1e-9")
    assert e[0] <= 1.1 * e[1] + 1e-9 and e[0] <= 2e-6 * float(ref.abs().max()) / ref_rms, (name, e)
