"""The 2-D decoder on HIP (csrc/deconv2d_bf16s.hip, the concat-free form of the 2-D conv): per-layer error against float64 with the
fp32 CPU layer as the yardstick, bit identities, edge shapes, the twins against tests/golden/decoder.npz, a whole forward and the
switches.  Run on the MI355X box: pytest -m gpu.  (Set SS_DECODER_ERR_OUT=<file> to keep the error table.)"""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from golden import decoder_cases as dc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (Cin, Cout, pyramid level of the INPUT: 1/2^level) of the nine transposed layers: FeatUp's four, the spx chain's four, spx2
DECONVS = [("featup.deconv32_16", 512, 384, 5), ("featup.deconv16_8", 768, 256, 4), ("featup.deconv8_4", 512, 128, 3),
           ("featup.deconv4_2", 256, 64, 2), ("spx32_16", 256, 384, 5), ("spx16_8", 768, 256, 4), ("spx8_4", 512, 128, 3),
           ("spx4_2", 256, 64, 2), ("spx2", 128, 6, 1)]
# (channels of each half = Csplit, pyramid level) of the four concat convs: Cin = Cout = 2 Csplit
CATS = [("conv2@1/16", 384, 4), ("conv2@1/8", 256, 3), ("conv2@1/4", 128, 2), ("conv2@1/2", 64, 1)]


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    assert semstereo_amd.engine.CONV_ENGINE == "f16x3"
    return semstereo_amd


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _deconv_params(Cin, Cout, seed, bias_only=False):
    g = _gen(seed)
    w = (torch.rand(Cin, Cout, 4, 4, generator=g) * 2 - 1) * (3.0 / (4 * Cin)) ** 0.5
    if bias_only:
        return w, None, torch.rand(Cout, generator=g) * 0.2 - 0.1
    return w, torch.rand(Cout, generator=g) * 0.8 + 0.6, torch.rand(Cout, generator=g) * 0.2 - 0.1


def _conv_params(Cin, Cout, seed):
    g = _gen(seed)
    w = (torch.rand(Cout, Cin, 3, 3, generator=g) * 2 - 1) * (3.0 / (9 * Cin)) ** 0.5
    return w, torch.rand(Cout, generator=g) * 0.8 + 0.6, torch.rand(Cout, generator=g) * 0.2 - 0.1


def _affine(y, scale, shift, relu):
    if scale is not None:
        y = y * scale.to(y.dtype)[None, :, None, None]
    if shift is not None:
        y = y + shift.to(y.dtype)[None, :, None, None]
    return F.relu(y) if relu else y


def _deconv_ref(x, w, scale, shift, relu, dtype):
    return _affine(F.conv_transpose2d(x.to(dtype), w.to(dtype), None, 2, 1), scale, shift, relu)


def _conv_ref(x, w, scale, shift, relu, dtype):
    return _affine(F.conv2d(x.to(dtype), w.to(dtype), None, 1, 1), scale, shift, relu)


def _hip_deconv(sa, x, w, scale, shift, relu, xb=None):
    E = sa.engine
    ws = E.pack_deconv2d_weight(w.cuda())
    c = lambda t: None if t is None else t.cuda().contiguous()
    return E.deconv2d_bf16s_hip(x, ws, w.shape[1], c(scale), c(shift), relu, xb=xb)


def _hip_conv(sa, x, w, scale, shift, relu):
    E = sa.engine
    ws = E.pack_conv2d_weight_bf16s(w.cuda(), 19)
    return E.conv2d_bf16s_hip(x, ws, w.shape[0], scale.cuda(), shift.cuda(), relu, 19)


def _hip_cat(sa, xa, ra, w, scale, shift, relu, xb=None, rb=None):
    ws = sa.engine.pack_conv2d_weight_bf16s(w.cuda(), 19)
    Cs, Cin = xa.shape[1], xa.shape[1] + ra.shape[1]
    B, _, H, W = xa.shape
    out = torch.empty(((2 if xb is not None else 1) * B, w.shape[0], H, W), device="cuda")
    p = sa._lib.ptr
    sc, sh = scale.cuda(), shift.cuda()                        # (held until the launch is issued)
    with torch.cuda.device(xa.device):
        sa._lib.call("ss_conv2d_bf16s_cat_fwd", p(xa), p(ra), p(xb), p(rb), p(ws), p(sc), p(sh), p(out), B, Cs, Cin,
                     H, W, w.shape[0], int(relu), 19)
    return out


_TABLE = []


def _judge(name, hip, cpu32, truth):
    """HIP rms error <= 2x the fp32 CPU layer's, max-abs <= 4x its max-abs, both against float64."""
    eh, ec = (hip.double() - truth).abs(), (cpu32.double() - truth).abs()
    rh, rc = float(eh.pow(2).mean().sqrt()), float(ec.pow(2).mean().sqrt())
    mh, mc = float(eh.max()), float(ec.max())
    line = f"{name:44s} rms hip {rh:.3e} cpu {rc:.3e} ratio {rh / rc:5.2f} | max hip {mh:.3e} cpu {mc:.3e} ratio {mh / mc:5.2f}"
    print(line)
    _TABLE.append(line)
    path = os.environ.get("SS_DECODER_ERR_OUT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(_TABLE) + "\n")
    return rh <= 2.0 * rc and mh <= 4.0 * mc, line


def _corners(H, W, h, w):
    """Four corner windows (y0, y1, x0, x1) of an H x W map, h x w each (the whole map when it is smaller)."""
    h, w = min(h, H), min(w, W)
    return [(0, h, 0, w), (0, h, W - w, W), (H - h, H, 0, w), (H - h, H, W - w, W)]


@pytest.mark.parametrize("size", [256, 1024])
@pytest.mark.parametrize("layer", DECONVS, ids=[d[0] for d in DECONVS])
def test_deconv_error_against_float64(sa, layer, size):
    """256^2 pyramid: the whole layer.  1024^2: the kernel runs the whole layer, the float64 answer is computed on four corner crops
    (all four borders; the crop's rows / columns next to its artificial cut are left out of the comparison)."""
    name, Cin, Cout, lvl = layer
    H = W = size >> lvl
    spx2 = name == "spx2"
    w, scale, shift = _deconv_params(Cin, Cout, 100 + lvl + Cin, bias_only=spx2)
    x = torch.randn(1, Cin, H, W, generator=_gen(7 + lvl + Cout))
    hip = _hip_deconv(sa, x.cuda(), w, scale, shift, not spx2).cpu()
    assert tuple(hip.shape) == (1, Cout, 2 * H, 2 * W)
    parts = {"hip": [], "cpu": [], "truth": []}
    wins = [(0, H, 0, W)] if size == 256 else _corners(H, W, 40, 48)
    for (y0, y1, x0, x1) in wins:
        xc = x[:, :, y0:y1, x0:x1].contiguous()
        # output rows computed from a cut edge are wrong in the crop: drop 2 output rows / columns there
        oy0, oy1 = (0 if y0 == 0 else 2), (2 * (y1 - y0) - (0 if y1 == H else 2))
        ox0, ox1 = (0 if x0 == 0 else 2), (2 * (x1 - x0) - (0 if x1 == W else 2))
        parts["cpu"].append(_deconv_ref(xc, w, scale, shift, not spx2, torch.float32)[:, :, oy0:oy1, ox0:ox1].reshape(-1))
        parts["truth"].append(_deconv_ref(xc, w, scale, shift, not spx2, torch.float64)[:, :, oy0:oy1, ox0:ox1].reshape(-1))
        parts["hip"].append(hip[:, :, 2 * y0 + oy0:2 * y0 + oy1, 2 * x0 + ox0:2 * x0 + ox1].reshape(-1))
    ok, line = _judge(f"deconv {name} {Cin}->{Cout} @{H}x{W}", torch.cat(parts["hip"]), torch.cat(parts["cpu"]), torch.cat(parts["truth"]))
    assert ok, line


@pytest.mark.parametrize("size", [256, 1024])
@pytest.mark.parametrize("layer", CATS, ids=[c[0] for c in CATS])
def test_concat_free_conv_error_against_float64(sa, layer, size):
    name, Cs, lvl = layer
    H = W = size >> lvl
    Cin = Cout = 2 * Cs
    w, scale, shift = _conv_params(Cin, Cout, 200 + lvl)
    g = _gen(17 + lvl)
    xa, ra = F.relu(torch.randn(1, Cs, H, W, generator=g)), torch.randn(1, Cs, H, W, generator=g)
    hip = _hip_cat(sa, xa.cuda(), ra.cuda(), w, scale, shift, True).cpu()
    x = torch.cat((xa, ra), 1)
    parts = {"hip": [], "cpu": [], "truth": []}
    wins = [(0, H, 0, W)] if size == 256 else _corners(H, W, 40, 48)
    for (y0, y1, x0, x1) in wins:
        xc = x[:, :, y0:y1, x0:x1].contiguous()
        oy0, oy1 = (0 if y0 == 0 else 1), (y1 - y0) - (0 if y1 == H else 1)
        ox0, ox1 = (0 if x0 == 0 else 1), (x1 - x0) - (0 if x1 == W else 1)
        parts["cpu"].append(_conv_ref(xc, w, scale, shift, True, torch.float32)[:, :, oy0:oy1, ox0:ox1].reshape(-1))
        parts["truth"].append(_conv_ref(xc, w, scale, shift, True, torch.float64)[:, :, oy0:oy1, ox0:ox1].reshape(-1))
        parts["hip"].append(hip[:, :, y0 + oy0:y0 + oy1, x0 + ox0:x0 + ox1].reshape(-1))
    ok, line = _judge(f"cat-conv {name} {Cin}->{Cout} @{H}x{W}", torch.cat(parts["hip"]), torch.cat(parts["cpu"]), torch.cat(parts["truth"]))
    assert ok, line


def _conv2d_tile(B, Cout, H, W):
    """The tile the 2-D conv (plain and concat-free form alike) picks for a launch of B elements: 0 = 4 x 16 rows, 1 = 2 x 8, 2 = 1 x 4
    (conv2d_bf16s_impl: the first candidate that gives at least 512 workgroups)."""
    blocks = lambda th: -(-W // 32) * -(-H // th) * -(-Cout // 32) * B
    return 0 if blocks(16) >= 512 else (1 if blocks(8) >= 512 else 2)


# (B, Csplit, Crem, Cout, H, W): the last three reach the 2 x 8 tile, the 4 x 16 tile, and change tile between one and two views
CAT_IDENTITY = [(1, 64, 64, 128, 40, 72), (2, 8, 20, 12, 9, 33), (1, 384, 384, 768, 16, 16), (3, 16, 8, 40, 5, 100),
                (1, 64, 64, 128, 128, 256), (1, 64, 64, 128, 256, 256), (1, 384, 384, 768, 64, 64)]


@pytest.mark.parametrize("shape", CAT_IDENTITY, ids=["x".join(map(str, c)) for c in CAT_IDENTITY])
def test_concat_free_conv_equals_the_conv_on_the_materialised_cat(sa, shape):
    """Bit for bit the plain form on torch.cat((x, rem), 1), on every tile; two views in one launch: the plain form at batch 2B bit
    for bit, and the two single-view launches bit for bit where the doubled launch keeps the tile -- to 2e-6 on these O(1) outputs
    where it moves to a larger one (the block-floating scale is per tile; the bound of test_conv2d_on_both_views_in_one_launch)."""
    B, Cs, Cr, Cout, H, W = shape
    w, scale, shift = _conv_params(Cs + Cr, Cout, 300 + Cs)
    g = _gen(Cs + H)
    xa, ra = torch.randn(B, Cs, H, W, generator=g).cuda(), torch.randn(B, Cr, H, W, generator=g).cuda()
    for relu in (True, False):
        want = _hip_conv(sa, torch.cat((xa, ra), 1), w, scale, shift, relu)
        assert torch.equal(_hip_cat(sa, xa, ra, w, scale, shift, relu), want), (shape, relu)
    xb, rb = torch.randn(B, Cs, H, W, generator=g).cuda(), torch.randn(B, Cr, H, W, generator=g).cuda()
    both = _hip_cat(sa, xa, ra, w, scale, shift, True, xb, rb)
    conv2 = _hip_conv(sa, torch.cat((torch.cat((xa, ra), 1), torch.cat((xb, rb), 1)), 0), w, scale, shift, True)
    assert torch.equal(both, conv2)                          # (same launch geometry: the plain form at batch 2B)
    one_a, one_b = _hip_cat(sa, xa, ra, w, scale, shift, True), _hip_cat(sa, xb, rb, w, scale, shift, True)
    same_tile = _conv2d_tile(B, Cout, H, W) == _conv2d_tile(2 * B, Cout, H, W)
    da, db = float((both[:B] - one_a).abs().max()), float((both[B:] - one_b).abs().max())
    print(f"cat pair vs singles {shape}: tiles {_conv2d_tile(B, Cout, H, W)} -> {_conv2d_tile(2 * B, Cout, H, W)}, max diff {da:.2e} {db:.2e}, max |y| {float(both.abs().max()):.2f}")
    if same_tile:
        assert torch.equal(both[:B], one_a) and torch.equal(both[B:], one_b), shape
    else:
        assert da <= 2e-6 and db <= 2e-6, (shape, da, db)


def test_concat_free_conv_tile_cases_cover_every_tile():
    tiles = {_conv2d_tile(c[0], c[3], c[4], c[5]) for c in CAT_IDENTITY}
    moved = [c for c in CAT_IDENTITY if _conv2d_tile(c[0], c[3], c[4], c[5]) != _conv2d_tile(2 * c[0], c[3], c[4], c[5])]
    assert tiles == {0, 1, 2} and moved


def test_concat_free_conv_refuses_a_split_inside_a_chunk(sa):
    # Csplit % 8 != 0 is refused, and the engine wrapper then declines
    with pytest.raises(sa._lib.SemStereoHipError):
        w, scale, shift = _conv_params(24, 8, 1)
        _hip_cat(sa, torch.zeros(1, 12, 4, 4).cuda(), torch.zeros(1, 12, 4, 4).cuda(), w, scale, shift, True)
    cv = nn.Conv2d(24, 8, 3, 1, 1, bias=False).cuda().eval()
    assert sa.engine.run_conv2d_cat(cv, "k", cv, None, torch.zeros(1, 12, 4, 4).cuda(), torch.zeros(1, 12, 4, 4).cuda(), True) is None


def test_ragged_conv2x_pair_runs_the_deconv_once(sa, monkeypatch):
    """forward_pair where the concat-free launch declines (Csplit = 12): the pair deconv's result feeds the plain 3x3, no second deconv."""
    M, E = sa.modules, sa.engine
    mod = dc.fill(M.Conv2x(20, 12, deconv=True).eval(), 8).cuda()
    g = _gen(4)
    xa, xb = torch.randn(1, 20, 5, 7, generator=g).cuda(), torch.randn(1, 20, 5, 7, generator=g).cuda()
    ra, rb = torch.randn(1, 12, 10, 14, generator=g).cuda(), torch.randn(1, 12, 10, 14, generator=g).cuda()
    calls = []
    real = E.run_deconv2d
    monkeypatch.setattr(E, "run_deconv2d", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        before = dict(M.PATH_COUNTS)
        za, zb = mod.forward_pair(xa, ra, xb, rb)
        assert len(calls) == 1 and M.PATH_COUNTS["hip"] == before["hip"] + 1 and M.PATH_COUNTS["torch"] == before["torch"]
        assert torch.equal(za, mod(xa, ra)) and torch.equal(zb, mod(xb, rb))


def test_deconv_pair_and_batch_bit_identities(sa):
    for (Cin, Cout, H, W) in ((256, 64, 64, 64), (768, 256, 16, 16), (20, 12, 5, 7), (128, 6, 128, 128)):
        w, scale, shift = _deconv_params(Cin, Cout, 400 + Cin)
        g = _gen(Cin + W)
        xa, xb = torch.randn(1, Cin, H, W, generator=g).cuda(), torch.randn(1, Cin, H, W, generator=g).cuda()
        one_a, one_b = _hip_deconv(sa, xa, w, scale, shift, True), _hip_deconv(sa, xb, w, scale, shift, True)
        pair = _hip_deconv(sa, xa, w, scale, shift, True, xb=xb)
        assert torch.equal(pair[:1], one_a) and torch.equal(pair[1:], one_b), (Cin, Cout, H, W)
        # a sample alone and as element 0 of a batch of 4: the tile is chosen per layer, never per launch
        x4 = torch.cat((xa, xb, torch.randn(2, Cin, H, W, generator=g).cuda() * 100.0), 0)
        b4 = _hip_deconv(sa, x4, w, scale, shift, True)
        assert torch.equal(b4[:1], one_a) and torch.equal(b4[1:2], one_b), (Cin, Cout, H, W)


def _bound(x, w, scale, K):
    """|error| the two-term fp16 form may have against the exact layer: per product 2^-21 (two operand representations at 2^-23 and
    the dropped lo*lo at 2^-22), a K-term fp32 accumulation as a random walk with a factor 4, and two roundings of the affine --
    all relative to sum |x| |w| (times |scale|)."""
    S = F.conv_transpose2d(x.double().abs(), w.double().abs(), None, 2, 1)
    if scale is not None:
        S = S * scale.double().abs()[None, :, None, None]
    return (2.0 ** -21 + 4.0 * K ** 0.5 * 2.0 ** -24) * S + 1e-30


@pytest.mark.parametrize("Cin", [6, 20, 768])
@pytest.mark.parametrize("Cout", [6, 12, 384])
def test_deconv_edge_shapes(sa, Cin, Cout):
    for W in (1, 31, 33):
        for mode in ("relu", "plain", "shift_only"):
            H, B = 1, 3
            w, scale, shift = _deconv_params(Cin, Cout, Cin * 7 + Cout + W, bias_only=(mode == "shift_only"))
            x = torch.randn(B, Cin, H, W, generator=_gen(W + Cin))
            relu = mode == "relu"
            got = _hip_deconv(sa, x.cuda(), w, scale, shift, relu).cpu().double()
            want = _deconv_ref(x, w, scale, shift, relu, torch.float64)
            assert got.shape == want.shape == (B, Cout, 2, 2 * W)
            excess = ((got - want).abs() - _bound(x, w, scale, 4 * Cin) - 2.0 ** -22 * want.abs()).max()
            assert float(excess) <= 0.0, (Cin, Cout, W, mode, float(excess))
    # taller than one tile, ragged rows and columns, B = 3
    w, scale, shift = _deconv_params(Cin, Cout, 5)
    x = torch.randn(3, Cin, 11, 37, generator=_gen(3))
    got = _hip_deconv(sa, x.cuda(), w, scale, shift, True).cpu().double()
    want = _deconv_ref(x, w, scale, shift, True, torch.float64)
    assert float(((got - want).abs() - _bound(x, w, scale, 4 * Cin) - 2.0 ** -22 * want.abs()).max()) <= 0.0


def test_deconv_nan_and_inf_propagate(sa):
    Cin, Cout, H, W = 20, 12, 6, 40
    w, scale, shift = _deconv_params(Cin, Cout, 9)
    x = torch.randn(2, Cin, H, W, generator=_gen(9))
    clean = _hip_deconv(sa, x.cuda(), w, scale, shift, False).cpu()
    for bad in (float("nan"), float("inf"), -float("inf")):
        for relu in (False, True):
            xb = x.clone()
            xb[1, 3, 2, 17] = bad
            got = _hip_deconv(sa, xb.cuda(), w, scale, shift, relu).cpu()
            # the 4 x 4 output pixels that read input (2, 17) are not finite, in every channel; nothing else is touched
            hit = torch.zeros(2, Cout, 2 * H, 2 * W, dtype=torch.bool)
            hit[1, :, 2 * 2 - 1:2 * 2 + 3, 2 * 17 - 1:2 * 17 + 3] = True
            if relu and bad != bad:
                assert bool(torch.isnan(got[hit]).all())         # a NaN survives the ReLU, as in F.relu
            if not relu:
                assert bool((~torch.isfinite(got[hit])).all()), bad
            want = F.relu(clean) if relu else clean
            assert torch.equal(got[~hit], want[~hit]), (bad, relu)


def _fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "decoder.npz"))


def _check_fixture(t, rec, salt, what):
    """the bound the project uses for stack modules against fixtures: 1e-5 on O(1) outputs, scaled by the output's rms where the
    closed-form weights make it larger"""
    err, rms, dsum, dsq = dc.compare(t, rec, salt)
    tol = 1e-5 * max(1.0, rms)
    print(f"fixture {what}: max err {err:.2e}, rms {rms:.3f}, sum {dsum:.2e}, sum of squares {dsq:.2e} (tolerance {tol:.1e})")
    assert err <= tol, (what, err, rms)
    assert dsum <= tol and dsq <= 2 * tol, (what, dsum, dsq)  # what the per-element bound implies for the two sums


def test_twins_against_the_reference_fixture(sa):
    M, fx = sa.modules, _fixture()
    before = dict(M.PATH_COUNTS)
    with torch.no_grad():
        for n, (B, Cin, Cout, H, W, Hr, Wr) in dc.CONV2X.items():
            mod = dc.fill(M.Conv2x(Cin, Cout, deconv=True).eval(), dc.conv2x_salt(n)).cuda()
            x, rem = dc.conv2x_inputs(n)
            _check_fixture(mod(x.cuda(), rem.cuda()), fx[f"conv2x/{n}"], 0, n)
        mid = dict(M.PATH_COUNTS)
        assert mid["hip"] == before["hip"] + 1 and mid["torch"] == before["torch"] + 2       # "ragged" on HIP, "mismatch" (interpolate) on PyTorch
        fu = dc.fill(M.FeatUp().eval(), dc.FEATUP_SALT).cuda()
        featL, featR = dc.featup_inputs()
        L, R = fu([t.cuda() for t in featL], [t.cuda() for t in featR])
        for side, maps in (("L", L), ("R", R)):
            for k, t in enumerate(maps):
                _check_fixture(t, fx[f"featup/{side}{k}"], 10 + k, f"featup/{side}{k}")
        mods = {"spx32_16": M.Conv2x(256, 384, True), "spx16_8": M.Conv2x(768, 256, True), "spx8_4": M.Conv2x(512, 128, True),
                "spx4_2": M.Conv2x(256, 64, True), "spx2": M.Spx2(128, 6)}
        for name, salt in dc.SPX_SALTS.items():
            dc.fill(mods[name].eval(), salt).cuda()
        for k, t in enumerate(dc.run_spx(mods, [t.cuda() for t in dc.spx_inputs()])):
            _check_fixture(t, fx[f"spx/{k}"], 20 + k, f"spx/{k}")
    assert M.PATH_COUNTS["torch"] == mid["torch"] and M.PATH_COUNTS["hip"] == mid["hip"] + 4 + 5


def _model(sa):
    import decoder_model
    from oracle import detdata as dd
    net = decoder_model.DecoderStandIn(64, sa.modules, twins=True)
    with torch.no_grad():
        for i, (name, t) in enumerate(sorted(list(net.named_parameters()) + list(net.named_buffers()))):
            if name.endswith("num_batches_tracked") or name in ("gamma", "beta"):
                continue
            if name.endswith("running_var") or (name.endswith(".weight") and t.dim() == 1):
                t.copy_(dd.t_uniform(tuple(t.shape), 900 + i, 0.6, 1.4))
            elif t.dim() == 1:
                t.copy_(dd.t_uniform(tuple(t.shape), 900 + i, -0.1, 0.1))
            else:
                if ".conv5.0." in name or ".conv6.0." in name:
                    fan_in = t.shape[0] * 27 // 8
                elif t.dim() == 4 and t.shape[2] == 4:
                    fan_in = t.shape[0] * 4
                else:
                    fan_in = t[0].numel()
                a = (3.0 / fan_in) ** 0.5
                t.copy_(dd.t_uniform(tuple(t.shape), 900 + i, -a, a))
    return net.cuda().eval()


def test_whole_forward_with_the_decoder_on_hip(sa):
    from oracle import detdata as dd
    net = _model(sa)
    left = dd.t_normalish((1, 3, 128, 160), 951)
    right = torch.roll(left, shifts=-3, dims=3) + 0.05 * dd.t_normalish((1, 3, 128, 160), 952)
    left, right = left.cuda(), right.cuda()
    done = sa.accelerate(net, decoder=True, fuse_forward=True)
    assert done == []                                            # built from the twins already
    M = sa.modules
    with torch.no_grad():
        net(left, right)                                         # (packs the weights)
        torch.cuda.synchronize()
        before = dict(M.PATH_COUNTS)
        torch.cuda.set_sync_debug_mode("error")
        try:
            (d1,), lab1 = net(left, right)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert M.PATH_COUNTS["torch"] == before["torch"]
        assert M.PATH_COUNTS["hip"] >= before["hip"] + 4 + 4 + 1  # four pair layers of FeatUp, the spx chain, spx2
        sa.engine.DECODER_HIP = False
        try:
            mid = dict(M.PATH_COUNTS)
            (d0,), lab0 = net(left, right)
            assert M.PATH_COUNTS["torch"] >= mid["torch"] + 2 * 8 + 2 * 4 + 1
        finally:
            sa.engine.DECODER_HIP = "auto"
    assert d1.shape == d0.shape == (1, 128, 160)
    err = (d1 - d0).abs()
    print("whole forward: median", float(err.median()), "max", float(err.max()), "label max", float((lab1 - lab0).abs().max()))
    # the SSR head's tolerance (test_dropin_gpu): full-resolution disparities (x4), 1e-3 px at 1/4 scale = 4e-3 here
    assert float(err.median()) <= 1e-4 and float((err <= 4e-3).float().mean()) >= 0.995, (float(err.median()), float(err.max()))
    assert float((lab1 - lab0).abs().max()) <= 1e-4 * max(1.0, float(lab0.abs().max()))


def test_switches_route_to_pytorch_and_count_it(sa):
    M, E = sa.modules, sa.engine
    mod = dc.fill(M.Conv2x(16, 8, deconv=True).eval(), 5).cuda()
    spx2 = dc.fill(M.Spx2(16, 6).eval(), 6).cuda()
    x, rem = torch.randn(1, 16, 8, 8).cuda(), torch.randn(1, 8, 16, 16).cuda()

    def counts(fn):
        b = dict(M.PATH_COUNTS)
        y = fn()
        return y, M.PATH_COUNTS["hip"] - b["hip"], M.PATH_COUNTS["torch"] - b["torch"]
    with torch.no_grad():
        y_hip, h, t = counts(lambda: mod(x, rem))
        assert (h, t) == (1, 0)
        s_hip, h, t = counts(lambda: spx2(x))
        assert (h, t) == (1, 0)
        for name, value in (("DECODER_HIP", False), ("CONV_ENGINE", "f32")):
            old = getattr(E, name)
            setattr(E, name, value)
            try:
                y, h, t = counts(lambda: mod(x, rem))
                assert (h, t) == (0, 2), (name, h, t)
                assert torch.allclose(y, y_hip, atol=2e-5, rtol=1e-5)
                s, h, t = counts(lambda: spx2(x))
                assert (h, t) == (0, 1), (name, h, t)
                assert torch.allclose(s, s_hip, atol=2e-5, rtol=1e-5)
            finally:
                setattr(E, name, old)
    # autograd on (the parameters require grad): the stock layers, counted
    y, h, t = counts(lambda: mod(x, rem))
    assert (h, t) == (0, 2) and y.requires_grad
    y, h, t = counts(lambda: spx2(x))
    assert (h, t) == (0, 1) and y.requires_grad
