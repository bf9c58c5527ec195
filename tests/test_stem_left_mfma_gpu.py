"""stem_left_mfma (semstereo_amd/csrc/stem_left.hip): the broadcast half of concat_stem on two fp16 terms with Q by shifts, against the
float64 convolution on the CPU, F.conv3d((att * left.unsqueeze(2)).double(), w_left.double(), padding=1), and against the kernel it
replaces (ss_stem_left_fused_fwd, six bf16 products), run in the same test.

  (a) the inputs of tests/test_parity_gpu.py (unit-gain weights, t_normalish left, att uniform in [0, 1]): max-abs error <= 2e-6 (the
      project's figure for this operand) and <= 2 x the old kernel's + 1e-7;
  (b) range cases: f16_model.ALL_RANGE_CASES on the left channels and the weight rows, a softmax tail of 12 decades across the candidates
      and three batch elements 12 decades apart in att; element-wise inside f16_bound(S, want, K = 864, BLOCK), S = sum |att| |left| |w|,
      BLOCK = 2^-38 M sum_taps |att| sum_c |w| with M the largest |left| of the output's 6 x 34 halo tile: the kernel has one block
      exponent, the left tile's (Q stays fp32 in registers, att is an fp32 operand), and the term is derived in
      tests/test_stem_left_mfma.py's docstring, where a numpy model of the kernel is held to the same bound;
  (c) a pair alone and as element 1 of a batch of 3: the same bits;  (d) two calls: the same bits;
  (e) the whole stem on the new partial sum (stem_gather_half, also writing over it) against the float64 convolution of the 64-channel
      volume: <= 2 e_full + 1e-6;
  (f) which launches of stem_broadcast_half take the kernel, restated here.

Every figure is printed; SS_STEM_LEFT_MFMA_ERR_OUT=<file> keeps the table (profiles/stem_left_mfma_err.txt is a copy of one run).
Run on the MI355X box: pytest -m gpu."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f16_model as fm
import test_stem_left_mfma as model

pytestmark = pytest.mark.gpu

SHAPES = [(2, 32, 24, 9, 37), (1, 32, 6, 5, 70), (1, 32, 32, 3, 3), (1, 32, 24, 40, 96), (1, 32, 6, 13, 65),
          (1, 32, 24, 4, 32),        # exactly one tile
          (1, 32, 24, 5, 33)]        # one row and one column past a tile
_TABLE = []


@pytest.fixture(scope="module", autouse=True)
def _dump_table():
    yield
    path = os.environ.get("SS_STEM_LEFT_MFMA_ERR_OUT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(_TABLE) + "\n")


def _record(line):
    print(line)
    _TABLE.append(line)


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    if semstereo_amd.engine.CONV_ENGINE != "f16x3":
        pytest.skip("stem_left_mfma exists for the f16x3 engine")
    return semstereo_amd


def dev(t):
    return t.cuda()


def _want(left, wl, att):
    """the float64 reference; left [B,C,H,W], wl [Cout,C,3,3,3], att [B,1,nd,H,W] (CPU)"""
    return F.conv3d((att * left.unsqueeze(2)).double(), wl.double(), padding=1)


def _new(sa, left, wl, att):
    ws = sa.ops.pack_stem_left_weights_f16s(dev(wl).reshape(32, 32, 27))
    return sa.ops.stem_left_mfma(dev(left), ws, dev(att), 32)


def _old(sa, left, wl, att):
    Cout, C = wl.shape[:2]
    wf = torch.zeros(Cout // 2, 64, C)
    wf[:, :54] = wl.reshape(Cout // 2, 2, C, 27).permute(0, 3, 1, 2).reshape(Cout // 2, 54, C)
    ws = sa.modules.pack_pointwise_weight_bf16s(dev(wf.reshape(Cout // 2 * 64, C)))
    return sa.ops.stem_left_fused(dev(left), ws, dev(att), Cout, 6)


def _parity_inputs(shape):
    from oracle import detdata as dd
    B, C, nd, H, W = shape
    left = dd.t_normalish((B, C, H, W), 301)
    att = dd.t_uniform((B, 1, nd, H, W), 303, 0.0, 1.0)
    w = dd.t_uniform((C, 2 * C, 3, 3, 3), 305, -1, 1) * (3.0 / (2 * C * 27)) ** 0.5
    return left, w, att


@pytest.mark.parametrize("shape", SHAPES)
def test_against_float64_and_the_bf16_kernel(sa, shape):
    """(a), (c'), (d)"""
    left, w, att = _parity_inputs(shape)
    wl = w[:, :32].contiguous()
    want = _want(left, wl, att)
    got, got2, old = _new(sa, left, wl, att), _new(sa, left, wl, att), _old(sa, left, wl, att)
    assert got.shape == want.shape
    e_new, e_old = float((got.double().cpu() - want).abs().max()), float((old.double().cpu() - want).abs().max())
    _record(f"parity inputs {str(shape):22s} new {e_new:.3e}   old (bf16x6) {e_old:.3e}")
    assert torch.equal(got, got2)                                                         # (d)
    assert e_new <= 2e-6, e_new
    assert e_new <= 2.0 * e_old + 1e-7, (e_new, e_old)


RANGE_SHAPE = (1, 32, 24, 5, 33)


@pytest.mark.parametrize("name", model.CASES)
def test_range_cases_inside_the_bound(sa, name):
    """(b)"""
    left, w, att = (torch.from_numpy(t) for t in model.make_case(name, RANGE_SHAPE, 29))
    wl, att5 = w.reshape(32, 32, 3, 3, 3), att.unsqueeze(1)
    want = _want(left, wl, att5)
    assert bool(torch.isfinite(want).all())
    S = F.conv3d((att5.abs() * left.abs().unsqueeze(2)).double(), wl.abs().double(), padding=1)
    A = F.conv3d(att5.abs().double(), wl.abs().double().sum(dim=1, keepdim=True), padding=1)
    block = 2.0 ** -38 * torch.from_numpy(model.tile_maxima(left.numpy()))[:, None, None] * A
    bound = fm.f16_bound(S.numpy(), want.numpy(), 864, block.numpy())
    got = _new(sa, left, wl, att5).double().cpu().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got - want.numpy())
    share = float((err / bound).max())
    _record(f"range case {name:34s} err {float(err.max()):.3e}   {share:8.3f} of f16_bound(K=864)")
    assert share <= 1.0, share


def test_a_pair_has_the_same_bits_alone_and_in_a_batch(sa):
    """(c)"""
    left, w, att = _parity_inputs((3, 32, 24, 9, 37))
    wl = w[:, :32].contiguous()
    left = left * torch.tensor([1e3, 1.0, 1e-3]).reshape(3, 1, 1, 1)            # neighbours of other magnitudes
    batch = _new(sa, left, wl, att)
    alone = _new(sa, left[1:2].contiguous(), wl, att[1:2].contiguous())
    assert torch.equal(batch[1:2], alone)


@pytest.mark.parametrize("shape", [(2, 32, 24, 9, 37), (1, 32, 6, 13, 65)])
def test_the_whole_stem_on_the_new_partial_sum(sa, shape):
    """(e)"""
    from oracle import detdata as dd
    B, C, nd, H, W = shape
    cl, cr = dd.t_normalish((B, C, H, W), 331), dd.t_normalish((B, C, H, W), 332) * 3.0
    samples = dd.distinct_sorted_candidates(B, nd, H, W, max(nd, min(W // 2, 48)), 333)
    att = dd.t_uniform((B, 1, nd, H, W), 334, 0.0, 0.7)
    stem = sa.modules.BasicConv(2 * C, C, is_3d=True, kernel_size=3, stride=1, padding=1)
    with torch.no_grad():
        stem.conv.weight.copy_(dd.t_uniform((C, 2 * C, 3, 3, 3), 336, -1, 1) * (3.0 / (2 * C * 27)) ** 0.5)
        stem.bn.weight.copy_(dd.t_uniform((C,), 337, 0.6, 1.4)); stem.bn.bias.copy_(dd.t_uniform((C,), 338, -0.1, 0.1))
        stem.bn.running_mean.copy_(dd.t_uniform((C,), 339, -0.1, 0.1)); stem.bn.running_var.copy_(dd.t_uniform((C,), 340, 0.6, 1.4))
    stem = stem.cuda().eval()
    assert sa.engine.stem_left_takes_mfma(C, C, nd)
    with torch.no_grad():
        assert sa.modules.stem_gather_applies(stem, dev(cr), dev(samples))
        partial = sa.modules.stem_broadcast_half(stem, dev(cl), dev(att))
        direct = sa.ops.stem_left_mfma(dev(cl), sa.engine._stem_halves_params(stem, C)[5], dev(att), C)
        assert torch.equal(partial, direct)                                               # the new kernel made it
        y = sa.modules.stem_gather_half(stem, dev(cr), dev(samples), dev(att), partial, None)
        y_in = sa.modules.stem_gather_half(stem, dev(cr), dev(samples), dev(att), partial.clone(), None, consume_partial=True)
        right = sa.ops.concat_volume_sampled(None, dev(cr), dev(samples), dev(att)).cpu()
        vol = torch.cat((att * cl.unsqueeze(2).expand(B, C, nd, H, W), right), dim=1)
        full = stem(dev(vol))
    sc, sh = sa.modules.fold_bn(stem.bn)
    ref = F.conv3d(vol.double(), stem.conv.weight.detach().cpu().double(), None, 1, 1)
    ref = F.relu(ref * sc.cpu().double().reshape(1, -1, 1, 1, 1) + sh.cpu().double().reshape(1, -1, 1, 1, 1))
    e_full = float((full.double().cpu() - ref).abs().max())
    for what, t in (("out of place", y), ("over the partial sum", y_in)):
        e = float((t.double().cpu() - ref).abs().max())
        _record(f"whole stem {str(shape):22s} {what:22s} {e:.3e}   full conv {e_full:.3e}")
        assert e <= 2.0 * e_full + 1e-6, (what, e, e_full)


def test_selection_rule(sa):
    """(f) the new kernel runs for: the f16x3 engine, 32 left channels, 32 output channels, 6 / 24 / 32 candidates, both switches on"""
    E = sa.engine

    def rule(engine, C, Cout, nd, fused=True, mfma=True):
        return engine == "f16x3" and fused and mfma and C == 32 and Cout == 32 and nd in (6, 24, 32)
    old = (E.CONV_ENGINE, E.STEM_LEFT_FUSED, E.STEM_LEFT_MFMA)
    try:
        for engine in ("f16x3", "bf16x6", "bf16x3"):
            for C, Cout, nd in ((32, 32, 24), (32, 32, 6), (32, 32, 32), (32, 32, 7), (32, 16, 24), (16, 16, 6)):
                for fused, mfma in ((True, True), (True, False), (False, True)):
                    E.CONV_ENGINE, E.STEM_LEFT_FUSED, E.STEM_LEFT_MFMA = engine, fused, mfma
                    assert E.stem_left_takes_mfma(C, Cout, nd) == rule(engine, C, Cout, nd, fused, mfma), (engine, C, Cout, nd, fused, mfma)
    finally:
        E.CONV_ENGINE, E.STEM_LEFT_FUSED, E.STEM_LEFT_MFMA = old
    assert "STEM_LEFT_MFMA" in E.SWITCHES and E.stem_left_takes_mfma(32, 32, 24) and not E.stem_left_takes_mfma(32, 32, 7)
    assert not E.stem_left_takes_mfma(32, 16, 24)
    # the launcher itself refuses what the rule keeps away from it
    left, att = torch.zeros(1, 32, 4, 4).cuda(), torch.zeros(1, 7, 4, 4).cuda()
    ws = sa.ops.pack_stem_left_weights_f16s(torch.zeros(32, 32, 27).cuda())
    with pytest.raises(Exception):
        sa.ops.stem_left_mfma(left, ws, att, 32)
    # ... and a fall-back shape still runs, on the old kernel: 16 output channels
    from oracle import detdata as dd
    stem = sa.modules.BasicConv(64, 16, is_3d=True, kernel_size=3, stride=1, padding=1).cuda().eval()
    cl, a = dd.t_normalish((1, 32, 5, 9), 351), dd.t_uniform((1, 1, 24, 5, 9), 352, 0.0, 1.0)
    with torch.no_grad():
        p = sa.modules.stem_broadcast_half(stem, dev(cl), dev(a))
    want = _want(cl, stem.conv.weight.detach().cpu()[:, :32], a)
    assert float((p.double().cpu() - want).abs().max()) <= 2e-6
