"""attention_block.final1x1 folded into hourglass.conv5 (SS_ATTN_FOLD; engine.fold_pointwise_into_deconv, the SHIFT27 form of
semstereo_amd/csrc/deconv3d_bf16s.hip) on the GPU, at the level of `hourglass`: from the attention core's output y (128 channels) and
the 64-channel skip tensor to relu(bn(conv5(final1x1(y))) + bn(redir2(skip))), un-padded and un-cropped, against float64 on the CPU.

  * two small volumes whose last odd plane, row and column land in ragged tiles: (D, H, W) = (2, 5, 37) -- H no multiple of the
    4-row tile, W beyond one 32-column tile -- and (1, 3, 6); B = 2, the f16x3 engine (and (2, 3, 5), and two of them on bf16x6);
  * the folded path (ONE launch) must be as close to float64 as today's two launches (pointwise_bf16s, deconv3d_bf16s) on the
    same input: error <= 1.5 x theirs + 1e-6 (the margin of test_parity_gpu.test_deconv3d_split_bf16_engine for two roundings of
    the same size), SEPARATELY on the border set (the last odd plane, row and column: cases 2 of the shift table) and on the
    interior, so that a wrong table entry cannot hide in the mean -- on the fp16 engine under every form of the kernel: what the
    launcher picks at this size, SS_DECONV_GROUPS = 0 / 1 / 2, and groups 0 with nontemporal stores (SS_DECONV_STREAM=1);
  * HotSegment at the s128 fixture with SS_ATTN_FOLD 0 and 1: the same candidates, `pred` / `pred_att` within the bounds of
    test_parity_gpu.test_hot_segment_with_hip_2d_convs.
Every figure is printed; SS_ATTN_FOLD_ERR_OUT=<file> keeps the table (profiles/attn_fold_err.txt is a copy of one run).
Run on the MI355X box: pytest -m gpu."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from golden import cases
from oracle import detdata as dd
from oracle import hot_segment as oseg

pytestmark = pytest.mark.gpu

_TABLE = []


@pytest.fixture(scope="module", autouse=True)
def _dump_table():
    yield
    path = os.environ.get("SS_ATTN_FOLD_ERR_OUT")
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
    return semstereo_amd


@pytest.fixture
def engine(sa, request):
    old = sa.engine.CONV_ENGINE
    sa.engine.CONV_ENGINE = request.param
    yield request.param
    sa.engine.CONV_ENGINE = old


def _hourglass(sa):
    """hourglass(32) with seeded weights on the layers this test runs: final1x1 (with bias), conv5 + BN, redir2 + BN"""
    hg = sa.modules.hourglass(32).eval()
    seed = [920]

    def fill(p, lo, hi):
        seed[0] += 1
        p.copy_(dd.t_uniform(tuple(p.shape), seed[0], lo, hi))
    with torch.no_grad():
        fin = hg.attention_block.final1x1
        fill(fin.weight, -(3.0 / 128) ** 0.5, (3.0 / 128) ** 0.5)
        fill(fin.bias, -0.5, 0.5)
        fill(hg.conv5[0].weight, -(3.0 / (128 * 27 / 8)) ** 0.5, (3.0 / (128 * 27 / 8)) ** 0.5)
        fill(hg.redir2[0].weight, -(3.0 / 64) ** 0.5, (3.0 / 64) ** 0.5)
        for bn in (hg.conv5[1], hg.redir2[1]):
            fill(bn.weight, 0.5, 1.5)
            fill(bn.bias, -0.2, 0.2)
            fill(bn.running_mean, -0.2, 0.2)
            fill(bn.running_var, 0.5, 1.5)
    return hg


def _bn64(bn, t):
    sh = (1, -1, 1, 1, 1)
    inv = 1.0 / torch.sqrt(bn.running_var.double() + bn.eps)
    return (t - bn.running_mean.double().reshape(sh)) * (bn.weight.double() * inv).reshape(sh) + bn.bias.double().reshape(sh)


# (2, 3, 5): the kernel's 2 x 2-row tile, taken where H < 4 and D >= 2; bf16x6: the table in the kernel's three-bf16-term form
@pytest.mark.parametrize("engine,shape", [("f16x3", (2, 5, 37)), ("f16x3", (1, 3, 6)), ("f16x3", (2, 3, 5)), ("bf16x6", (2, 5, 37)),
                                          ("bf16x6", (2, 3, 5))], indirect=["engine"])
def test_conv5_with_final1x1_folded(sa, engine, shape, tuning_env):
    D, H, W = shape
    hg = _hourglass(sa)
    y = dd.t_normalish((2, 128, D, H, W), 911)
    skip = dd.t_normalish((2, 64, 2 * D, 2 * H, 2 * W), 912)
    with torch.no_grad():
        fin = hg.attention_block.final1x1
        z = F.conv3d(y.double(), fin.weight.double(), fin.bias.double())
        up = F.conv_transpose3d(z, hg.conv5[0].weight.double(), None, stride=2, padding=1, output_padding=1)
        ref = F.relu(_bn64(hg.conv5[1], up) + _bn64(hg.redir2[1], F.conv3d(skip.double(), hg.redir2[0].weight.double())))
    hg = hg.cuda()
    yd, sd = y.cuda(), skip.cuda()
    M = sa.modules
    border = torch.zeros(ref.shape[2:], dtype=torch.bool)
    border[2 * D - 1], border[:, 2 * H - 1], border[:, :, 2 * W - 1] = True, True, True
    # (SS_DECONV_GROUPS, SS_DECONV_STREAM) of the SHIFT27 instantiations; the bf16 engine has one form
    forms = [(None, None)] + ([("0", "0"), ("0", "1"), ("1", None), ("2", None)] if engine == "f16x3" else [])
    for groups, stream in forms:
        if groups is not None:
            tuning_env("SS_DECONV_GROUPS", groups)
            tuning_env("SS_DECONV_STREAM", stream or "-1")
        form = "" if groups is None else f" groups {groups}" + (" stream" if stream == "1" else "")
        with torch.no_grad():
            assert hg._up_takes_split_engine("u5", hg.conv5, hg.redir2, yd) and M._deconv_nterms() == (19 if engine == "f16x3" else 6)
            _, _, wo, bo, bf = hg.attention_block._params_split()
            assert bf
            two = hg._up("u5", hg.conv5, hg.redir2, M.conv3d_pointwise_bf16s_hip(yd, wo, 128, None, bo, False, M._aux_nterms()), sd)
            one = hg._up5_folded(yd, sd)
        torch.cuda.synchronize()
        assert one.shape == two.shape == ref.shape and bool(torch.isfinite(one).all())
        e_one, e_two = (one.double().cpu() - ref).abs(), (two.double().cpu() - ref).abs()
        for name, mask in (("border", border), ("interior", ~border)):
            a, b = float(e_one[:, :, mask].max()), float(e_two[:, :, mask].max())
            _record(f"conv5 fold {engine}{form} {shape} {name:8s} ({int(mask.sum())} positions): folded {a:.3e}  two launches {b:.3e}  max|ref| {float(ref.abs().max()):.3g}")
            assert a <= 1.5 * b + 1e-6, (form, name, a, b)
        # the same bits for batch element 1 alone
        with torch.no_grad():
            alone = hg._up5_folded(yd[1:2].contiguous(), sd[1:2].contiguous())
        assert torch.equal(alone[0], one[1]), form


def test_hot_segment_fold_on_and_off(sa, golden):
    name = "s128"
    fl4, fr4, fl8, fr8, maxdisp = cases.segment_inputs(name)
    g = golden["segment"]
    old = sa.engine.ATTN_FOLD
    out = {}
    try:
        for fold in (False, True):
            sa.engine.ATTN_FOLD = fold
            seg = sa.HotSegment(cases.SEGMENT[name][3])
            res = seg.load_state_dict(oseg.deterministic_params(), strict=False)
            assert not res.unexpected_keys
            seg = seg.cuda().eval()
            with torch.no_grad():
                out[fold] = r = seg(fl4.cuda(), fr4.cuda(), fl8.cuda(), fr8.cuda())
            assert (r["samples"].cpu().numpy().astype(np.int16) == g[f"{name}/samples"]).all()
            e_att = float((r["pred_att"].cpu() - torch.as_tensor(g[f"{name}/pred_att"])).abs().max())
            err = (r["pred"].cpu() - torch.as_tensor(g[f"{name}/pred"])).abs()
            _record(f"hot segment {name} SS_ATTN_FOLD={int(fold)}: pred_att max err {e_att:.3e}, pred median {float(err.median()):.3e} "
                    f"max {float(err.max()):.3e}, {int((err > 1e-3).sum())} pixels beyond 1e-3")
            assert e_att <= 1e-3
            assert float(err.median()) <= 1e-5 and int((err > 1e-3).sum()) <= 1, float(err.max())
    finally:
        sa.engine.ATTN_FOLD = old
    assert torch.equal(out[False]["samples"], out[True]["samples"])
