"""attention_block.final1x1 folded into hourglass.conv5 (engine.fold_pointwise_into_deconv): the host-side builder of the
composed weights W' and of the 27-case shift table against float64 conv_transpose3d(conv3d(y, Wo, b), W5) * bn_scale + shift.
No GPU.  The second case has axes of length 1, where the only odd output index is the LAST one (case 2, never case 1)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import detdata as dd


def _case_of(n_out):
    """per output index of an axis of 2 N outputs: 0 = even, 1 = odd interior, 2 = the last odd index"""
    o = torch.arange(n_out)
    return torch.where(o % 2 == 0, 0, torch.where(o == n_out - 1, 2, 1))


@pytest.mark.parametrize("case", [(16, 8, 2, 3, 5), (16, 8, 1, 1, 4)])
def test_fold_pointwise_into_deconv(case):
    from semstereo_amd import engine as E
    C, Co, D, H, W = case
    y = dd.t_normalish((2, C, D, H, W), 901).double()
    wo = dd.t_uniform((C, C, 1, 1, 1), 902, -1, 1).double() * (3.0 / C) ** 0.5
    bo = dd.t_uniform((C,), 903, -0.5, 0.5).double()
    w5 = dd.t_uniform((C, Co, 3, 3, 3), 904, -1, 1).double() * (3.0 / (C * 27 / 8)) ** 0.5
    scale, shift = dd.t_uniform((Co,), 905, 0.5, 1.5).double(), dd.t_uniform((Co,), 906, -0.2, 0.2).double()
    ref = F.conv_transpose3d(F.conv3d(y, wo, bo), w5, None, stride=2, padding=1, output_padding=1)
    ref = ref * scale.reshape(1, -1, 1, 1, 1) + shift.reshape(1, -1, 1, 1, 1)

    # the builder computes in float64 and rounds to fp32 once at the end; that rounding alone (2^-24) is far above the 1e-12
    # asked of the identity, so the identity is checked on the float64 result and the fp32 form as its rounding (below)
    wf, t27 = E.fold_pointwise_into_deconv(wo, bo, w5, scale, shift, dtype=torch.float64)
    assert wf.shape == (C, Co, 3, 3, 3) and t27.shape == (27, Co) and wf.dtype == t27.dtype == torch.float64
    cd, ch, cw = _case_of(2 * D), _case_of(2 * H), _case_of(2 * W)
    row = (cd.reshape(-1, 1, 1) * 3 + ch.reshape(1, -1, 1)) * 3 + cw.reshape(1, 1, -1)          # [2D, 2H, 2W]
    got = F.conv_transpose3d(y, wf, None, stride=2, padding=1, output_padding=1) + t27[row].permute(3, 0, 1, 2).unsqueeze(0)
    err = float((got - ref).abs().max()) / float(ref.abs().max())
    print(f"fold {case}: max |diff| / max |ref| = {err:.3e}")
    assert err <= 1e-12, err
    # all three border cases of every axis were hit (N = 1: cases 0 and 2 only -- there is no odd interior index)
    for c, n in ((cd, D), (ch, H), (cw, W)):
        assert set(c.tolist()) == ({0, 1, 2} if n > 1 else {0, 2})
    if min(D, H, W) > 1:
        assert set(row.reshape(-1).tolist()) == set(range(27))

    # the fp32 form the GPU path packs is that result rounded once
    wf32, t2732 = E.fold_pointwise_into_deconv(wo, bo, w5, scale, shift)
    assert wf32.dtype == t2732.dtype == torch.float32
    assert torch.equal(wf32, wf.float()) and torch.equal(t2732, t27.float())
