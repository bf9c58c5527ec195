"""`train.concat_volume_sampled` (models/SemStereo.py:316-318 under autograd, one launch each way) at quarter-resolution widths that are
no multiple of 64, behind `train.CONCAT_VOLUME_ANY_WIDTH` (SS_TRAIN_CONCAT_ANY_WIDTH=1, off by default): rows narrower than a wave,
a partial last block per row, windows that reach past the row end.  Same generators, same fp32 CPU reference (the oracle's restatement
of the reference's warp + cat + multiply) and same bounds as tests/test_parity_gpu.py::test_concat_volume_training_one_launch_each_way:
the arithmetic per pixel is that kernel's, only the pixel-to-lane mapping is new.  Run on the MI355X box: pytest -m gpu."""
import pytest
import torch

from oracle import ops as oops
# (the parity suite's own comparison: max |a - ref| <= atol + rtol * max |ref|, a NaN that both sides have -- H == 1 divides by
# (H - 1) / 2 in the reference and in the kernels alike -- counted as agreement)
from test_parity_gpu import check, dev

pytestmark = pytest.mark.gpu

CASES = [
    # (B, C, H, W, nd, kind, margin)
    (1, 32, 6, 40, 24, "int", 16),          # a row narrower than a wave: one partial block per row (the 160-wide image)
    (2, 12, 5, 72, 6, "int", 16),           # one whole block + an 8-lane tail, a wave with 4 of its 8 channels, batch 2
    (1, 40, 4, 200, 5, "frac", 64),         # two channel groups on the grid (grad_att through atomics), fractional candidates, window past the row end
    (1, 8, 7, 70, 24, "int", 2),            # width no multiple of 4, every tap beyond the margin
    (1, 16, 1, 33, 3, "frac", 8),           # H == 1, odd width
    (1, 32, 3, 224, 24, "int", 16),         # the 896-wide crop's rows
]
_REF = {}


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    return semstereo_amd


def _reference(case):
    """inputs and the fp32 CPU run (forward, three gradients) of a case: computed once, read-only afterwards"""
    if case not in _REF:
        from oracle import detdata as dd
        B, C, H, W, nd, kind, _ = case
        left, right = dd.t_normalish((B, C, H, W), 881), dd.t_normalish((B, C, H, W), 882)
        d = dd.distinct_sorted_candidates(B, nd, H, W, max(nd, 20), 883) if kind == "int" else dd.t_uniform((B, nd, H, W), 883, -20.0, 20.0)
        att = dd.t_uniform((B, 1, nd, H, W), 884, 0.0, 1.0)
        seed = dd.t_normalish((B, 2 * C, nd, H, W), 885)
        rs = [t.clone().requires_grad_(True) for t in (left, right, att)]
        right_w, left_b = oops.SpatialTransformer_grid(rs[0], rs[1], d)
        ref = rs[2] * torch.cat((left_b, right_w), dim=1)
        (ref * seed).sum().backward()
        _REF[case] = dict(left=left, right=right, d=d, att=att, seed=seed, fwd=ref.detach(), grads=[r.grad for r in rs])
    return _REF[case]


def _applies_both_ways(T, monkeypatch, R):
    args = [dev(R[k]) for k in ("left", "right", "d", "att")]
    monkeypatch.setattr(T, "CONCAT_VOLUME_ANY_WIDTH", False)
    assert not T.concat_volume_applies(*args), "the default must keep the statements at this width"
    monkeypatch.setattr(T, "CONCAT_VOLUME_ANY_WIDTH", True)
    assert T.concat_volume_applies(*args)


@pytest.mark.parametrize("case", CASES)
def test_concat_volume_training_one_launch_any_width(sa, monkeypatch, case):
    R = _reference(case)
    T = sa.train
    _applies_both_ways(T, monkeypatch, R)
    xs = [dev(R[k]).clone().requires_grad_(True) for k in ("left", "right", "att")]
    vol = T.concat_volume_sampled(xs[0], xs[1], dev(R["d"]), xs[2], margin=case[-1])
    (vol * dev(R["seed"])).sum().backward()
    torch.cuda.synchronize()
    check(f"train/concat_anywidth/{case}/fwd", vol, R["fwd"], 2e-6, 2e-6)
    for name, a_, r_ in zip(("left", "right", "att"), xs, R["grads"]):
        check(f"train/concat_anywidth/{case}/grad_{name}", a_.grad, r_, 1e-5, 3e-6)


@pytest.mark.parametrize("only", ["left", "right"])
def test_one_input_requires_grad(sa, monkeypatch, only):
    """the kernel's g_right == NULL / g_att == NULL (and g_left == NULL) branches at a ragged width"""
    case = CASES[1]
    R = _reference(case)
    T = sa.train
    _applies_both_ways(T, monkeypatch, R)
    xs = [dev(R[k]).clone().requires_grad_(k == only) for k in ("left", "right", "att")]
    vol = T.concat_volume_sampled(xs[0], xs[1], dev(R["d"]), xs[2], margin=case[-1])
    (vol * dev(R["seed"])).sum().backward()
    torch.cuda.synchronize()
    i = ("left", "right").index(only)
    assert xs[1 - i].grad is None and xs[2].grad is None
    check(f"train/concat_anywidth/only_{only}/grad", xs[i].grad, R["grads"][i], 1e-5, 3e-6)


@pytest.mark.parametrize("case", CASES[:2])
def test_no_write_outside_the_gradients(sa, monkeypatch, case):
    """The three gradients are allocated INSIDE larger buffers filled with a sentinel (the backward's `torch.empty_like` is handed a
    slice of a padded buffer): after the backward the gradients are right and every element before and after each is the sentinel."""
    R = _reference(case)
    T = sa.train
    _applies_both_ways(T, monkeypatch, R)
    PAD, SENTINEL = 4096, -12345.5
    pads = []

    class TorchWithPaddedEmptyLike:
        """what semstereo_amd.train sees as `torch` during the backward: torch, except that empty_like returns the middle of a padded buffer"""

        def __getattr__(self, name):
            return getattr(torch, name)

        @staticmethod
        def empty_like(t):
            buf = torch.full((t.numel() + 2 * PAD,), SENTINEL, dtype=t.dtype, device=t.device)
            pads.append(buf)
            return buf[PAD:PAD + t.numel()].view(t.shape)
    xs = [dev(R[k]).clone().requires_grad_(True) for k in ("left", "right", "att")]
    vol = T.concat_volume_sampled(xs[0], xs[1], dev(R["d"]), xs[2], margin=case[-1])
    loss = (vol * dev(R["seed"])).sum()
    with monkeypatch.context() as m:
        m.setattr(T, "torch", TorchWithPaddedEmptyLike())
        loss.backward()
        torch.cuda.synchronize()
    assert len(pads) == 3, len(pads)
    for name, buf, r_ in zip(("left", "right", "att"), pads, R["grads"]):
        assert bool((buf[:PAD] == SENTINEL).all()) and bool((buf[-PAD:] == SENTINEL).all()), f"grad_{name}: a write outside the tensor"
        check(f"train/concat_anywidth/padded/{case}/grad_{name}", buf[PAD:-PAD].view(r_.shape), r_, 1e-5, 3e-6)
