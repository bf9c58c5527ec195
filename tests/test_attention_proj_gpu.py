"""attention_block's "proj" form (ss_window_attention_proj_fwd, semstereo_amd/csrc/window_attention.hip): the (window, 4 heads) core
that projects its own q/k/v slab from x, against the oracle's restatement of the block and against the "split" form whose first
two launches it replaces.  The five shapes of test_parity_gpu.test_attention_block_forms_agree (T = 64 / 96; padding of both
axes, of one, of none; the scalar-load fallback of W % 4 != 0), B = 2, the same seeded weights and input.

  * the block in the proj form against oracle.stack.attention_block: <= 2e-5 (the project's bound for this block);
  * the core's output (before final1x1) bit-identical to the split form's: the in-kernel projection keeps pointwise_bf16s's
    packed fragments, K-steps, product order and bias add, so the slab holds the bits that launch writes;
  * batch element 1 alone gives the bits it gives in the batch of 2.
Run on the MI355X box: pytest -m gpu."""
import pytest
import torch

from oracle import detdata as dd
from oracle import stack as ostack

pytestmark = pytest.mark.gpu

SHAPES = [((4, 4, 4), 8, 8, 12), ((6, 4, 4), 6, 8, 8), ((4, 4, 4), 4, 6, 7), ((6, 4, 4), 12, 5, 8), ((4, 4, 4), 4, 9, 3)]


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    return semstereo_amd


def maxerr(a, ref):
    return float((a.detach().float().cpu() - torch.as_tensor(ref).float()).abs().max())


def check(name, a, ref, atol):
    e = maxerr(a, ref)
    print(f"{name}: max abs err {e:.3e}")
    assert e <= atol, f"{name}: max abs err {e:.3e} > {atol:.1e}"


def _block(sa, block):
    mod = sa.modules.attention_block(128, 16, block).cuda().eval()
    with torch.no_grad():
        for i, p in enumerate(mod.parameters()):
            a = (3.0 / 128) ** 0.5 if p.dim() > 1 else 0.2
            p.copy_(dd.t_uniform(tuple(p.shape), 600 + i, -a, a).cuda())
    return mod


def _run(sa, mod, x, form, final=True):
    old = sa.engine.ATTENTION_FORM
    sa.engine.ATTENTION_FORM = form
    try:
        with torch.no_grad():
            return mod(x, final=final)
    finally:
        sa.engine.ATTENTION_FORM = old


@pytest.mark.parametrize("shape", SHAPES)
def test_attention_proj_form(sa, shape):
    if sa.engine.CONV_ENGINE == "f32":
        pytest.skip("the proj form projects on the split-bf16 matrix core; the f32 engine keeps the split form")
    block, D, H, W = shape
    mod = _block(sa, block)
    x = dd.t_normalish((2, 128, D, H, W), 610).cuda()
    P = {"ab." + k: v.detach().cpu() for k, v in mod.state_dict().items()}
    ref = ostack.attention_block(P, "ab", x.cpu(), block)
    before = dict(sa.modules.PATH_COUNTS)
    out = _run(sa, mod, x, "proj")
    assert sa.modules.PATH_COUNTS["torch"] == before["torch"]
    check(f"attention_proj/{shape}", out, ref, 2e-5)

    y_proj, y_split = _run(sa, mod, x, "proj", final=False), _run(sa, mod, x, "split", final=False)
    assert bool(torch.isfinite(y_proj).all())
    assert torch.equal(y_proj, y_split), f"core output differs from the split form's: {maxerr(y_proj, y_split.cpu()):.3e}"
    assert torch.equal(out, _run(sa, mod, x, "split"))

    alone = _run(sa, mod, x[1:2].contiguous(), "proj", final=False)
    assert torch.equal(alone[0], y_proj[1]), "batch element 1 alone differs from itself in the batch of 2"
