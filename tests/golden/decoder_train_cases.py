"""Case table of the 2-D decoder's TRAINING fixture (`decoder_train.npz`), shared by `make_golden_decoder_train.py` (which runs the
REFERENCE's own Conv2x and SemStereo.spx2 in train(), in float64, in the build container only) and by the tests (which run the twins
on the same inputs, anywhere).  Weights, BatchNorm statistics and inputs are the closed-form ones of `decoder_cases` (imported, not
edited), the loss is the closed-form linear functional <out, t_normalish(out.shape)>, so only reference RESULTS are stored: the
output, the gradients of both inputs and of every parameter, and each BatchNorm's buffers after the call.
"""
import numpy as np
import torch

from golden import decoder_cases as dc
from oracle import detdata as dd

BATCH = 2                                        # (batch statistics of one element would hide the per-batch reduction)
_, IH, IW = dc.PYRAMID                           # the 64 x 96 image of decoder_cases

# Conv2x(Cin, Cout, deconv=True) layers at the pyramid of that image: name -> (Cin, Cout, level of x); x is the map at 1 / 2^(level+1),
# the skip map the one above it.  "featup": FeatUp.deconv4_2 (models/SemStereo.py:66); "spx": spx32_16 (:208).
CONV2X = {
    "featup": (256, 64, 1),
    "spx": (256, 384, 4),
}
SPX2 = (128, 6, 0)                               # spx2 (models/SemStereo.py:207) on the map at 1/2
SALTS = {"featup": 51, "spx": 52, "spx2": 53}
WHOLE = 2048                                     # arrays up to this many elements are stored whole (float64: the bound is 1e-9)


def _map(C, level, salt):
    return dd.t_normalish((BATCH, C, IH >> (level + 1), IW >> (level + 1)), salt)


def conv2x_inputs(name):
    Cin, Cout, level = CONV2X[name]
    s = 1300 + 10 * sorted(CONV2X).index(name)
    return _map(Cin, level, s), _map(Cout, level - 1, s + 1)


def spx2_input():
    return _map(SPX2[0], SPX2[2], 1350)


def loss_weight(shape, name):
    return dd.t_normalish(tuple(shape), 1400 + SALTS[name])


def run(module, inputs, name, dtype=torch.float64, device="cpu"):
    """One train() forward + backward of loss = <module(*inputs), loss_weight> -> {key: tensor}: "out", "grad_in/k", "grad/<parameter>",
    "buf/<buffer>" (after the call)."""
    module = module.to(device=device, dtype=dtype).train()
    module.zero_grad(set_to_none=True)
    xs = [t.detach().to(device=device, dtype=dtype).clone().requires_grad_(True) for t in inputs]
    out = module(*xs)
    (out * loss_weight(out.shape, name).to(device=device, dtype=dtype)).sum().backward()
    res = {"out": out.detach()}
    res.update({f"grad_in/{k}": x.grad for k, x in enumerate(xs)})
    res.update({"grad/" + k: p.grad for k, p in module.named_parameters()})
    res.update({"buf/" + k: b.detach().clone() for k, b in module.named_buffers()})
    return res


def salt_of(key):
    """The sampling salt of a recorded array (decoder_cases.record / compare): a function of its key alone."""
    return 100 + sum(ord(c) for c in key) % 97


def record(t, salt):
    """decoder_cases.record in float64 throughout: the array itself where it is small, else [sum, sum of squares, SAMPLES samples]."""
    a = t.detach().double().reshape(-1)
    if a.numel() <= WHOLE:
        return a.numpy().astype(np.float64)
    idx = dc.sample_index(a.numel(), salt)
    return np.concatenate([[a.sum().item(), (a * a).sum().item()], a[idx].numpy()]).astype(np.float64)


def compare(t, rec, salt):
    """-> (max |difference| over the recorded elements, max |reference| over them, |difference of the sums| / n, |difference of the
    sums of squares| / (n rms)); the last two are 0 for an array stored whole."""
    a = t.detach().double().cpu().reshape(-1)
    n = a.numel()
    r = torch.from_numpy(np.asarray(rec, dtype=np.float64))
    if n <= WHOLE:
        assert r.numel() == n, (r.numel(), n)
        return float((a - r).abs().max()), float(r.abs().max()), 0.0, 0.0
    assert r.numel() == dc.SAMPLES + 2, (r.numel(), n)
    rms = (float(r[1]) / n) ** 0.5
    return (float((a[dc.sample_index(n, salt)] - r[2:]).abs().max()), float(r[2:].abs().max()), abs(a.sum().item() - float(r[0])) / n,
            abs((a * a).sum().item() - float(r[1])) / (n * rms + 1e-30))
