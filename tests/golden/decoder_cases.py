"""Case table of the 2-D decoder fixture (`decoder.npz`), shared by `make_golden_decoder.py` (which runs the REFERENCE's own Conv2x,
FeatUp and SemStereo.spx* on these inputs, in the build container only) and by the tests (which run the twins on the same inputs,
anywhere).  Weights, BatchNorm statistics and inputs are closed-form (`oracle.detdata`), so only reference OUTPUTS are stored.
"""
import numpy as np
import torch
import torch.nn as nn

from oracle import detdata as dd

# single Conv2x(in, out, deconv=True) layers (models/submodule.py:119-161): name -> (B, Cin, Cout, H, W, rem H, rem W)
CONV2X = {
    "ragged": (2, 20, 12, 5, 7, 10, 14),        # ragged channels (Csplit = 12: the concatenated input is materialised), odd H / W
    "mismatch": (1, 16, 8, 4, 5, 9, 11),        # rem is not 2H x 2W: the F.interpolate branch
}
# the image whose pyramid FeatUp and the spx chain run on: 64 x 96 (2 x 3 at 1/32), batch 1
PYRAMID = (1, 64, 96)
CHANS = (64, 128, 256, 384, 512)                # the backbone's maps at 1/2 .. 1/32 (models/SemStereo.py:62)
CHANS2 = (64, 128, 256, 384, 256)               # ... after chal_0 .. chal_4 (models/SemStereo.py:197)
SAMPLES = 512                                    # sampled elements of a case array that is not stored whole
WHOLE = 8192                                     # arrays up to this many elements are stored whole


def fill(module, salt):
    """Closed-form fill of every parameter and BatchNorm buffer of `module`, by sorted state_dict key: conv weights ~ U(-a, a) with
    a = sqrt(3 / fan_in) (unit gain; a 4x4 stride-2 transposed kernel feeds each output from 4 of its 16 taps), BN weight / var ~
    U(0.6, 1.4), BN bias / mean and conv bias ~ U(-0.1, 0.1).  Depends on key order and shapes only, so a twin with the reference's
    keys gets the reference's values."""
    sd = module.state_dict()
    with torch.no_grad():
        for i, key in enumerate(sorted(sd)):
            t = sd[key]
            if key.endswith("num_batches_tracked"):
                continue
            s = salt * 1000 + i
            shape = tuple(t.shape)
            if len(shape) == 4:
                fan_in = shape[0] * 4 if shape[2] == 4 else shape[1] * shape[2] * shape[3]
                v = dd.t_uniform(shape, s, -1.0, 1.0) * (3.0 / fan_in) ** 0.5
            elif key.endswith("running_var") or key.endswith(".weight"):
                v = dd.t_uniform(shape, s, 0.6, 1.4)
            else:
                v = dd.t_uniform(shape, s, -0.1, 0.1)
            t.copy_(v.float())
    return module


def conv2x_inputs(name):
    B, Cin, Cout, H, W, Hr, Wr = CONV2X[name]
    s = 1100 + sorted(CONV2X).index(name) * 2
    return dd.t_normalish((B, Cin, H, W), s), dd.t_normalish((B, Cout, Hr, Wr), s + 1)


def conv2x_salt(name):
    return 31 + sorted(CONV2X).index(name)


def pyramid(chans, salt):
    """The five maps at 1/2 .. 1/32 of PYRAMID with `chans` channels."""
    B, H, W = PYRAMID
    return [dd.t_normalish((B, c, H >> (k + 1), W >> (k + 1)), salt + k) for k, c in enumerate(chans)]


def featup_inputs():
    return pyramid(CHANS, 1200), pyramid(CHANS, 1210)


def spx_inputs():
    return pyramid(CHANS2, 1220)


FEATUP_SALT = 41
SPX_SALTS = {"spx32_16": 42, "spx16_8": 43, "spx8_4": 44, "spx4_2": 45, "spx2": 46}
SPX_ORDER = ("spx32_16", "spx16_8", "spx8_4", "spx4_2")


def run_spx(mods, feats):
    """models/SemStereo.py:267-271 on the five left maps; -> the four Conv2x outputs and spx_pred."""
    outs = []
    x = feats[4]
    for k, name in enumerate(SPX_ORDER):
        x = mods[name](x, feats[3 - k])
        outs.append(x)
    outs.append(mods["spx2"](x))
    return outs


def sample_index(numel, salt):
    u = dd.uniform((SAMPLES,), 9500 + salt, 0.0, 1.0).astype(np.float64)
    return np.minimum((u * numel).astype(np.int64), numel - 1)


def record(t, salt):
    """What the fixture keeps of a case array: the array itself where it is small, else [sum, sum of squares, SAMPLES samples]."""
    a = t.detach().double().reshape(-1)
    if a.numel() <= WHOLE:
        return t.detach().cpu().numpy().astype(np.float32)
    idx = sample_index(a.numel(), salt)
    return np.concatenate([[a.sum().item(), (a * a).sum().item()], a[idx].numpy()]).astype(np.float64)


def compare(t, rec, salt):
    """-> (max |difference| over the recorded elements, rms of the reference array, |difference of the sums| / n,
    |difference of the sums of squares| / (n rms)).  With every element within `tol` of the reference the last two are at most
    tol and 2 tol."""
    a = t.detach().double().cpu().reshape(-1)
    n = a.numel()
    if rec.dtype == np.float32:
        r = torch.from_numpy(rec.astype(np.float64)).reshape(-1)
        assert r.numel() == n, (r.numel(), n)
        rsum, rsq, err = r.sum().item(), (r * r).sum().item(), float((a - r).abs().max())
    else:
        rsum, rsq = float(rec[0]), float(rec[1])
        err = float((a[sample_index(n, salt)] - torch.from_numpy(rec[2:])).abs().max())
    rms = (rsq / n) ** 0.5
    return err, rms, abs(a.sum().item() - rsum) / n, abs((a * a).sum().item() - rsq) / (n * rms + 1e-30)
