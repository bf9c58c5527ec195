"""Closed-form inputs of the image-output fixtures (tests/golden/vis.npz): shared by make_golden_vis.py, which feeds them to the
reference's own utils/visualization.py and utils/mask_vis.py, and by the tests, which feed them to semstereo_amd.visualization.  Values
come from oracle.detdata and from float32 numpy arithmetic (IEEE), so they are the same bits wherever they are built.

Error-map inputs.  The ground truth is 60 * (u - 0.2): a fifth of it is negative, hence not valid.  The estimate is placed so that the
error measure e = min(|gt - est| / 3, |gt - est| / gt / 0.05) is log-uniform over 2^-6 .. 2^6, which fills all ten rows of the colour
table (a noise model proportional to |gt| leaves the last one, e >= 16, empty).  Rows 10 and 11 of the cases that have them carry the
special pixels, clear of the colour key: one pixel per finite threshold whose float32 e EQUALS the float32 threshold (found by a search
over float32 pairs, see `threshold_pixels`), a NaN and a +inf estimate, a NaN and a zero ground truth.  make_golden_vis.py asserts all
of this about the inputs (`check_error_inputs`), so a test cannot pass on an empty case."""
import numpy as np
import torch

from oracle import detdata as dd

NCLS = 6
ABS_THRES, REL_THRES = np.float32(3.0), np.float32(0.05)
# the ten lower bounds of utils/visualization.py:11-24, computed in float64 and cast to float32 as the reference's table is
BOUNDS = np.array([0.0, 0.1875 / 3.0, 0.375 / 3.0, 0.75 / 3.0, 1.5 / 3.0, 3 / 3.0, 6 / 3.0, 12 / 3.0, 24 / 3.0, 48 / 3.0], dtype=np.float32)

# name: batch, height, width, seed, whether rows 10 and 11 carry the special pixels
ERROR_CASES = {
    "clip_w_2x23x41": dict(B=2, H=23, W=41, seed=9810, specials=True),         # the colour key is clipped in width
    "clip_h_1x7x201": dict(B=1, H=7, W=201, seed=9820, specials=False),        # ... in height; column 200 is no key
    "exact_1x10x200": dict(B=1, H=10, W=200, seed=9830, specials=False),       # the picture IS the key
    "ragged_3x75x203": dict(B=3, H=75, W=203, seed=9840, specials=True),       # rows that start at every offset mod 4
}
# name: batch, channels, height, width, seed
LOGIT_CASES = {
    "c6_2x6x23x41": dict(B=2, C=6, H=23, W=41, seed=9910),
    "c3_1x3x12x20": dict(B=1, C=3, H=12, W=20, seed=9920),
}
# name: batch, height, width, dtype, extra rows / columns of the tensor the label map is a view of, seed
LABEL_CASES = {
    "int64_2x23x41": dict(B=2, H=23, W=41, dtype=torch.int64, pad=(0, 0), seed=9930),
    "uint8_2x12x20": dict(B=2, H=12, W=20, dtype=torch.uint8, pad=(0, 0), seed=9940),
    "float32_crop_2x20x36": dict(B=2, H=20, W=36, dtype=torch.float32, pad=(3, 5), seed=9950),
}

_THRESHOLD_PIXELS = []


def error_measure(gt, est):
    """e of utils/visualization.py:38-40 in float32 numpy, for gt > 0."""
    gt, est = np.asarray(gt, dtype=np.float32), np.asarray(est, dtype=np.float32)
    with np.errstate(all="ignore"):
        err = np.abs(gt - est)
        return np.minimum(err / ABS_THRES, (err / gt) / REL_THRES)


def threshold_pixels():
    """[(gt, est)] float32 pairs, one per finite threshold BOUNDS[1:], with error_measure(gt, est) == the threshold exactly.  The pairs
    are searched, not assumed (three roundings lie between est and e): for a grid of ground truths, est runs over the 4097 float32
    values around gt - 3 t, and the first whose float32 e equals t is taken -- for some thresholds an est next to the nominal one,
    whose e rounds onto the threshold."""
    if not _THRESHOLD_PIXELS:
        steps = np.arange(-2048, 2049, dtype=np.int64)
        for t in BOUNDS[1:]:
            found = None
            for g in np.arange(4.0, 59.0, 0.37, dtype=np.float32):
                centre = np.float32(g - np.float32(3.0) * t)
                bits = np.array([centre], dtype=np.float32).view(np.int32).astype(np.int64)[0]
                if abs(centre) < 1e-3:
                    continue                                               # (stay clear of zero: the bit pattern steps change sign there)
                ests = (bits + steps).astype(np.int32).view(np.float32)
                hit = np.nonzero(error_measure(np.full_like(ests, g), ests) == t)[0]
                if hit.size:
                    found = (np.float32(g), ests[hit[0]])
                    break
            assert found is not None, f"no float32 pair reaches the threshold {t!r}"
            _THRESHOLD_PIXELS.append(found)
    return list(_THRESHOLD_PIXELS)


def error_inputs(name):
    """float32 tensors `est`, `gt` [B,H,W]."""
    c = ERROR_CASES[name]
    B, H, W, s = c["B"], c["H"], c["W"], c["seed"]
    gt = (np.float32(60.0) * (dd.uniform((B, H, W), s, 0.0, 1.0) - np.float32(0.2))).astype(np.float32)
    t = np.exp2(dd.uniform((B, H, W), s + 1, -6.0, 6.0).astype(np.float64))                 # the error measure aimed at
    err = t * np.maximum(3.0, 0.05 * np.abs(gt.astype(np.float64)))
    sign = np.where(dd.uniform((B, H, W), s + 2) < 0, -1.0, 1.0)
    est = (gt.astype(np.float64) + sign * err).astype(np.float32)
    if c["specials"]:
        for b in range(B):
            for i, (g, e) in enumerate(threshold_pixels()):
                gt[b, 10, 2 + 4 * i], est[b, 10, 2 + 4 * i] = g, e
        gt[0, 11, 1], est[0, 11, 1] = 20.0, np.nan
        gt[0, 11, 6], est[0, 11, 6] = 20.0, np.inf
        gt[0, 11, 11], est[0, 11, 11] = np.nan, 20.0
        gt[0, 11, 16], est[0, 11, 16] = 0.0, 20.0
        gt[0, 11, 21], est[0, 11, 21] = 20.0, -np.inf
        gt[0, 11, 26], est[0, 11, 26] = np.inf, 20.0
        gt[0, 11, 31], est[0, 11, 31] = 20.0, 20.0                          # e = 0: the first row's lower bound
    return {"est": torch.from_numpy(est), "gt": torch.from_numpy(gt)}


def check_error_inputs():
    """What make_golden_vis.py asserts about the inputs."""
    for name, c in ERROR_CASES.items():
        d = error_inputs(name)
        gt, est = d["gt"].numpy(), d["est"].numpy()
        with np.errstate(invalid="ignore"):
            invalid = ~(gt > 0)
        share = invalid.mean()
        assert 0.10 <= share <= 0.60, (name, share)
        if not c["specials"]:
            continue
        e = error_measure(gt, est)
        for i, t in enumerate(BOUNDS[1:]):                                   # a pixel exactly on every finite threshold, in every image
            for b in range(c["B"]):
                assert gt[b, 10, 2 + 4 * i] > 0 and e[b, 10, 2 + 4 * i] == t, (name, b, i, e[b, 10, 2 + 4 * i], t)
        valid = ~invalid
        assert np.isnan(est[valid]).any() and np.isposinf(est[valid]).any(), name
        assert np.isnan(gt).any() and (gt == 0).any(), name
    d = error_inputs("ragged_3x75x203")
    gt, est = d["gt"].numpy(), d["est"].numpy()
    with np.errstate(invalid="ignore"):
        valid = gt > 0
    e = error_measure(gt, est)[valid]
    hi = np.append(BOUNDS[1:], np.float32(np.inf))
    for i in range(10):
        with np.errstate(invalid="ignore"):
            share = ((e >= BOUNDS[i]) & (e < hi[i])).mean()
        assert share >= 0.01, ("ragged_3x75x203", i, share)


def logit_inputs(name):
    """float32 `logits` [B,C,H,W].  Row 0 carries the edge cases: exact ties (the first maximum wins), two NaN channels at one pixel (the
    first NaN wins), a NaN beside a larger finite value (the NaN wins), +inf and -inf."""
    c = LOGIT_CASES[name]
    B, C, H, W, s = c["B"], c["C"], c["H"], c["W"], c["seed"]
    z = dd.uniform((B, C, H, W), s, -2.0, 2.0).copy()
    z[0, :, 0, 0] = 0.5                                    # all equal: class 0
    z[0, :, 0, 1] = -1.0
    z[0, 1, 0, 1] = z[0, 2, 0, 1] = 1.5                    # a tie of channels 1 and 2: class 1
    z[0, 2, 0, 2] = np.nan
    z[0, 1, 0, 2] = np.nan                                 # two NaN channels: class 1
    z[0, 0, 0, 3] = 9.0
    z[0, C - 1, 0, 3] = np.nan                             # a NaN after a larger finite value: the NaN
    z[0, 1, 0, 4] = np.inf
    z[0, 2, 0, 4] = np.inf                                 # +inf twice: class 1
    z[0, :, 0, 5] = -np.inf                                # all -inf: class 0
    z[0, 0, 0, 6] = np.nan                                 # NaN first: class 0 whatever follows
    z[0, C - 1, 0, 7] = 5.0                                # the last channel
    return {"logits": torch.from_numpy(z)}


def label_inputs(name):
    """`labels` [B,H,W] of the case's dtype with classes 0..5 -- a view into a larger tensor where the case has padding -- and `inside`,
    the same labels as a contiguous int64 tensor (what the reference's one_hot is given)."""
    c = LABEL_CASES[name]
    B, H, W, s = c["B"], c["H"], c["W"], c["seed"]
    ph, pw = c["pad"]
    full = np.minimum(np.floor(dd.uniform((B, H + ph, W + pw), s, 0.0, float(NCLS))), NCLS - 1).astype(np.int64)
    big = torch.from_numpy(full).to(c["dtype"])
    labels = big[:, :H, :W]
    return {"labels": labels, "inside": torch.from_numpy(full[:, :H, :W].copy())}
