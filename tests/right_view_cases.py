"""What the right-view tests share (test infrastructure, like abi.py): the case generator and a SEQUENTIAL restatement of the definitions
of include/semstereo_hip.h (section "right-view ground truth"), written for these tests from those definitions: per row, the sources in
ascending x, a plain assignment into an owner list (so the last writer, the largest x, owns a column), then the three outputs.  All
arithmetic is numpy float32 scalars: `np.float32(x) - d` and np.rint, half to even."""
import numpy as np
import torch

FILL_DISPARITY, FILL_LABEL = -999.0, 5.0

#: name -> (B, H, W, maxdisp): the smallest shapes at which each mechanism can go wrong
CASES = {
    "quads_w7": (1, 3, 7, 4),            # less than two quads, W % 4 == 3, odd W
    "batch_w37": (2, 5, 37, 8),          # batch and row indexing, odd W
    "trips_w1030": (1, 4, 1030, 48),     # more than 256 * 4 columns: a lane makes a second trip; W % 4 == 2, even W
    "leaving_w64": (1, 2, 64, 64),       # most pixels leave the row
    "wide_w8200": (1, 2, 8200, 48),      # wider than the kernel's limit: the composition, silently
}
KERNEL_CASES = tuple(k for k in CASES if CASES[k][2] <= 8192)


def make_case(name):
    """(disparity float32 [B,H,W], label int64 [B,H,W], lo, hi) of a case, with the planted values:
    every column x % 11 == 10 is -999; row 0 of image 0 has x=0 d=0.5 and x=1 d=1.5 (both aim at -0.5, which rounds to -0: column 0, and
    x=1 owns it) and x=W-1 d=-0.5 (W - 0.5: column W-1 for an odd W, column W -- outside -- for an even one); NaN, +inf, -inf, d == lo
    (kept) and d == hi (dropped) stand at x = 2..6 of row 0 (W >= 8) or row 1; the last row of the last image is all invalid."""
    B, H, W, maxdisp = CASES[name]
    g = torch.Generator().manual_seed(9100 + W)
    u = (2 * torch.rand(B, H, W, generator=g) - 1) * 1.2 * maxdisp
    d = torch.round(u * 2) / 2
    label = torch.randint(0, 6, (B, H, W), generator=g)
    lo, hi = float(-maxdisp), float(maxdisp)
    d[:, :, 10::11] = -999.0
    d[0, 0, 0], d[0, 0, 1], d[0, 0, W - 1] = 0.5, 1.5, -0.5
    x = torch.arange(W)
    d[0, 0][(x > 1) & (torch.round(x.float() - d[0, 0]) == 0)] += 1.0     # (no other pixel of that row aims at column 0)
    row = 0 if W >= 8 else 1
    d[0, row, 2], d[0, row, 3], d[0, row, 4], d[0, row, 5], d[0, row, 6] = float("nan"), float("inf"), float("-inf"), lo, hi
    bad = torch.tensor([float("nan"), -999.0, hi, float("inf"), hi + 0.5, lo - 0.5, float("-inf")])
    d[B - 1, H - 1] = bad[torch.arange(W) % len(bad)]
    return d.contiguous(), label, lo, hi


def _targets(row, lo, hi):
    W = len(row)
    tgt = [-1] * W
    for x in range(W):
        v = row[x]
        if lo <= v < hi:                                     # (False for a NaN)
            t = np.rint(np.float32(x) - v)
            if 0 <= t < W:
                tgt[x] = int(t)
    return tgt


def restate(disparity, label, lo, hi, fill_disparity=FILL_DISPARITY, fill_label=FILL_LABEL):
    """{"right_disparity", "right_label" (with a label), "left_visible"} as torch tensors, from the sequential loop."""
    d = disparity.numpy().astype(np.float32)
    y = None if label is None else label.numpy()
    lo, hi = np.float32(lo), np.float32(hi)
    B, H, W = d.shape
    rd = np.full((B, H, W), fill_disparity, dtype=np.float32)
    rl = np.full((B, H, W), fill_label, dtype=np.float32)
    vis = np.zeros((B, H, W), dtype=bool)
    for b in range(B):
        for h in range(H):
            tgt = _targets(d[b, h], lo, hi)
            owner = [-1] * W
            for x in range(W):
                if tgt[x] >= 0:
                    owner[tgt[x]] = x
            for r in range(W):
                if owner[r] >= 0:
                    rd[b, h, r] = d[b, h, owner[r]]
                    if y is not None:
                        rl[b, h, r] = np.float32(y[b, h, owner[r]])
            for x in range(W):
                vis[b, h, x] = tgt[x] >= 0 and owner[tgt[x]] == x
    out = {"right_disparity": torch.from_numpy(rd), "left_visible": torch.from_numpy(vis)}
    if y is not None:
        out["right_label"] = torch.from_numpy(rl)
    return out


def restate_lr(disp_left, disp_right, lo, hi, threshold):
    """(consistent bool, diff float32) of the left-right check, pixel by pixel."""
    dl, dr = disp_left.numpy().astype(np.float32), disp_right.numpy().astype(np.float32)
    lo, hi, threshold = np.float32(lo), np.float32(hi), np.float32(threshold)
    B, H, W = dl.shape
    diff = np.full((B, H, W), np.inf, dtype=np.float32)
    for b in range(B):
        for h in range(H):
            tgt = _targets(dl[b, h], lo, hi)
            for x in range(W):
                if tgt[x] >= 0 and lo <= dr[b, h, tgt[x]] < hi:
                    diff[b, h, x] = np.abs(dl[b, h, x] - dr[b, h, tgt[x]])
    return torch.from_numpy(diff <= threshold), torch.from_numpy(diff)


_MEMO = {}


def case(name):
    """(disparity, label, lo, hi, restatement), computed once and shared: leave it unchanged."""
    if name not in _MEMO:
        d, y, lo, hi = make_case(name)
        _MEMO[name] = (d, y, lo, hi, restate(d, y, lo, hi))
    return _MEMO[name]


def right_estimate(name):
    """A right-view estimate for the consistency cases: the case's own right view, every third column moved by a quarter or made
    invalid (NaN, the fill value is one already), so that every branch of the definition occurs."""
    d, _, lo, hi, want = case(name)
    dr = want["right_disparity"].clone()
    dr[..., 1::3] += 0.25
    dr[..., 5::7] = float("nan")
    return dr


def closed_forms():
    """(what, disparity [1,1,W], label [1,1,W], maxdisp, right_disparity, right_label, left_visible) as literals."""
    F, L = FILL_DISPARITY, FILL_LABEL
    y = [1, 2, 3, 4, 0, 1, 2, 3, 4, 0]                       # W = 10
    t = lambda v, dtype=torch.float32: torch.tensor(v, dtype=dtype).view(1, 1, -1)        # noqa: E731
    yf = [float(v) for v in y]
    forms = [
        # d == 0: identity, everything visible
        ("zero", [0.0] * 10, [0.0] * 10, yf, [True] * 10),
        # d == 3: right[r] = left[r + 3], 3 fill columns at the right border, 7 pixels visible (the first three leave the row)
        ("shift_3", [3.0] * 10, [3.0] * 7 + [F] * 3, yf[3:] + [L] * 3, [False] * 3 + [True] * 7),
        # d == -2: right[r] = left[r - 2], 2 fill columns at the left border, 8 pixels visible
        ("shift_-2", [-2.0] * 10, [F] * 2 + [-2.0] * 8, [L] * 2 + yf[:8], [True] * 8 + [False] * 2),
        # a step up at s = 5, k = 2: the near surface x >= 5 moves left onto columns 3..7 and hides exactly the left pixels 3, 4; the
        # columns nothing reaches are the last two
        ("step_up", [0.0] * 5 + [2.0] * 5, [0.0] * 3 + [2.0] * 5 + [F] * 2, yf[:3] + yf[5:] + [L] * 2, [True] * 3 + [False] * 2 + [True] * 5),
        # a step down at s = 5, k = 2: the surface x >= 5 moves right, the 2 columns 5, 6 become holes, nothing is hidden and the last
        # two pixels leave the row
        ("step_down", [0.0] * 5 + [-2.0] * 5, [0.0] * 5 + [F] * 2 + [-2.0] * 3, yf[:5] + [L] * 2 + yf[5:8], [True] * 8 + [False] * 2),
    ]
    return [(what, t(d), t(y, torch.int64), 4, t(rd), t(rl), t(vis, torch.bool)) for what, d, rd, rl, vis in forms]
