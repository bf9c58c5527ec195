"""Inputs that steer the training backward kernels onto each of their shape-dependent paths (tests/test_bwd_paths_gpu.py), with the
properties each case is named for computed on the CPU (tests/test_bwd_path_cases.py) -- importable without a GPU.

The probe's backward (attention_tail_bwd.hip: sample_strength_bwd_kernel, ssb_dcorr_kernel + ssb_scatter_kernel) sums the gradient of the
right features in per-wave row buffers where W % 64 == 0: a workgroup is 64 consecutive pixels of one row y, its buffer covers the columns
[xb, xb + 194), xb = (first column of the block) - 64, of row y (and, in the two-launch form, of the one other row the bilinear taps
reach); taps elsewhere go to memory with one atomic each.  Which rows and columns a tap reaches is decided by grid_sample's fp32
coordinate round trip, restated here with the kernels' own arithmetic (train_calls.warp_coords32):
    ix = ((w - d) / half_w - 1 + 1) * half_w,   iy = (h / half_h - 1 + 1) * half_h,   half = (float)((n - 1) / 2)."""
import numpy as np
import torch

import train_calls as TC
from oracle import detdata as dd
from oracle import ops as oops

#: the kernels' row-buffer geometry (attention_tail_bwd.hip: SSB_M, SSB_RB) and the pixels of one workgroup
MARGIN, ROW_BUFFER, BLOCK = 64, 64 + 2 * 64 + 2, 64


# ---- the probe (_SampleStrength) ------------------------------------------------------------------------------------------------------

def row_kinds(H):
    """Per image row y: -1 where the fp32 row coordinate lands just below y (taps in rows y - 1 and y), 0 where it is y exactly (row y
    alone), +1 where it lands just above (rows y and y + 1)."""
    _, iy = TC.warp_coords32(torch.zeros((1, 1, H, 1)), H, 1)
    iy = iy.reshape(H)
    rows = torch.arange(H, dtype=torch.float32)
    return [(-1 if float(iy[y].floor()) == y - 1 else 0 if float(iy[y]) == float(rows[y]) else 1) for y in range(H)]


def _max_lanes_on_one_slot(keys):
    """keys [n] (int64, < 0: the lane adds nothing): over the 64-lane blocks, the largest number of lanes with the same key."""
    n = keys.shape[0]
    pad = (-n) % BLOCK
    k = np.concatenate([keys, np.full(pad, -1, dtype=np.int64)]).reshape(-1, BLOCK)
    k = np.where(k < 0, -1 - np.arange(BLOCK, dtype=np.int64)[None, :], k)            # idle lanes: distinct keys
    k = np.sort(k, axis=1)
    best = 1 if (k >= 0).any() else 0
    for s in range(1, BLOCK):
        if ((k[:, s:] == k[:, :-s]) & (k[:, s:] >= 0)).any():
            best = s + 1
    return best


def tap_properties(pred0):
    """What the 5 x 4 bilinear taps of every pixel of `pred0` [B,H,W] do, from the fp32 coordinates: a tap counts where its weight is
    non-zero (the kernels skip the others)."""
    B, H, W = pred0.shape
    cand = oops.propagation(pred0.unsqueeze(1))                                       # [B,5,H,W]
    ix, iy = TC.warp_coords32(cand, H, W)
    x0, y0 = ix.floor(), iy.floor()
    fw, fn = ix - x0, iy - y0
    fe, fs = 1.0 - fw, 1.0 - fn
    xs = torch.arange(W, dtype=torch.float32).reshape(1, 1, 1, W).expand_as(ix)
    ys = torch.arange(H, dtype=torch.float32).reshape(1, 1, H, 1).expand_as(ix)
    out = {"row_above": 0, "row_same": 0, "row_below": 0, "beyond_margin": 0, "outside_window": 0, "leave_image": 0, "col_minus1": 0,
           "col_W": 0, "max_lanes_one_slot": 0}
    first = (xs // BLOCK) * BLOCK - MARGIN                                            # xb of the pixel's block where W % 64 == 0
    for dy, dx, wgt in ((0, 0, fs * fe), (0, 1, fs * fw), (1, 0, fn * fe), (1, 1, fn * fw)):
        row, col = y0 + dy, x0 + dx
        live = wgt != 0
        inside = live & (row >= 0) & (row < H) & (col >= 0) & (col < W)
        out["row_above"] += int((inside & (row == ys - 1)).sum())
        out["row_same"] += int((inside & (row == ys)).sum())
        out["row_below"] += int((inside & (row == ys + 1)).sum())
        out["beyond_margin"] += int((inside & ((col - xs).abs() > MARGIN)).sum())
        out["outside_window"] += int((inside & ((col < first) | (col >= first + ROW_BUFFER))).sum())
        out["leave_image"] += int((live & ~inside).sum())
        out["col_minus1"] += int((live & (col == -1)).sum())
        out["col_W"] += int((live & (col == W)).sum())
        image = torch.arange(B, dtype=torch.float32).reshape(B, 1, 1, 1) * (H * W)
        key = torch.where(inside, image + row * W + col, torch.full_like(row, -1.0)).to(torch.int64)
        for t in range(5):                                                            # one tagged add = one tap of one candidate, 64 lanes
            out["max_lanes_one_slot"] = max(out["max_lanes_one_slot"], _max_lanes_on_one_slot(key[:, t].reshape(-1).numpy()))
    out["min_frac"] = float((ix - ix.round()).abs().min())
    out["row_kinds"] = row_kinds(H)
    out["blocks"] = -(-B * H * W // BLOCK)
    out["lanes_in_last_block"] = (B * H * W - 1) % BLOCK + 1
    return out


def _fractional(shape, salt, lo, hi):
    return torch.round(dd.t_uniform(shape, salt, lo, hi)) + dd.t_uniform(shape, salt + 1, 0.2, 0.8)


def _pred0_collide(B, H, W, salt):
    f = dd.t_uniform((B, H, 1), salt, 0.2, 0.8)
    return (torch.arange(W, dtype=torch.float32).reshape(1, 1, W) - 70.0 + f).contiguous()


def _pred0_beyond(B, H, W, salt):
    mag = torch.round(dd.t_uniform((B, H, W), salt, 70.0, 119.0)) + dd.t_uniform((B, H, W), salt + 1, 0.2, 0.8)
    return torch.where(dd.t_uniform((B, H, W), salt + 2) > 0, mag, -mag)


#: name -> ((B, C, H, W), pred0 builder, salt)
STRENGTH_CASES = {
    "rows_exact": ((2, 20, 5, 64), lambda B, H, W, s: _fractional((B, H, W), s, -5.0, 5.0), 1100),
    "rows_below": ((1, 16, 10, 64), lambda B, H, W, s: _fractional((B, H, W), s, -5.0, 5.0), 1110),
    "rows_above": ((1, 16, 7, 128), lambda B, H, W, s: _fractional((B, H, W), s, -5.0, 5.0), 1120),
    "collide": ((1, 7, 6, 128), _pred0_collide, 1130),
    "beyond_margin": ((1, 16, 3, 256), _pred0_beyond, 1140),
    "borders": ((1, 12, 2, 192), lambda B, H, W, s: _fractional((B, H, W), s, -2.49, 1.49), 1150),
    "ragged": ((2, 9, 5, 70), lambda B, H, W, s: _fractional((B, H, W), s, -5.0, 5.0), 1160),
}


#: The taps of the second row carry weights of ~1e-7 (the distance of the fp32 row coordinate from the integer), so beside the main taps
#: their sum is far below any bound: losing all of them would go unnoticed.  These cases therefore zero `left` on the one image row whose
#: pixels put their main taps into row r of grad_right -- what is left in that row comes from the neighbouring row's second-row taps
#: alone, and is held to the bound on its own scale.  name -> r (rows_below: row 1 reaches up into row 0; rows_above: row 1 down into 2)
SECOND_ROW_ONLY = {"rows_below": 0, "rows_above": 2}


def strength_case(name):
    """-> ([left, right, pred0, var, gamma, beta], grad_strength, properties): the inputs of _SampleStrength (gamma = 0.25, beta = 2,
    var uniform in [0, 20], as test_attention_tail_training_functions_vs_float64_autograd) and the incoming gradient."""
    (B, C, H, W), make, salt = STRENGTH_CASES[name]
    left, right = dd.stereo_features(B, C, H, W, salt, max_shift=3)
    pred0 = make(B, H, W, salt + 1)
    var = dd.t_uniform((B, 1, H, W), salt + 4, 0.0, 20.0)
    go = dd.t_normalish((B, 5, H, W), salt + 5)
    props = tap_properties(pred0)
    if name in SECOND_ROW_ONLY:
        left = left.clone()
        left[:, :, SECOND_ROW_ONLY[name], :] = 0.0
        props["second_row_only"] = SECOND_ROW_ONLY[name]
    props.update(shape=(B, C, H, W), row_buffer=(W % BLOCK == 0))
    return [left, right, pred0, var, torch.tensor([0.25]), torch.tensor([2.0])], go, props


# ---- the group-wise correlation volume (_GwcVolume) -------------------------------------------------------------------------------

def gwc_rows_kernel_applies(C, W, nd, groups):
    """ss_gwc_volume_bwd's routing (gwc_volume.hip): the row-staged kernel, else one thread per element."""
    cg = C // groups
    return W <= 512 and nd <= 48 and cg <= 8 and (nd + 2 * cg) * W * 4 <= 64 * 1024


#: name -> ((B, C, G, H, W), maxdisp, signed range?, salt)
GWC_CASES = {
    "generic_cg12": ((2, 24, 2, 3, 20), 4, True, 1200),
    "generic_lds": ((1, 32, 4, 2, 512), 24, True, 1210),
    "generic_d50": ((1, 8, 2, 2, 40), 50, False, 1220),
    "rows_wide_d": ((1, 16, 4, 3, 12), 24, True, 1230),
    "same_sums": ((1, 16, 2, 4, 96), 8, True, 1240),
}


def gwc_case(name):
    """-> (ref, tgt, groups, maxdisp, signed, grad_out, properties)."""
    (B, C, G, H, W), maxdisp, signed, salt = GWC_CASES[name]
    rng = (-maxdisp, 2 * maxdisp) if signed else (0, maxdisp)
    ref, tgt = dd.t_normalish((B, C, H, W), salt), dd.t_normalish((B, C, H, W), salt + 1)
    go = dd.t_normalish((B, G, rng[1], H, W), salt + 2)
    props = {"range": rng, "rows_kernel": gwc_rows_kernel_applies(C, W, rng[1], G), "cg": C // G,
             "lds_bytes": (rng[1] + 2 * (C // G)) * W * 4, "empty_planes": sum(abs(rng[0] + i) >= W for i in range(rng[1]))}
    return ref, tgt, G, maxdisp, signed, go, props


def widen_groups(x, groups, times):
    """[B,C,H,W] -> [B,times*C,H,W]: every group's channels repeated `times` times inside the group."""
    B, C, H, W = x.shape
    return x.reshape(B, groups, 1, C // groups, H, W).expand(B, groups, times, C // groups, H, W).reshape(B, times * C, H, W).contiguous()


def narrow_groups(x, groups, times):
    """The inverse view of widen_groups: [B,times*C,H,W] -> [B,groups,times,C/groups,H,W]."""
    B, C, H, W = x.shape
    return x.reshape(B, groups, times, C // (groups * times), H, W)


# ---- the group normalisation (_GroupNormalise) --------------------------------------------------------------------------------------

GROUP_NORMALISE_SHAPE, GROUP_NORMALISE_GROUPS = (2, 16, 4, 9), 4
#: (b, group, y, x) whose four channels are all zero (features behind a ReLU), and one with a single channel left
ZERO_GROUPS = ((0, 0, 0, 0), (0, 3, 3, 8), (1, 2, 1, 4))
ONE_CHANNEL_GROUP = (1, 1, 2, 5)


def group_normalise_case():
    """-> (x, groups, grad_y, mask of the elements in all-zero groups)."""
    B, C, H, W = GROUP_NORMALISE_SHAPE
    G, cg = GROUP_NORMALISE_GROUPS, C // GROUP_NORMALISE_GROUPS
    x = dd.t_normalish((B, C, H, W), 1300).clone()
    zero = torch.zeros((B, C, H, W), dtype=torch.bool)
    for b, g, y, xx in ZERO_GROUPS:
        x[b, g * cg:(g + 1) * cg, y, xx] = 0.0
        zero[b, g * cg:(g + 1) * cg, y, xx] = True
    b, g, y, xx = ONE_CHANNEL_GROUP
    x[b, g * cg + 1:(g + 1) * cg, y, xx] = 0.0
    return x, G, dd.t_normalish((B, C, H, W), 1301), zero


# ---- the top-k candidates (_TopkCandidates) ------------------------------------------------------------------------------------------

#: (B, D, H, W, k): D = 48 with a partial second block of 64 pixels and H = 2; k == D on a one-column map; k == D, batch 2
TOPK_CASES = ((1, 48, 2, 66, 24), (1, 32, 6, 1, 32), (2, 24, 3, 5, 24))


def topk_case(shape):
    """-> (logits, strength, k, rng, grad_att_topk, grad_pred_att, properties)."""
    B, D, H, W, k = shape
    salt = 1400 + D
    logits = dd.t_normalish((B, 1, D, H, W), salt) * 3.0
    strength = torch.softmax(dd.t_normalish((B, 5, H, W), salt + 1), dim=1)
    ga, gp = dd.t_normalish((B, 1, k, H, W), salt + 2), dd.t_normalish((B, H, W), salt + 3)
    ys, xs = torch.arange(H).reshape(H, 1).expand(H, W), torch.arange(W).reshape(1, W).expand(H, W)
    border = sum(int(((ys + dy < 0) | (ys + dy >= H) | (xs + dx < 0) | (xs + dx >= W)).sum()) for dy, dx in oops._PROP_TAPS)
    props = {"border_taps": border, "off_centre_taps": 4 * H * W, "lds_bytes": D * 64 * 4}
    return logits, strength, k, (-(D // 2), D), ga, gp, props


# ---- the up-sampling soft-argmax (_UpsampleSoftmaxRegression) -----------------------------------------------------------------------------

#: coarse shapes (B, 1, Dc, Hc, Wc): a coarse axis of length 1 in H, in W, in D
UPSOFT_CASES = ((1, 1, 4, 1, 3), (1, 1, 6, 3, 1), (2, 1, 1, 2, 2))


def upsoft_case(shape):
    """-> (coarse, H, W, rng, (grad_up, grad_disp, grad_var))."""
    B, _, Dc, Hc, Wc = shape
    salt = 1500 + 10 * Dc + Hc
    D, H, W = 2 * Dc, 2 * Hc, 2 * Wc
    coarse = dd.t_normalish(shape, salt) * 2
    grads = (dd.t_normalish((B, 1, D, H, W), salt + 1), dd.t_normalish((B, H, W), salt + 2), dd.t_normalish((B, 1, H, W), salt + 3))
    return coarse, H, W, (-Dc, D), grads
