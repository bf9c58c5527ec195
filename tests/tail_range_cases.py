"""Inputs that take the attention tail (models/SemStereo.py:279-310; attention_tail.hip, attention_tail_bwd.hip) and its training consumer,
the sparse concat volume (warp.hip: ss_concat_sampled_bwd), over every plane count, disparity range and tie pattern of their dispatch
(tests/test_tail_ranges_gpu.py), with the properties each case is named for computed on the CPU (tests/test_tail_range_cases.py) --
importable without a GPU.

The selection (ss_topk_candidates_fwd) keeps the K most probable of D planes per pixel, descending, ties to the lower index (a stable
sort), and emits them ascending.  Which plane wins a tie is decided by exact equality of fp32 probabilities, so the tie inputs are built
to make that equality a property of the INPUT, not of an evaluation order:

    plane d = level[d] + field,      field: one [B,1,1,H,W] map shared by all planes

Planes of one level are bitwise identical as whole planes, so their propagated logits and probabilities are bitwise equal however they
are formed; distinct levels are at least 0.5 apart, so no rounding decides an order.  The expected candidates then follow from the
integer levels alone (`expected_planes`): sort the planes by (-level, index), take K, sort ascending."""
import torch
import torch.nn.functional as F

import bwd_path_cases as BP
from oracle import detdata as dd
from oracle import ops as oops

#: the one map shape of these tests: 270 pixels -- a partial last block for the 64-pixel kernels (4 blocks + 14) and for the 128-thread
#: kernel (2 blocks + 14), every border tap of the five-tap propagation present (H = 5 > 2, W = 27 > 2)
B, H, W = 2, 5, 27

# ---- the dispatch, restated (attention_tail.hip: ss_topk_candidates_fwd, ss_softmax_regress_split_launch) -------------------------------

TOPK_MAX_D = 128
TOPK_LDS_THREADS = 128


def topk_kernel(D):
    """-> (kernel, bytes of dynamic LDS, whether the launch goes through ensure_dynamic_lds) for ss_topk_candidates_fwd at D planes."""
    if D > TOPK_MAX_D:
        return None, 0, False
    if D in (32, 64, 96):
        return f"split<{D}>", 0, False
    lds = 2 * D * TOPK_LDS_THREADS * 4
    return "lds", lds, lds > 64 * 1024


def softarg_kernel(D):
    """-> (NCH of softmax_regress_split or None, 16-plane chunks with a plane, planes of the last such chunk, (round, wave) pairs of
    the kernel that hold no plane at all)."""
    if D > 128:
        return None, 0, 0, []
    nch = 1 if D <= 64 else 2
    chunks = -(-D // 16)
    idle = [(n, w) for n in range(nch) for w in range(4) if (n * 4 + w) * 16 >= D]
    return nch, chunks, D - 16 * (chunks - 1), idle


def ranges(D):
    """The three disparity ranges (dmin, D): signed, unsigned (WHU), and one asymmetric -- the ABI defines plane p as dmin + p."""
    return {"signed": (-(D // 2), D), "unsigned": (0, D), "asym": (-8, D)}


def quarter(d, D):
    """The wave of topk_candidates_split that owns plane d: quarter [q D/4, (q+1) D/4)."""
    return min(4 * d // D, 3)


# ---- tie patterns ----------------------------------------------------------------------------------------------------------------------

#: levels at or below (max - ZERO_BELOW) have an fp32 probability of exactly 0: expf(-150) underflows past the smallest subnormal
#: (1.4e-45 = exp(-103.3)) whatever the rounding of the exponent's argument
ZERO_BELOW = 150.0


def _scatter(D, n, exclude=()):
    """n plane indices outside `exclude`, spread over the whole axis in a fixed hashed order (so that every quarter holds winners and
    losers and no pattern degenerates into 'the first planes win')."""
    order = sorted((d for d in range(D) if d not in exclude), key=lambda d: ((d * 2654435761 + 12345) >> 5) % 1009)
    assert 0 <= n <= len(order), (D, n, len(order))
    return sorted(order[:n])


def _rest(D, *taken):
    used = set().union(*taken)
    return [d for d in range(D) if d not in used]


def _qstart(q, D):
    """The first plane of quarter q (the smallest d with 4 d // D >= q)."""
    return -(-q * D // 4)


def cross_wave_members(D):
    """Six planes, at least one in each quarter, on either side of the first and of the last quarter boundary."""
    q1, q2, q3 = (_qstart(q, D) for q in (1, 2, 3))
    return sorted({q1 - 1, q1, q2 + 1, q3 - 1, q3, D - 1})


def whole_members(D):
    q1, q2, q3 = (_qstart(q, D) for q in (1, 2, 3))
    return sorted({1, q1 + 1, q2 + 2, q3 + 1})


def partial_members(D):
    q1, q2, q3 = (_qstart(q, D) for q in (1, 2, 3))
    return sorted({q1 - 1, q1, q2 - 1, q2, D - 2, D - 1})


def levels_of(pattern, D, K, shift=0):
    """-> (levels [D] of floats, info dict) of tie pattern `pattern` at D planes and K candidates."""
    lv = [None] * D
    info = {}
    if pattern == "all_equal":
        return [0.25] * D, info
    if pattern == "cross_wave":
        grp = cross_wave_members(D)
        above = _scatter(D, K - 3, grp)
        for j, d in enumerate(above):
            lv[d] = 6.0 + 0.5 * j
        for d in grp:
            lv[d] = 5.0
        for j, d in enumerate(_rest(D, grp, above)):
            lv[d] = 3.5 - 0.5 * j
        info.update(group=grp, above=above)
        return lv, info
    if pattern == "whole_then_partial":
        whole, part = whole_members(D), partial_members(D)
        above = _scatter(D, max(K - 7, 0), whole + part)
        for j, d in enumerate(above):
            lv[d] = 10.0 + 0.5 * j
        for d in whole:
            lv[d] = 8.0
        for d in part:
            lv[d] = 5.0
        for j, d in enumerate(_rest(D, whole, part, above)):
            lv[d] = 3.5 - 0.5 * j
        info.update(whole=whole, partial=part, above=above)
        return lv, info
    if pattern == "pairs":
        return [float((d // 2 + shift) % 7) for d in range(D)], info
    if pattern == "underflow":
        near = _scatter(D, K - 4)
        for j, d in enumerate(near):
            lv[d] = -0.5 * j
        # the others in index order at -180, -170, -160, -150, ...: float64 would take the -150 ones, fp32 ties all of them by index
        for j, d in enumerate(_rest(D, near)):
            lv[d] = -180.0 + 10.0 * (j % 4)
        info.update(near=near)
        return lv, info
    if pattern == "subnormal":
        near = _scatter(D, K - 4)
        sub = _scatter(D, 7, near)
        for j, d in enumerate(near):
            lv[d] = -1.0 * j
        for j, d in enumerate(sub):            # ascending index = ascending level: the four winners are the HIGHEST indices of the seven
            lv[d] = -102.0 + 2.0 * j
        for j, d in enumerate(_rest(D, near, sub)):
            lv[d] = -180.0 + 10.0 * (j % 4)
        info.update(near=near, sub=sub)
        return lv, info
    raise KeyError(pattern)


def expected_planes(levels, K, zero_below=None):
    """The integer rule: planes sorted by (-level, index), the first K, ascending.  `zero_below`: every level <= max - zero_below is
    one tie group (fp32 probability exactly 0)."""
    top = max(levels)
    key = [(float("-inf") if (zero_below is not None and v <= top - zero_below) else v) for v in levels]
    order = sorted(range(len(levels)), key=lambda d: (-key[d], d))
    return sorted(order[:K])


def tie_groups(levels, K, zero_below=None):
    """-> list of (level, members, planes strictly above) of the tie groups that reach into the first K ranks, best first."""
    top = max(levels)
    key = [(float("-inf") if (zero_below is not None and v <= top - zero_below) else v) for v in levels]
    out = []
    for v in sorted(set(key), reverse=True):
        above = sum(1 for u in key if u > v)
        if above >= K:
            break
        out.append((v, [d for d, u in enumerate(key) if u == v], above))
    return out


def tie_inputs(levels, salt, shape=(B, H, W)):
    """-> (logits [B,1,D,H,W], strength [B,5,H,W]) fp32: plane d = levels[d] + one shared field."""
    b, h, w = shape
    field = 0.05 * dd.t_normalish((b, 1, 1, h, w), salt)
    logits = (torch.tensor(levels, dtype=torch.float32).reshape(1, 1, -1, 1, 1) + field).contiguous()
    strength = torch.softmax(dd.t_normalish((b, 5, h, w), salt + 1), dim=1)
    return logits, strength


def random_inputs(D, salt, shape=(B, H, W)):
    b, h, w = shape
    return dd.t_normalish((b, 1, D, h, w), salt) * 3.0, torch.softmax(dd.t_normalish((b, 5, h, w), salt + 1), dim=1)


def oracle_picks(logits, strength, K, dtype):
    """The oracle composition of :295-303 in `dtype` on the CPU -> (selected plane indices [B,K,H,W] ascending, prob [B,D,H,W]).
    The sum over the five taps is written tap by tap (elementwise adds): ATen's `.sum(dim=1)` walks the flattened D * H * W axis in
    vectors and finishes the last D * H * W % 32 elements in another association, so that in fp32 the end of the last plane can differ
    by an ulp from its bitwise-identical twins (seen at D = 66: 8910 % 32 = 14) -- an artefact of that reduction's blocking, not of
    the operation."""
    lg, st = logits.to(dtype), strength.to(dtype)
    taps = oops.propagation_prob(lg)
    aw = torch.zeros_like(lg)
    for t in range(5):
        aw = aw + taps[:, t:t + 1] * st[:, t:t + 1].unsqueeze(2)
    prob = F.softmax(aw, dim=2)
    _, ind = prob.sort(dim=2, descending=True, stable=True)
    return ind[:, :, :K].sort(2, False)[0].squeeze(1), prob.squeeze(1)


def planes_tensor(planes, shape=(B, H, W)):
    b, h, w = shape
    return torch.tensor(planes, dtype=torch.int64).reshape(1, -1, 1, 1).expand(b, len(planes), h, w)


PATTERNS = ("all_equal", "cross_wave", "whole_then_partial", "pairs", "underflow", "subnormal")
#: every pattern at the split kernels' D and at two D of the LDS kernel (66: the first past 64 KiB of LDS; 128: the limit), signed, K = 24;
#: `pairs` at D = 64 puts the cut ON a group boundary (8 + 8 + 8 planes at the levels 6, 5, 4), which is an edge of its own (the quota
#: equals the group), so D = 64 runs the pattern a second time shifted by three pairs, where the cut falls inside the level-4 group
TIE_D = (32, 64, 96, 66, 128)


def tie_cases():
    """-> list of (pattern, D, K, range name, shift)."""
    out = []
    for D in TIE_D:
        for p in PATTERNS:
            out.append((p, D, 24, "signed", 0))
        if D == 64:
            out.append(("pairs", 64, 24, "signed", 3))
    for D in TIE_D:                                   # patterns 1 to 3 on the unsigned range ...
        for p in PATTERNS[:3]:
            out.append((p, D, 24, "unsigned", 0))
    for D in TIE_D:                                   # ... and with K = 6 and K = 32 (K == D at D = 32 leaves nothing to straddle: all_equal)
        for K in (6, 32):
            for p in PATTERNS[:3]:
                if K + 3 <= D or p == "all_equal":
                    out.append((p, D, K, "signed", 0))
    out.append(("all_equal", 24, 24, "asym", 0))      # K == D on the LDS kernel, and the asymmetric range on a tie
    out.append(("cross_wave", 96, 24, "asym", 0))
    return out


def tie_case(pattern, D, K, shift=0):
    """-> (logits, strength, expected planes (list, ascending), levels, info)."""
    levels, info = levels_of(pattern, D, K, shift)
    logits, strength = tie_inputs(levels, 2000 + 7 * D + K + 100 * PATTERNS.index(pattern) + shift)
    zero = ZERO_BELOW if pattern in ("underflow", "subnormal") else None
    return logits, strength, expected_planes(levels, K, zero), levels, info


def flushed_planes(levels, K):
    """`subnormal` if an evaluation flushed subnormal probabilities to zero: every plane more than 87 below the maximum (below the
    smallest NORMAL fp32, exp(-87.3)) joins one tie group, and the lower index wins."""
    return expected_planes(levels, K, zero_below=87.0)


#: the remaining (D, K, range) on random logits: the LDS kernel below 64 KiB (24), at 126 and 128, K == D, every K, every range
RANDOM_CASES = (
    (24, 6, "signed"), (24, 24, "signed"), (24, 24, "unsigned"), (24, 6, "asym"),
    (32, 32, "signed"), (32, 24, "unsigned"), (32, 6, "asym"),
    (64, 24, "unsigned"), (64, 32, "asym"),
    (66, 24, "signed"), (66, 32, "unsigned"), (66, 6, "asym"),
    (96, 24, "unsigned"), (96, 6, "signed"), (96, 32, "asym"),
    (126, 24, "signed"), (126, 32, "unsigned"), (126, 6, "asym"),
    (128, 24, "signed"), (128, 24, "unsigned"), (128, 32, "asym"), (128, 6, "unsigned"),
)


def random_case(D, K, rname):
    salt = 3000 + 10 * D + K + {"signed": 0, "unsigned": 1, "asym": 2}[rname]
    return random_inputs(D, salt)


# ---- soft-argmax, forward ------------------------------------------------------------------------------------------------------------

SOFTARG_D = (2, 24, 64, 66, 96, 126, 128)
#: plane counts the fused kernels decline: past the limit, and odd (no exact 2x along D)
SOFTARG_DECLINED = (130, 25)


def softarg_logits(D):
    """[B,D,H,W] logits of ss_softmax_regression_fwd."""
    return dd.t_normalish((B, D, H, W), 4000 + D) * 2.0


def softarg_coarse(D):
    """[B,1,D/2,H,W] coarse logits of ss_upsample_softmax_regression_fwd: the map shape is the COARSE one, the fine map is 10 x 54
    (1080 pixels: 16 blocks of 64 + 56)."""
    return dd.t_normalish((B, 1, D // 2, H, W), 4200 + D) * 2.0


def softarg_ref(logits, rng):
    """float64 softmax over D, expectation and variance over the disparities of `rng` -> (prob, disp [B,H,W], var [B,1,H,W])."""
    p = torch.softmax(logits, dim=1)
    vals = torch.arange(rng[0], rng[0] + rng[1], dtype=p.dtype).reshape(1, -1, 1, 1)
    disp = (p * vals).sum(dim=1)
    return p, disp, (p * (vals - disp.unsqueeze(1)) ** 2).sum(dim=1, keepdim=True)


# ---- tail, backward ------------------------------------------------------------------------------------------------------------------

BWD_D = (32, 64, 96, 128)
BWD_K = (6, 24, 32)
BWD_RANGES = ("signed", "unsigned")


def topk_bwd_grads(D, K):
    """Incoming gradients of (att_topk, pred_att)."""
    return dd.t_normalish((B, 1, K, H, W), 5000 + D + K), dd.t_normalish((B, H, W), 5001 + D + K)


def upsoft_bwd_case(D):
    """-> (coarse [B,1,D/2,H,W], fine H, fine W, (grad_up, grad_disp, grad_var))."""
    coarse = dd.t_normalish((B, 1, D // 2, H, W), 5200 + D) * 2.0
    fh, fw = 2 * H, 2 * W
    grads = (dd.t_normalish((B, 1, D, fh, fw), 5201 + D), dd.t_normalish((B, fh, fw), 5202 + D), dd.t_normalish((B, 1, fh, fw), 5203 + D))
    return coarse, fh, fw, grads


#: the probe on the unsigned span: D = 32 on W = 27 columns
STRENGTH_UNSIGNED = {"shape": (B, 12, H, W), "D": 32, "salt": 5400}


def strength_unsigned_case():
    """-> ([left, right, pred0, var, gamma, beta], grad_strength, tap properties): pred0 = round(uniform(0, D - 1)) + frac, frac in
    [0.2, 0.8] (clear of the integers, where the bilinear derivative jumps) -- every pred0 >= 0, as the unsigned model's soft-argmax."""
    (b, C, h, w), D, salt = STRENGTH_UNSIGNED["shape"], STRENGTH_UNSIGNED["D"], STRENGTH_UNSIGNED["salt"]
    left, right = dd.stereo_features(b, C, h, w, salt, max_shift=3)
    pred0 = torch.round(dd.t_uniform((b, h, w), salt + 1, 0.0, D - 1.0)) + dd.t_uniform((b, h, w), salt + 2, 0.2, 0.8)
    var = dd.t_uniform((b, 1, h, w), salt + 4, 0.0, 20.0)
    go = dd.t_normalish((b, 5, h, w), salt + 5)
    return [left, right, pred0, var, torch.tensor([0.25]), torch.tensor([2.0])], go, BP.tap_properties(pred0)


# ---- sparse concat volume, backward, one-sided candidates ------------------------------------------------------------------------------

CONCAT_SHAPE = (1, 8, 3, 192, 24)            # (B, C, H, W, nd)
CONCAT_MARGINS = (32, 64, 128)
#: ss_concat_sampled_bwd caps the margin its LDS windows cover (warp.hip)
CONCAT_MARGIN_CAP = 96


def concat_case(m):
    """-> (left, right, candidates [B,nd,H,W] distinct ascending integers in [0, m), att, incoming gradient): the candidates the unsigned
    model hands over at maxdisp / 4 = m, with margin = m."""
    b, C, h, w, nd = CONCAT_SHAPE
    salt = 5600 + m
    left, right = dd.t_normalish((b, C, h, w), salt), dd.t_normalish((b, C, h, w), salt + 1)
    d = dd.distinct_sorted_candidates(b, nd, h, w, m // 2, salt + 2) + float(m // 2)
    att = dd.t_uniform((b, 1, nd, h, w), salt + 3, 0.0, 1.0)
    seed = dd.t_normalish((b, 2 * C, nd, h, w), salt + 4)
    return left, right, d, att, seed


# ---- one training step of the unsigned segment -------------------------------------------------------------------------------------

SEGMENT_WHU_TRAIN = "whu_t128_md128"
#: the float64 oracle's own margin at the top-24 cut must stay this many times cases.DELTA24_REL, or the cap of two differing pixels
#: of the step test means nothing
SEGMENT_MIN_GAP_FACTOR = 5.0
