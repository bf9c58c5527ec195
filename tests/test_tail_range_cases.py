"""CPU: every input of tests/tail_range_cases.py has the property it is named for -- the plane count takes the kernel it claims, the tie
groups sit in the quarters and straddle the cut they claim, the fp32 and float64 oracle compositions select what the integer rule says,
the one-sided candidates pass the margin cap, and the unsigned training case keeps its distance from a top-24 tie."""
import pytest
import torch

import tail_range_cases as TR
import train_calls as TC
from golden import cases
from oracle import hot_segment as oseg
from oracle import stack as ostack

TINY = float(torch.finfo(torch.float32).tiny)


# ---- dispatch ---------------------------------------------------------------------------------------------------------------------------

def test_plane_counts_take_the_kernels_they_are_named_for():
    """ss_topk_candidates_fwd: 32, 64, 96 on topk_candidates_split, every other D <= 128 on the one-thread-per-pixel kernel with
    2 D 128 4 bytes of LDS -- through ensure_dynamic_lds from D = 65 (66 is the first even D past 64 KiB), 128 KiB at the limit."""
    for D in (32, 64, 96):
        assert TR.topk_kernel(D) == (f"split<{D}>", 0, False)
    assert TR.topk_kernel(24) == ("lds", 24 * 1024, False)
    assert TR.topk_kernel(64 + 2) == ("lds", 66 * 1024, True) and TR.topk_kernel(65)[2] and not TR.topk_kernel(63)[2]
    assert TR.topk_kernel(126) == ("lds", 126 * 1024, True)
    assert TR.topk_kernel(128) == ("lds", 128 * 1024, True) and TR.topk_kernel(130)[0] is None
    used = {d for (_p, d, _k, _r, _s) in TR.tie_cases()} | {d for (d, _k, _r) in TR.RANDOM_CASES}
    assert used == {24, 32, 64, 66, 96, 126, 128}
    assert {TR.topk_kernel(d)[0] for d in used} == {"lds", "split<32>", "split<64>", "split<96>"}


def test_softargmax_plane_counts_leave_partial_chunks_and_idle_waves():
    """softmax_regress_split<1> up to D = 64, <2> up to 128: 66 and 126 leave a partial last 16-plane chunk, 66 three waves of the second
    round without a plane; 2 and 24 the same in the one-round kernel; 128 fills every chunk."""
    assert TR.softarg_kernel(2) == (1, 1, 2, [(0, 1), (0, 2), (0, 3)])
    assert TR.softarg_kernel(24) == (1, 2, 8, [(0, 2), (0, 3)])
    assert TR.softarg_kernel(64) == (1, 4, 16, [])
    assert TR.softarg_kernel(66) == (2, 5, 2, [(1, 1), (1, 2), (1, 3)])
    assert TR.softarg_kernel(96) == (2, 6, 16, [(1, 2), (1, 3)])
    assert TR.softarg_kernel(126) == (2, 8, 14, [])
    assert TR.softarg_kernel(128) == (2, 8, 16, [])
    assert TR.softarg_kernel(130)[0] is None
    assert set(TR.SOFTARG_D) == {2, 24, 64, 66, 96, 126, 128}


def test_the_map_leaves_partial_blocks_and_has_every_border_tap():
    n = TR.B * TR.H * TR.W
    assert n == 270 and n % 64 == 14 and n % 128 == 14 and n > 128
    assert (2 * TR.H) * (2 * TR.W) * TR.B % 64 != 0
    assert TR.H >= 3 and TR.W >= 3                      # interior pixels and all four borders


def test_ranges():
    assert TR.ranges(64) == {"signed": (-32, 64), "unsigned": (0, 64), "asym": (-8, 64)}


# ---- tie patterns ------------------------------------------------------------------------------------------------------------------------

TIE_SET = sorted(set((p, d, k, s) for (p, d, k, _r, s) in TR.tie_cases()))


def test_tie_cases_cover_what_the_selection_tests_claim():
    got = TR.tie_cases()
    for D in (32, 64, 96, 66, 128):
        for p in TR.PATTERNS:
            assert (p, D, 24, "signed", 0) in got
        for p in TR.PATTERNS[:3]:
            assert (p, D, 24, "unsigned", 0) in got
            for K in (6, 32):
                assert (p, D, K, "signed", 0) in got or (K == D and p != "all_equal")
    assert ("all_equal", 32, 32, "signed", 0) in got and ("all_equal", 24, 24, "asym", 0) in got      # K == D on either kind of kernel
    assert all(k <= d and k in (6, 24, 32) for (_p, d, k, _r, _s) in got)
    assert all(k <= d and k in (6, 24, 32) and r in ("signed", "unsigned", "asym") for (d, k, r) in TR.RANDOM_CASES)
    assert {d for (d, _k, _r) in TR.RANDOM_CASES} >= {24, 126} and (24, 24, "signed") in TR.RANDOM_CASES


@pytest.mark.parametrize("case", TIE_SET, ids=lambda c: "-".join(map(str, c)))
def test_tie_pattern_properties_and_oracle_compositions(case):
    """The stated property of each pattern, from the levels; then the oracle composition (propagation_prob x strength, softmax, stable
    sort) in fp32 AND in float64 selects exactly the planes of the integer rule -- `underflow` in fp32 only, that being its point."""
    pattern, D, K, shift = case
    logits, strength, want, levels, info = TR.tie_case(pattern, D, K, shift)
    assert logits.shape == (TR.B, 1, D, TR.H, TR.W) and logits.dtype == torch.float32 and len(want) == K == len(set(want))
    distinct = sorted(set(levels))
    assert all(b - a >= 0.5 for a, b in zip(distinct, distinct[1:]))
    for d in range(D):                                   # planes of one level are bitwise identical as whole planes
        first = levels.index(levels[d])
        assert torch.equal(logits[:, :, d], logits[:, :, first])
    zero = TR.ZERO_BELOW if pattern in ("underflow", "subnormal") else None
    groups = TR.tie_groups(levels, K, zero)
    last_level, last, above = groups[-1]                 # the group the cut falls into (or ends on)
    quarters = lambda members: {TR.quarter(d, D) for d in members}      # noqa: E731
    if pattern == "all_equal":
        assert len(groups) == 1 and len(last) == D and want == list(range(K))
    elif pattern == "cross_wave":
        assert last == info["group"] and len(last) >= 6 and quarters(last) == {0, 1, 2, 3}
        assert above == len(info["above"]) < K < above + len(last)
        others = [levels[d] for d in range(D) if d not in last and d not in info["above"]]
        assert len(set(others)) == len(others) and max(others) < last_level
        assert len(set(levels[d] for d in info["above"])) == above
        assert want == sorted(info["above"] + last[:K - above])
    elif pattern == "whole_then_partial":
        (lw, whole, aw), (lp, part, ap) = groups[-2], groups[-1]
        assert whole == info["whole"] and part == info["partial"] and lw > lp
        assert len(quarters(whole)) >= 3 and len(quarters(part)) >= 3
        assert aw + len(whole) == ap < K < ap + len(part)                     # the first whole, the second straddling the cut
        assert set(whole) <= set(want) and 0 < len(set(part) & set(want)) < len(part)
        assert sorted(set(part) & set(want)) == part[:K - ap]
    elif pattern == "pairs":
        assert levels == [float((d // 2 + shift) % 7) for d in range(D)]
        assert all(levels[2 * i] == levels[2 * i + 1] for i in range(D // 2))
        if (D, K, shift) == (64, 24, 0):
            assert above + len(last) == K                 # three whole groups of eight: the cut ON a group boundary
        else:
            assert above < K < above + len(last)          # the cut inside a group, hence inside one of its pairs or between two
        assert len(groups) >= 2
    elif pattern == "underflow":
        top = max(levels)
        near = [d for d in range(D) if levels[d] >= top - 20.0]
        rest = [d for d in range(D) if d not in near]
        assert near == info["near"] and len(near) < K
        assert all(levels[d] <= top - TR.ZERO_BELOW for d in rest) and len({levels[d] for d in rest}) >= 3
        assert last == rest and above == len(near) < K < above + len(rest)
        assert want != TR.expected_planes(levels, K)     # float64 (no underflow) would order them by level
    elif pattern == "subnormal":
        top = max(levels)
        sub = info["sub"]
        assert len(sub) == 7 and sorted(top - levels[d] for d in sub) == [90.0, 92.0, 94.0, 96.0, 98.0, 100.0, 102.0]
        assert len(info["near"]) == K - 4 and sum(1 for d in sub if d in want) == 4 and set(info["near"]) <= set(want)
        assert want == TR.expected_planes(levels, K)     # every level distinct at the cut: the plain rule
        assert want != TR.flushed_planes(levels, K)      # ... and an evaluation that flushes subnormals would be seen
    picks32, prob32 = TR.oracle_picks(logits, strength, K, torch.float32)
    picks64, prob64 = TR.oracle_picks(logits, strength, K, torch.float64)
    assert torch.equal(picks32, TR.planes_tensor(want)), "the fp32 oracle composition differs from the integer rule"
    if pattern == "underflow":
        assert bool((prob32[:, last] == 0).all()) and bool((prob64[:, last] > 0).all())
        assert torch.equal(picks64, TR.planes_tensor(TR.expected_planes(levels, K)))
    else:
        assert torch.equal(picks64, TR.planes_tensor(want)), "the float64 oracle composition differs from the integer rule"
    if pattern == "subnormal":
        p = prob32[:, info["sub"]]
        assert bool(((p > 0) & (p < TINY)).all()), "the seven planes at the cut are not subnormal in fp32 on the CPU"
        assert bool((p[:, 1:] > p[:, :-1]).all()), "... or not distinct"
    for d in range(D):                                   # equal planes -> bitwise equal probabilities
        first = levels.index(levels[d])
        assert torch.equal(prob32[:, d], prob32[:, first])


def test_random_cases_are_far_from_exact_ties():
    """The random logits decide their picks by value: no two probabilities of a pixel are equal in float64."""
    for D, K, rname in TR.RANDOM_CASES:
        logits, strength = TR.random_case(D, K, rname)
        assert logits.shape == (TR.B, 1, D, TR.H, TR.W)
        _, prob = TR.oracle_picks(logits, strength, K, torch.float64)
        srt = prob.sort(dim=1).values
        assert bool((srt[:, 1:] > srt[:, :-1]).all()), (D, K, rname)


# ---- soft-argmax ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", TR.SOFTARG_D)
def test_softargmax_inputs_and_references(D):
    logits, coarse = TR.softarg_logits(D), TR.softarg_coarse(D)
    assert logits.shape == (TR.B, D, TR.H, TR.W) and coarse.shape == (TR.B, 1, D // 2, TR.H, TR.W)
    for rng in TR.ranges(D).values():
        p, disp, var = TR.softarg_ref(logits.double(), rng)
        assert float((p.sum(dim=1) - 1).abs().max()) < 1e-12
        assert float(disp.min()) >= rng[0] and float(disp.max()) <= rng[0] + rng[1] - 1 and float(var.min()) >= 0
        up, disp_u, var_u = TC.upsoft_ref(coarse.double(), 2 * TR.H, 2 * TR.W, rng)
        assert up.shape == (TR.B, 1, D, 2 * TR.H, 2 * TR.W)
        _, d2, v2 = TR.softarg_ref(up.squeeze(1), rng)    # the two references agree with each other
        assert float((d2 - disp_u).abs().max()) < 1e-10 and float((v2 - var_u).abs().max()) < 1e-8


# ---- backward cases --------------------------------------------------------------------------------------------------------------------

def test_backward_axes():
    assert TR.BWD_D == (32, 64, 96, 128) and TR.BWD_K == (6, 24, 32) and TR.BWD_RANGES == ("signed", "unsigned")
    for D in TR.BWD_D:
        coarse, fh, fw, grads = TR.upsoft_bwd_case(D)
        assert coarse.shape == (TR.B, 1, D // 2, TR.H, TR.W) and (fh, fw) == (2 * TR.H, 2 * TR.W)
        assert grads[0].shape == (TR.B, 1, D, fh, fw) and grads[1].shape == (TR.B, fh, fw) and grads[2].shape == (TR.B, 1, fh, fw)
        assert D * 64 * 4 <= 64 * 1024                    # ss_topk_candidates_bwd: D x 64 floats of LDS


def test_strength_case_on_the_unsigned_span():
    """pred0 over [0, D) with D = 32 on 27 columns: every candidate is >= 0, so a tap can leave the image on the LEFT only (column
    w - d <= w) -- partly (the west tap at column -1 beside a live east tap) and wholly; the bilinear derivative's jumps are kept clear."""
    ins, go, p = TR.strength_unsigned_case()
    b, C, h, w = TR.STRENGTH_UNSIGNED["shape"]
    assert (h, w) == (TR.H, TR.W) and TR.STRENGTH_UNSIGNED["D"] == 32
    pred0 = ins[2]
    assert pred0.shape == (b, h, w) and float(pred0.min()) >= 0.2 and float(pred0.max()) <= 31.8 and float(pred0.max()) > w
    assert p["min_frac"] >= 0.1 and p["leave_image"] > 0 and p["col_minus1"] > 0 and p["col_W"] == 0
    assert p["row_same"] > 0 and set(p["row_kinds"]) == {0}
    out = TC.strength_ref(*[t.double() for t in ins])
    assert bool(torch.isfinite(out).all()) and go.shape == out.shape


@pytest.mark.parametrize("m", TR.CONCAT_MARGINS)
def test_concat_candidates_are_one_sided(m):
    left, right, d, att, seed = TR.concat_case(m)
    b, C, h, w, nd = TR.CONCAT_SHAPE
    assert d.shape == (b, nd, h, w) and w % 64 == 0 and seed.shape == (b, 2 * C, nd, h, w)
    assert float(d.min()) >= 0 and float(d.max()) < m and torch.equal(d, d.round())
    assert bool((d[:, 1:] > d[:, :-1]).all())                                 # distinct, ascending
    beyond = d > TR.CONCAT_MARGIN_CAP
    if m == 128:                                          # candidates 97 ... 127 lie past the capped windows, in every image row
        assert bool(beyond.any(dim=3).any(dim=1).all()) and float(d.max()) == 127.0
        assert int(beyond.sum()) > 100
    else:
        assert not bool(beyond.any()) and m <= TR.CONCAT_MARGIN_CAP


# ---- the unsigned training step -----------------------------------------------------------------------------------------------------

def test_unsigned_training_case_keeps_its_distance_from_a_top24_tie():
    """The float64 oracle in training mode on the committed inputs: the smallest relative gap between the 24th and 25th probabilities
    is at least SEGMENT_MIN_GAP_FACTOR x DELTA24_REL, so that 'at most two pixels with other candidates, each within DELTA24_REL' is a
    criterion the oracle itself does not exhaust."""
    name = TR.SEGMENT_WHU_TRAIN
    assert cases.SEGMENT_TRAIN[name] == (1, 128, 128, 128) and cases._SEGMENT_SEED[name] == 908
    fl4, fr4, fl8, fr8, maxdisp = cases.segment_inputs(name)
    assert fl4.shape == (1, 128, 32, 32) and fl8.shape == (1, 256, 16, 16) and maxdisp == 128
    P64 = {k: v.double() for k, v in oseg.deterministic_params().items()}
    keep = {}
    with ostack.training_mode(), torch.no_grad():
        _, smp, _ = oseg.attention_branch(P64, fl8.double(), fr8.double(), fl4.double(), fr4.double(), maxdisp, keep, unsigned=True)
    assert float(smp.min()) >= 0 and float(smp.max()) <= maxdisp // 4 - 1
    assert float(keep["gap24_rel"].min()) >= TR.SEGMENT_MIN_GAP_FACTOR * cases.DELTA24_REL, float(keep["gap24_rel"].min())
