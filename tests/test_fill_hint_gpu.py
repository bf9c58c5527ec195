"""The "chip is shared" hint (ss_set_fill_hint; PairPipeline sets it to its lane count for the duration of a call).

The hint scales the workgroup counts of the conv launchers' FILL heuristics only -- which output tile a stride-1 3x3x3 layer gets
(4 rows / 2 rows / 1 row per wave), which form a stride-2 layer -- so a launch that is one of several in flight gets the larger tile.
What is checked here, through the C ABI on the default (two-term fp16) engine:

  * bit identity across the hint (torch.equal on seeded inputs): hints 1, 8 and 64 (the clamp) on every case, and every form the
    tuning switches can force (SS_CONV_TILE 0 / 1 / 2; SS_CONV_S2_MT1 0 / 1).  Kernels are not inspected: that two hints select
    different kernels is asserted as "the result under hint h IS the result of the tile the rule picks for h, forced", with the
    rule restated below, and the picked tiles differ.  At these (small, quick) shapes the counts are 4 .. 32 workgroups, so 8 pairs
    in flight do not reach the 512 (stride 2: 256) workgroups of the next form and 64 do: hint 8 must equal hint 1 trivially, hint
    64 moves tile 2 -> tile 0 (4 x 4 and 2 x 8 forms), tile 2 -> tile 1, and the one-tile-per-wave stride-2 form -> the form whose
    waves split the 64 channels.  The 4-row forms reached this way are the chunk-blocked (two-pass) instantiations.
  * every case against a float64 CPU convolution with the bound of the existing conv tests for this engine
    (tests/test_parity_gpu.py: 1.5 x the error of the exact-fp32 MFMA kernel + 1e-7, stride 2: + 1e-6).
  * PairPipeline(seg, 3) on the 128 x 128 fixture: three different inputs, exactly what the one-stream segment returns, and the hint
    is back to 1 afterwards.
  * hint scoping (no GPU: a stub segment, stub streams): the hint is the lane count inside a pipelined call and 1 after it, also when
    the call raises; one lane leaves it alone.
"""
import contextlib
import os

import pytest
import torch

# (Cin, Cout, (D, H, W), stride)
CASES = {
    "s1_c64_4x16x64": (64, 64, (4, 16, 64), 1),         # tile 2 -> tile 0, the 4 x 4 x 32 form (depth a multiple of 4)
    "s1_c64_6x16x40": (64, 64, (6, 16, 40), 1),         # ... the 2 x 8 x 32 form, ragged W
    "s1_c128_2x8x32": (128, 128, (2, 8, 32), 1),        # tile 2 -> tile 1
    "s2_c32to64_4x16x64": (32, 64, (4, 16, 64), 2),     # one 32-channel tile per workgroup -> the waves split 64 channels
}
HINTS = (1, 8, 64)


def _cdiv(a, b):
    return (a + b - 1) // b


def _rule(case, hint, batch=1):
    """The launchers' fill rule (ss::plan_conv3d of csrc/conv_plan.h; tests/test_conv_plan.py holds this restatement to it): stride 1 -> the tile
    candidate, stride 2 -> the form."""
    _cin, cout, (d, h, w), stride = case
    if stride == 1:
        blocks = lambda td, th: _cdiv(w, 32) * _cdiv(h, th) * _cdiv(d, td) * _cdiv(cout, 32) * batch      # noqa: E731
        return 0 if blocks(2, 8) * hint >= 512 else (1 if blocks(1, 8) * hint >= 512 else 2)
    do, ho, wo = (d - 1) // 2 + 1, (h - 1) // 2 + 1, (w - 1) // 2 + 1
    wg2 = _cdiv(wo, 32) * _cdiv(ho, 2) * _cdiv(do, 2) * _cdiv(cout, 64) * batch * hint
    return "split" if cout > 32 and wg2 >= 256 else "one_tile"


def _inputs(case, batch=1):
    from oracle import detdata as dd
    cin, cout, (d, h, w), _stride = case
    # (pair 0 of a batch is the batch-1 input: the second pair is drawn from another seed)
    x = torch.cat([dd.t_normalish((1, cin, d, h, w), 2301 + 10 * i) for i in range(batch)])
    wt = dd.t_uniform((cout, cin, 3, 3, 3), 2302, -1, 1) * (3.0 / (cin * 27)) ** 0.5
    scale, shift = dd.t_uniform((cout,), 2303, 0.5, 1.5), dd.t_uniform((cout,), 2304, -0.2, 0.2)
    return x, wt, scale, shift


@contextlib.contextmanager
def _hint(lib, value):
    prev = lib.ss_set_fill_hint(value)
    try:
        assert lib.ss_get_fill_hint() == value
        yield
    finally:
        lib.ss_set_fill_hint(prev)


@pytest.fixture(scope="module")
def sa():
    import semstereo_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    semstereo_amd._lib.load()
    return semstereo_amd


_REF = {}


def _reference(name):
    """float64 CPU convolution + affine + ReLU of a case (computed once, shared, never written to)."""
    if name not in _REF:
        import torch.nn.functional as F
        case = CASES[name]
        x, wt, scale, shift = _inputs(case)
        _REF[name] = F.relu(F.conv3d(x.double(), wt.double(), None, case[3], 1) * scale.double().reshape(1, -1, 1, 1, 1)
                            + shift.double().reshape(1, -1, 1, 1, 1))
    return _REF[name]


def _run(sa, case, x, wt, scale, shift):
    ws = sa.modules.pack_conv_weight_bf16s(wt.cuda(), 19)
    return sa.modules.conv3d_bf16s_hip(x.cuda(), ws, case[1], scale.cuda(), shift.cuda(), True, 19, stride=case[3])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_hint_changes_the_kernel_and_not_a_bit(sa, name, tuning_env):
    case = CASES[name]
    lib = sa._lib.load()
    assert os.environ.get("SS_FILL_HINT") is None and lib.ss_get_fill_hint() == 1
    x, wt, scale, shift = _inputs(case)
    by_hint = {}
    for h in HINTS:
        with _hint(lib, h):
            by_hint[h] = _run(sa, case, x, wt, scale, shift)
    assert lib.ss_get_fill_hint() == 1
    # the rule: 8 pairs in flight leave these small layers where they are, 64 move them
    assert _rule(case, 1) == _rule(case, 8) != _rule(case, 64)
    assert _rule(case, 64) == {"s1_c64_4x16x64": 0, "s1_c64_6x16x40": 0, "s1_c128_2x8x32": 1, "s2_c32to64_4x16x64": "split"}[name]
    forced = {}
    if case[3] == 1:
        for tile in (0, 1, 2):
            tuning_env("SS_CONV_TILE", str(tile))
            forced[tile] = _run(sa, case, x, wt, scale, shift)
        tuning_env("SS_CONV_TILE", "-1")
    else:
        # SS_CONV_S2_MT1=1: one channel tile per wave whatever the count; =0 under hint 64: two channel tiles per wave (the r02 form);
        # the form whose waves split the channels is reached by the count alone (hint 64, nothing forced)
        tuning_env("SS_CONV_S2_MT1", "1")
        with _hint(lib, 64):
            forced["one_tile"] = _run(sa, case, x, wt, scale, shift)
        tuning_env("SS_CONV_S2_MT1", "0")
        with _hint(lib, 64):
            forced["two_tiles"] = _run(sa, case, x, wt, scale, shift)
        tuning_env("SS_CONV_S2_MT1", "-1")
        forced["split"] = by_hint[64]
    for h in HINTS:
        assert torch.equal(by_hint[h], forced[_rule(case, h)]), (name, h, "differs from the form the rule picks, forced")
        assert torch.equal(by_hint[h], by_hint[1]), (name, h, float((by_hint[h] - by_hint[1]).abs().max()))
    for k, y in forced.items():
        assert torch.equal(y, by_hint[1]), (name, "forced", k, float((y - by_hint[1]).abs().max()))
    # ... and what all of them computed is the convolution: the bound of test_conv3d_split_bf16_engine / _stride2 for this engine
    ref = _reference(name)
    y32 = sa.modules.conv3d_hip(x.cuda(), sa.modules.pack_conv_weight(wt.cuda()), scale.cuda(), shift.cuda(), 3, case[3], True)
    e, e_f32 = float((by_hint[1].double().cpu() - ref).abs().max()), float((y32.double().cpu() - ref).abs().max())
    print(f"{name}: max err vs float64 {e:.3e} (exact-fp32 kernel {e_f32:.3e})")
    assert by_hint[1].shape == ref.shape
    assert e <= 1.5 * e_f32 + (1e-7 if case[3] == 1 else 1e-6), (e, e_f32)


@pytest.mark.gpu
def test_pair_zero_of_a_batch_gets_the_bits_of_the_pair_alone(sa):
    """Cin = Cout = 64 on [4,16,64], batch 1 vs batch 2 (and under every hint): pair 0 identical -- the summation order is the
    layer's, whatever tile the launch's batch or the pairs in flight select."""
    name = "s1_c64_4x16x64"
    case = CASES[name]
    lib = sa._lib.load()
    x2, wt, scale, shift = _inputs(case, batch=2)
    alone = _run(sa, case, x2[:1].contiguous(), wt, scale, shift)
    for h in HINTS:
        with _hint(lib, h):
            both = _run(sa, case, x2, wt, scale, shift)
        assert torch.equal(both[:1], alone), (h, float((both[:1] - alone).abs().max()))
    assert _rule(case, 1, batch=2) != _rule(case, 64, batch=2)


@pytest.mark.gpu
def test_pipeline_of_three_lanes_returns_what_one_stream_returns(sa):
    """PairPipeline(seg, 3) -- the hint is 3 inside its calls -- on the 128 x 128 fixture and two more inputs of its shape."""
    from golden import cases
    from oracle import detdata as dd
    from oracle import hot_segment as oseg
    lib = sa._lib.load()
    B, H, W, maxdisp = cases.SEGMENT["s128"]
    seg = sa.HotSegment(maxdisp)
    seg.load_state_dict(oseg.deterministic_params(), strict=False)
    seg = seg.cuda().eval()
    pairs = [[t.cuda() for t in cases.segment_inputs("s128")[:4]]]
    for i in (1, 2):
        fl8, fr8 = dd.stereo_features(B, 256, H // 8, W // 8, 2400 + 2 * i, max_shift=3)
        fl4, fr4 = dd.stereo_features(B, 128, H // 4, W // 4, 2401 + 2 * i, max_shift=6)
        pairs.append([t.cuda() for t in (fl4, fr4, fl8, fr8)])
    with torch.no_grad():
        want = [{k: v.clone() for k, v in seg(*p).items()} for p in pairs]
    torch.cuda.synchronize()
    assert lib.ss_get_fill_hint() == 1
    pipe = sa.PairPipeline(seg, 3)
    got = [pipe(*p) for p in pairs]
    assert lib.ss_get_fill_hint() == 1
    pipe.synchronize()
    for i, (g_, w_) in enumerate(zip(got, want)):
        for k in ("pred", "pred_att", "samples", "att_topk"):
            assert torch.equal(g_[k], w_[k]), (i, k, float((g_[k] - w_[k]).abs().max()))
    pipe.close()


# ---- scoping: no GPU ----

class _FakeStream:
    def wait_stream(self, other):
        pass

    def query(self):
        return True

    def synchronize(self):
        pass


class _FakeEvent:
    def record(self, stream):
        pass


class _FakeInput:
    device = "stub"


def _stub_pipeline(monkeypatch, lanes, seen, fail):
    from semstereo_amd import _lib
    from semstereo_amd import segment as S
    lib = _lib.load()

    class Seg:
        training = False

        def __call__(self, *inputs):
            seen.append(lib.ss_get_fill_hint())
            if fail:
                raise RuntimeError("the segment failed")
            return "out"
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: _FakeStream())
    monkeypatch.setattr(torch.cuda, "Event", _FakeEvent)
    pipe = S.PairPipeline(Seg(), lanes)
    pipe.lanes, pipe._primed = [_FakeStream() for _ in range(lanes)], True        # (priming is device work: allocator pools, weight packing)
    return lib, pipe


@pytest.mark.parametrize("lanes", [1, 3, 6])
def test_hint_is_the_lane_count_inside_a_pipelined_call_and_one_after_it(monkeypatch, lanes):
    monkeypatch.delenv("SS_FILL_HINT", raising=False)
    seen = []
    lib, pipe = _stub_pipeline(monkeypatch, lanes, seen, fail=False)
    lib.ss_reload_tuning()
    assert lib.ss_get_fill_hint() == 1
    assert pipe(_FakeInput()) == "out" and pipe(_FakeInput()) == "out"
    assert seen == [lanes, lanes]             # (one lane: left at 1)
    assert lib.ss_get_fill_hint() == 1
    pipe.lanes = None


def test_hint_is_restored_when_the_call_raises(monkeypatch):
    monkeypatch.delenv("SS_FILL_HINT", raising=False)
    seen = []
    lib, pipe = _stub_pipeline(monkeypatch, 4, seen, fail=True)
    lib.ss_reload_tuning()
    with pytest.raises(RuntimeError, match="the segment failed"):
        pipe(_FakeInput())
    assert seen == [4] and lib.ss_get_fill_hint() == 1
    pipe.lanes = None


def test_set_returns_the_previous_value_clamps_and_the_environment_overrides(monkeypatch):
    from semstereo_amd import _lib
    from semstereo_amd import segment as S
    lib = _lib.load()
    monkeypatch.delenv("SS_FILL_HINT", raising=False)
    lib.ss_reload_tuning()
    try:
        assert lib.ss_set_fill_hint(5) == 1 and lib.ss_get_fill_hint() == 5
        assert lib.ss_set_fill_hint(0) == 5 and lib.ss_get_fill_hint() == 1            # clamped to [1, 64]
        assert lib.ss_set_fill_hint(1000) == 1 and lib.ss_get_fill_hint() == 64
        assert lib.ss_set_fill_hint(1) == 64
        with S.fill_hint(None):
            assert lib.ss_get_fill_hint() == 1
        with S.fill_hint(3):
            assert lib.ss_get_fill_hint() == 3
            with S.fill_hint(7):                                                      # nested: each level puts back what it found
                assert lib.ss_get_fill_hint() == 7
            assert lib.ss_get_fill_hint() == 3
        assert lib.ss_get_fill_hint() == 1
        monkeypatch.setenv("SS_FILL_HINT", "1")                                       # A/B runs: the launches sized as if alone, whatever is set
        lib.ss_reload_tuning()
        with S.fill_hint(6):
            assert lib.ss_get_fill_hint() == 1
    finally:
        monkeypatch.delenv("SS_FILL_HINT", raising=False)
        lib.ss_reload_tuning()
        lib.ss_set_fill_hint(1)
