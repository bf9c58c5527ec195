"""The numpy model of the two-term fp16 protocol (tests/f16_model.py) against float64, on every range case: the model stays inside
the bound the GPU range tests use, and four deliberately wrong models leave it by at least 10x -- so the bound is one a kernel with
a stale exponent, a forgotten rescale or a dropped cross term cannot meet.  No GPU."""
import numpy as np
import pytest

import f16_model as fm

# (Cin, Cout, positions, chunk, tile): the 1x1 projection's chunk of 32 on 64-position tiles (ragged last tile, Cout no multiple
# of 32), and the 8-channel chunks of the other kernels (ragged last chunk)
SETUPS = {"c96to33_chunk32": (96, 33, 200, 32, 64), "c20to12_chunk8": (20, 12, 70, 8, 32)}
WRONG = {"no_rescale": dict(rescale=False), "hl_dropped": dict(drop="hl"), "lh_dropped": dict(drop="lh"),
         "rescale_off_by_one": dict(rescale_shift=1)}


def _inputs(name, setup):
    Cin, Cout, P, _chunk, _tile = SETUPS[setup]
    rng = np.random.default_rng(1234)
    in_mul, w_mul, batch = fm.case_multipliers(name, Cin, Cout)
    B = 3 if batch else 1
    x = np.maximum(rng.standard_normal((B, Cin, P)), 0.0) * in_mul[None, :, None]            # ReLU'd: exact zeros among them
    if batch:
        x = x * np.array(batch)[:, None, None]
    w = rng.uniform(-1, 1, (Cout, Cin)) * (3.0 / Cin) ** 0.5 * w_mul[:, None]
    scale = rng.uniform(0.6, 1.4, Cout)
    return x.astype(np.float32), w.astype(np.float32), scale.astype(np.float32)


_CACHE = {}


def _want_and_bound(name, setup, block=True):
    key = (name, setup, block)
    if key not in _CACHE:
        Cin, Cout, P, chunk, _tile = SETUPS[setup]
        x, w, scale = _inputs(name, setup)
        x64, w64, s64 = x.astype(np.float64), w.astype(np.float64), scale.astype(np.float64)
        want = np.einsum("oc,bcp->bop", w64, x64) * s64[None, :, None]
        S = np.einsum("oc,bcp->bop", np.abs(w64), np.abs(x64)) * s64[None, :, None]
        blk = fm.block_term(x, np.abs(w64), scale, chunk)[:, :, None] if block else 0.0
        _CACHE[key] = (want, fm.f16_bound(S, want, Cin, blk))
    return _CACHE[key]


def _share(name, setup, block=True, **switches):
    """largest |error| / bound of the (possibly wrong) model on a case"""
    _Cin, _Cout, _P, chunk, tile = SETUPS[setup]
    x, w, scale = _inputs(name, setup)
    got = fm.project(x, w, scale, chunk=chunk, tile=tile, **switches).astype(np.float64)
    want, bound = _want_and_bound(name, setup, block)
    assert np.isfinite(got).all(), (name, setup)
    return float((np.abs(got - want) / bound).max())


def test_constants_of_the_header():
    assert (fm.E_MIN, fm.E_ONE) == (16, 141)
    for m in (1e-30, 3e-7, 1.0, 1.5, 6.5e4, 1e30):
        e = fm.biased_exponent(m)
        assert 2.0 ** 14 <= float(np.float32(m)) * float(fm.scale_for(e)) < 2.0 ** 15
        assert float(fm.scale_for(e)) * float(fm.unscale_for(e)) == 1.0
    # E_MIN: the scale and its inverse stay normal fp32 numbers
    assert np.isfinite(fm.scale_for(fm.E_MIN)) and fm.unscale_for(fm.E_MIN) >= np.finfo(np.float32).tiny
    # the range table at n = 32 is the table the 3-D range test has always used
    in_mul, w_mul, _ = fm.case_multipliers("channels_1e-6_to_1e+6", 32, 32)
    assert in_mul[5] == 10.0 ** (-6 + 12 * 5 / 31) and w_mul[5] == 1.0
    in_mul, _, _ = fm.case_multipliers("one_huge_channel", 32, 32)
    assert in_mul[17] == 3e4 and (np.delete(in_mul, 17) == 1e-3).all()


@pytest.mark.parametrize("setup", sorted(SETUPS))
@pytest.mark.parametrize("name", sorted(fm.ALL_RANGE_CASES))
def test_model_stays_inside_the_bound(name, setup):
    share = _share(name, setup)
    print(f"model {setup} {name}: {share:.3f} of the bound")
    assert share <= 1.0, (name, setup, share)


@pytest.mark.parametrize("setup", sorted(SETUPS))
@pytest.mark.parametrize("wrong", sorted(WRONG))
def test_each_wrong_model_leaves_the_bound_tenfold(wrong, setup):
    shares = {name: _share(name, setup, **WRONG[wrong]) for name in sorted(fm.ALL_RANGE_CASES)}
    worst = max(shares, key=shares.get)
    print(f"wrong model {wrong} {setup}: {shares[worst]:.3g} x the bound on {worst}")
    assert shares[worst] >= 10.0, (wrong, setup, shares)


def test_block_term_is_needed_and_is_not_slack():
    """one_huge_channel on ReLU'd inputs: values 2^-25 of the chunk maximum lose their low term's bits; without BLOCK the (right)
    model is outside the bound, with it inside"""
    without = _share("one_huge_channel", "c96to33_chunk32", block=False)
    print(f"model without BLOCK on one_huge_channel: {without:.3g} x the bound")
    assert without > 1.0 and _share("one_huge_channel", "c96to33_chunk32") <= 1.0


def test_batch_elements_share_no_exponent_state():
    x, w, scale = _inputs("batch_1e+6_1e-6_1", "c96to33_chunk32")
    whole = fm.project(x, w, scale)
    for b in range(3):
        assert np.array_equal(whole[b:b + 1], fm.project(x[b:b + 1], w, scale))
