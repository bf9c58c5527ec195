"""A numpy restatement of stem_left_mfma (semstereo_amd/csrc/stem_left.hip), the broadcast half of concat_stem on two fp16 terms with Q
by shifts, held to the bound the GPU test (tests/test_stem_left_mfma_gpu.py) holds the kernel to, and two deliberately wrong models
shown outside it.  No GPU, no kernel code; the protocol's pieces (split2, scale_for, the range cases, f16_bound) are tests/f16_model.py's.

What the kernel does, restated here from its header comment:
  * a workgroup owns 4 x 32 output positions of one batch element; the `left` halo tile (6 x 34 positions x 32 channels) is scaled by
    ONE power of two -- scale_for(exponent of the tile's largest finite |left|, floored at E_MIN) -- and split into two fp16 terms;
  * the weights of one (tap, output channel) row are divided by u = unscale_for(exponent of the row's largest |w|) and split;
  * Q[tap, co, p'] = sum over two K-steps of 16 channels of (w_lo x_hi + w_hi x_lo + w_hi x_hi), fp32 accumulate, then times the
    tile's inverse scale, then times u: Q is an fp32 number (it is handed over in registers, NOT as fp16 terms under an exponent of
    its own, and att is an fp32 operand: the kernel has ONE block exponent, the left tile's, not three);
  * out[co, j, p] = the fp32 fma chain over (kh, kw) outer, kd inner of att[j + kd - 1, p + off] * Q[tap, co, p + off].

The bound: f16_bound(S, want, K = 864, BLOCK), S = sum |att| |left| |w| over the 27 taps x 32 channels an output reads, and
BLOCK = 2^-38 M sum_taps |att| sum_c |w|, M = the largest finite |left| of the output's halo tile (floored at 2^-110).  From the
format, as f16_model.block_term: the tile maximum is scaled into [2^14, 2^15), an fp16 term below the normal range (2^-14) rounds with
absolute error 2^-25 = 2^-39 M per element, and twice that is allowed.

The issue that asked for this test names "a Q exponent kept from the previous batch" as the first wrong model.  This kernel keeps Q in
fp32 and has no Q exponent; the same mistake on the exponent it does have is modelled instead -- the left tile's exponent kept from
the previous tile -- beside the dropped w_lo x_hi product."""
import numpy as np
import pytest

import f16_model as fm

TH, TW = 4, 32


def _halo(a, h0, w0):
    """a [..., H, W] -> its [h0 - 1, h0 + TH + 1) x [w0 - 1, w0 + TW + 1) window, zero outside the image"""
    H, W = a.shape[-2:]
    out = np.zeros(a.shape[:-2] + (TH + 2, TW + 2), dtype=a.dtype)
    ys, xs = range(max(h0 - 1, 0), min(h0 + TH + 1, H)), range(max(w0 - 1, 0), min(w0 + TW + 1, W))
    if len(ys) and len(xs):
        out[..., ys[0] - h0 + 1:ys[-1] - h0 + 2, xs[0] - w0 + 1:xs[-1] - w0 + 2] = a[..., ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
    return out


def pack_rows(w):
    """w [Cout, C, 27] fp32 -> (hi, lo [27, Cout, C], u [27, Cout]): one power of two per (tap, output channel) row"""
    wt = np.ascontiguousarray(np.transpose(np.asarray(w, dtype=np.float32), (2, 0, 1)))
    m = np.abs(wt).max(axis=2)
    u = np.array([[fm.unscale_for(max(fm.biased_exponent(v), fm.E_MIN)) for v in row] for row in m], dtype=np.float32)
    hi, lo = fm.split2(wt / u[:, :, None])
    return hi, lo, u


def tile_maxima(left):
    """[B, C, H, W] -> [B, H, W]: the largest finite |left| of the halo tile each output position is computed in, floored at 2^-110"""
    left = np.asarray(left, dtype=np.float64)
    B, _, H, W = left.shape
    a = np.abs(left)
    a = np.where(np.isfinite(a), a, 0.0).max(axis=1)
    m = np.zeros((B, H, W))
    for h0 in range(0, H, TH):
        for w0 in range(0, W, TW):
            m[:, h0:h0 + TH, w0:w0 + TW] = _halo(a, h0, w0).reshape(B, -1).max(axis=1)[:, None, None]
    return np.maximum(m, fm.M_FLOOR)


def stem_left_model(left, w, att, drop=None, stale_exponent=False):
    """left [B, 32, H, W], w [Cout, 32, 27], att [B, nd, H, W] (fp32) -> [B, Cout, nd, H, W] fp32 as the kernel computes it.  The wrong
    models: drop="lh" leaves out w_lo * x_hi; stale_exponent=True scales a tile by the PREVIOUS tile's exponent (launch order)."""
    left, w, att = (np.asarray(t, dtype=np.float32) for t in (left, w, att))
    B, C, H, W = left.shape
    Cout, nd = w.shape[0], att.shape[1]
    wh, wl, u = pack_rows(w)
    out = np.zeros((B, Cout, nd, H, W), dtype=np.float32)
    e_prev = None
    for b in range(B):
        for h0 in range(0, H, TH):
            for w0 in range(0, W, TW):
                lt, at = _halo(left[b], h0, w0), _halo(att[b], h0, w0)
                a = np.abs(lt)
                e = max(fm.biased_exponent(np.max(np.where(np.isfinite(a), a, np.float32(0)))), fm.E_MIN)
                e_use = e_prev if (stale_exponent and e_prev is not None) else e
                e_prev = e
                xh, xl = fm.split2((lt * fm.scale_for(e_use)).reshape(C, -1))
                q = np.zeros((27, Cout, xh.shape[1]), dtype=np.float32)
                for ks in range(2):
                    c = slice(16 * ks, 16 * ks + 16)
                    if drop != "lh":
                        q = q + fm._dot(wl[:, :, c], xh[c])
                    q = q + fm._dot(wh[:, :, c], xl[c])
                    q = q + fm._dot(wh[:, :, c], xh[c])
                q = ((q * fm.unscale_for(e_use)) * u[:, :, None]).reshape(27, Cout, TH + 2, TW + 2)
                ap = np.zeros((nd + 2, TH + 2, TW + 2), dtype=np.float32)          # planes -1 and nd are zero
                ap[1:-1] = at
                o = np.zeros((Cout, nd, TH, TW), dtype=np.float32)
                for s in range(9):
                    kh, kw = divmod(s, 3)
                    for kd in range(3):
                        qs = q[kd * 9 + s][:, None, kh:kh + TH, kw:kw + TW].astype(np.float64)
                        av = ap[kd:kd + nd, kh:kh + TH, kw:kw + TW][None].astype(np.float64)
                        o = (o.astype(np.float64) + av * qs).astype(np.float32)      # one fma: a single rounding
                hh, ww = min(TH, H - h0), min(TW, W - w0)
                out[b, :, :, h0:h0 + hh, w0:w0 + ww] = o[:, :, :hh, :ww]
    return out


def reference_and_bound(left, w, att):
    """float64: (want, bound) of the module docstring"""
    left, w, att = (np.asarray(t, dtype=np.float64) for t in (left, w, att))
    B, C, H, W = left.shape
    Cout, nd = w.shape[0], att.shape[1]
    lp = np.pad(left, ((0, 0), (0, 0), (1, 1), (1, 1)))
    ap = np.pad(att, ((0, 0), (1, 1), (1, 1), (1, 1)))
    want, S, A = (np.zeros((B, Cout, nd, H, W)) for _ in range(3))
    for kd in range(3):
        for kh in range(3):
            for kw in range(3):
                wt = w[:, :, kd * 9 + kh * 3 + kw]
                ls, as_ = lp[:, :, kh:kh + H, kw:kw + W], ap[:, kd:kd + nd, kh:kh + H, kw:kw + W]
                want += np.einsum("oc,bchw->bohw", wt, ls)[:, :, None] * as_[:, None]
                S += np.einsum("oc,bchw->bohw", np.abs(wt), np.abs(ls))[:, :, None] * np.abs(as_)[:, None]
                A += np.abs(wt).sum(axis=1)[None, :, None, None, None] * np.abs(as_)[:, None]
    block = 2.0 ** -38 * tile_maxima(left)[:, None, None] * A
    return want, fm.f16_bound(S, want, 864, block)


def softmax_tail(B, nd, H, W, rng, decades=12.0):
    """att whose candidates span `decades` decades at every position, in a different order per position"""
    ramp = 10.0 ** (-decades * np.arange(nd) / max(nd - 1, 1))
    att = np.empty((B, nd, H, W))
    for b in range(B):
        for h in range(H):
            for x in range(W):
                att[b, :, h, x] = np.roll(ramp, (3 * h + 5 * x + b) % nd) * rng.uniform(0.5, 1.0, nd)
    return att


def make_case(name, shape, seed):
    """-> (left, w, att) fp32 of a range case at `shape` = (B, 32, nd, H, W): f16_model's multipliers on the left channels and the weight
    rows (output channels), or one of the two att-side cases"""
    B, C, nd, H, W = shape
    rng = np.random.default_rng(seed)
    att_case = name in ("att_softmax_tail_12_decades", "att_batch_1_1e-6_1e-12")
    in_mul, w_mul, batch = (np.ones(C), np.ones(32), None) if att_case else fm.case_multipliers(name, C, 32)
    if batch or name == "att_batch_1_1e-6_1e-12":
        B = 3
    left = rng.standard_normal((B, C, H, W))
    if name == "one_huge_channel":
        left = np.maximum(left, 0.0)
    left = left * in_mul[None, :, None, None]
    if batch:
        left = left * np.asarray(batch)[:, None, None, None]
    w = rng.uniform(-1, 1, (32, C, 27)) * (3.0 / (2 * C * 27)) ** 0.5 * w_mul[:, None, None]
    att = softmax_tail(B, nd, H, W, rng) if name == "att_softmax_tail_12_decades" else rng.uniform(0.0, 1.0, (B, nd, H, W))
    if name == "att_batch_1_1e-6_1e-12":
        att = att * np.array([1.0, 1e-6, 1e-12])[:, None, None, None]
    return left.astype(np.float32), w.astype(np.float32), att.astype(np.float32)


CASES = sorted(fm.ALL_RANGE_CASES) + ["att_softmax_tail_12_decades", "att_batch_1_1e-6_1e-12"]
SHAPE = (1, 32, 6, 5, 33)            # 2 x 2 tiles, one row and one column past a tile


def _share(got, want, bound, wrong_model=False):
    assert np.isfinite(want).all()
    if wrong_model and not np.isfinite(got).all():
        return float("inf")                  # (a scale 40 binades off overflows fp16: as far outside the bound as it gets)
    assert np.isfinite(got).all()
    return float((np.abs(got.astype(np.float64) - want) / bound).max())


@pytest.mark.parametrize("name", CASES)
def test_model_is_inside_the_bound(name):
    left, w, att = make_case(name, SHAPE, 17)
    want, bound = reference_and_bound(left, w, att)
    share = _share(stem_left_model(left, w, att), want, bound)
    print(f"{name}: {share:.3f} of the bound")
    assert share <= 1.0, share


@pytest.mark.parametrize("name", CASES)
def test_dropping_the_lo_hi_product_is_outside_the_bound(name):
    left, w, att = make_case(name, SHAPE, 17)
    want, bound = reference_and_bound(left, w, att)
    share = _share(stem_left_model(left, w, att, drop="lh"), want, bound, wrong_model=True)
    assert share > 4.0, share


def test_a_stale_tile_exponent_is_outside_the_bound():
    """three batch elements 12 decades apart: the second element's tiles scaled by the first element's exponent lose everything"""
    left, w, att = make_case("batch_1e+6_1e-6_1", SHAPE, 17)
    want, bound = reference_and_bound(left, w, att)
    share = _share(stem_left_model(left, w, att, stale_exponent=True), want, bound, wrong_model=True)
    assert share > 100.0, share


def test_model_nd24_ragged_borders():
    """the model's own indexing at the reference's 24 candidates: a ragged tile in both directions"""
    left, w, att = make_case("channels_1e-6_to_1e+6", (1, 32, 24, 6, 35), 23)
    want, bound = reference_and_bound(left, w, att)
    assert _share(stem_left_model(left, w, att), want, bound) <= 1.0
