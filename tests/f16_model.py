"""The two-term fp16 block-floating protocol of semstereo_amd/csrc/split_f16.h, restated in numpy from the header's text, the
range cases every kernel on it is tested with, and the bound those tests share.  No GPU, no kernel code: tests/test_f16_model.py
holds the model to the bound (and four deliberately wrong models out of it), tests/test_f16_ranges_gpu.py the kernels.

The contraction modelled is a 1x1 projection, y[b, co, p] = scale[co] * sum_c x[b, c, p] w[co, c]: K = Cin, staged in chunks of
`chunk` channels, with one block exponent per tile of `tile` consecutive positions of one batch element.
"""
import numpy as np

# ---- constants and helpers of split_f16.h ----
E_MIN, E_ONE = 16, 141


def pow2_biased(e):
    """2^(e - 127) from its biased exponent, 0 < e < 255 (0 gives 0), as an fp32 number"""
    return np.array(np.uint32(e) << np.uint32(23), dtype=np.uint32).view(np.float32)[()]


def scale_for(e):
    """the power of two that brings a maximum of biased exponent e into [2^14, 2^15)"""
    return pow2_biased(127 + E_ONE - e)


def unscale_for(e):
    return pow2_biased(127 - E_ONE + e)


def biased_exponent(m):
    return int(np.float32(m).view(np.uint32) >> np.uint32(23)) & 0xff


def split2(x):
    """x (fp32) -> hi = fp16(x), lo = fp16(x - hi), both returned as fp32"""
    with np.errstate(over="ignore"):
        hi = x.astype(np.float16).astype(np.float32)
        lo = (x - hi).astype(np.float16).astype(np.float32)
    return hi, lo


def pack_weights(w):
    """[Cout, Cin] fp32 -> (hi, lo, u): the two terms of w / u[co], u[co] = unscale_for(exponent of max |w[co]|, floored at E_MIN)"""
    w = np.asarray(w, dtype=np.float32)
    u = np.array([unscale_for(max(biased_exponent(np.abs(row).max()), E_MIN)) for row in w], dtype=np.float32)
    hi, lo = split2(w / u[:, None])
    return hi, lo, u


def project(x, w, scale=None, chunk=32, tile=64, rescale=True, drop=None, rescale_shift=0):
    """The protocol on x [B, Cin, P] and w [Cout, Cin] (fp32) -> [B, Cout, P] fp32.  The switches make the WRONG models of
    tests/test_f16_model.py: rescale=False leaves the accumulators alone when the exponent grows, drop="hl" / "lh" leaves out
    x_hi * w_lo / x_lo * w_hi, rescale_shift=1 rescales by twice the right power of two."""
    x, w = np.asarray(x, dtype=np.float32), np.asarray(w, dtype=np.float32)
    B, Cin, P = x.shape
    Cout = w.shape[0]
    wh, wl, u = pack_weights(w)
    out = np.zeros((B, Cout, P), dtype=np.float32)
    for b in range(B):
        for p0 in range(0, P, tile):
            xt = x[b, :, p0:p0 + tile]
            acc = np.zeros((Cout, xt.shape[1]), dtype=np.float32)
            e_cur, e_run = E_ONE, E_MIN                                  # BlockExp::reset()
            for c0 in range(0, Cin, chunk):
                xc = xt[c0:c0 + chunk]
                a = np.abs(xc)
                m = np.max(np.where(np.isfinite(a), a, np.float32(0)), initial=np.float32(0))
                e_run = max(e_run, biased_exponent(m))                   # advance(): monotone
                if e_run != e_cur:
                    if rescale:
                        acc = acc * pow2_biased(max(127 + e_cur - e_run + rescale_shift, 0))
                    e_cur = e_run
                xh, xl = split2(xc * scale_for(e_cur))
                whc, wlc = wh[:, c0:c0 + chunk], wl[:, c0:c0 + chunk]
                if drop != "hl":
                    acc = acc + _dot(wlc, xh)
                if drop != "lh":
                    acc = acc + _dot(whc, xl)
                acc = acc + _dot(whc, xh)
            y = acc * unscale_for(e_cur) * u[:, None]
            if scale is not None:
                y = y * np.asarray(scale, dtype=np.float32)[:, None]
            out[b, :, p0:p0 + tile] = y
    return out


def _dot(a, b):
    """fp32 matrix product of fp16-valued operands: every product is exact in fp32, the sum is accumulated in fp32"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.matmul(a.astype(np.float32), b.astype(np.float32), dtype=np.float32)


# ---- the range cases ----
# name: (multiplier of input channel c of n, multiplier of the weights of output channel c of n).  n = 32 gives the table the 3-D
# range test has always used (10^(-6 + 12 c / 31), channel 17 of 32).
F16_RANGE_CASES = {
    "tensor_1e-6": (lambda c, n=32: 1e-6, lambda c, n=32: 1.0),
    "tensor_1e+6": (lambda c, n=32: 1e6, lambda c, n=32: 1.0),
    "tensor_1e-20_weights_1e+12": (lambda c, n=32: 1e-20, lambda c, n=32: 1e12),
    "channels_1e-6_to_1e+6": (lambda c, n=32: 10.0 ** (-6 + 12 * c / max(n - 1, 1)), lambda c, n=32: 1.0),
    "channels_1e+6_to_1e-6": (lambda c, n=32: 10.0 ** (6 - 12 * c / max(n - 1, 1)), lambda c, n=32: 1.0),
    "out_channels_1e-8_to_1e+8": (lambda c, n=32: 1.0, lambda c, n=32: 10.0 ** (-8 + 16 * c / max(n - 1, 1))),
    "one_huge_channel": (lambda c, n=32: 3e4 if c == (17 * n) // 32 else 1e-3, lambda c, n=32: 1.0),
    "tensor_1e-30": (lambda c, n=32: 1e-30, lambda c, n=32: 1.0),
}
# ... and two more for the tests that came later: values at the flush floor (E_MIN: 2^-111), and three batch elements 12 decades
# apart in one launch (batch multipliers; no exponent state may pass from one element to the next)
F16_RANGE_CASES_NEW = {
    "tensor_1e-36": (lambda c, n=32: 1e-36, lambda c, n=32: 1.0),
    "batch_1e+6_1e-6_1": (lambda c, n=32: 1.0, lambda c, n=32: 1.0),
}
ALL_RANGE_CASES = dict(F16_RANGE_CASES, **F16_RANGE_CASES_NEW)
CHANNEL_CASES = ("channels_1e-6_to_1e+6", "channels_1e+6_to_1e-6", "one_huge_channel")
RAMP_CASES = ("channels_1e-6_to_1e+6", "channels_1e+6_to_1e-6")
TENSOR_CASES = ("tensor_1e-6", "tensor_1e+6", "tensor_1e-30", "tensor_1e-36", "tensor_1e-20_weights_1e+12")
BATCH_MULS = {"batch_1e+6_1e-6_1": (1e6, 1e-6, 1.0)}


def case_multipliers(name, Cin, Cout):
    """-> (float64 [Cin], float64 [Cout], batch multipliers or None) of a range case at these channel counts"""
    in_mul, w_mul = ALL_RANGE_CASES[name]
    return (np.array([in_mul(c, Cin) for c in range(Cin)], dtype=np.float64),
            np.array([w_mul(c, Cout) for c in range(Cout)], dtype=np.float64), BATCH_MULS.get(name))


# ---- the bound ----
M_FLOOR = 2.0 ** -110


def prefix_max(x, chunk):
    """x [B, Cin, ...] -> M [B, nchunks]: the largest finite |x| of batch element b in channels 0 .. end of chunk k (the running
    exponent is monotone), floored at 2^-110 (E_MIN)"""
    x = np.asarray(x, dtype=np.float64)
    B, Cin = x.shape[:2]
    a = np.abs(x.reshape(B, Cin, -1))
    a = np.where(np.isfinite(a), a, 0.0).max(axis=2)                     # [B, Cin]
    nch = -(-Cin // chunk)
    m = np.array([[a[b, k * chunk:(k + 1) * chunk].max() for k in range(nch)] for b in range(B)])
    return np.maximum(np.maximum.accumulate(m, axis=1), M_FLOOR)


def block_term(x, wabs_taps, scale, chunk):
    """BLOCK = 2^-38 |scale| sum_k M_k sum_{c in chunk k} |w[co, c, taps]| -> [B, Cout].  wabs_taps [Cout, Cin]: |w| summed over
    the taps an output reads.  From the format: the chunk's maximum is scaled into [2^14, 2^15); an fp16 term below the normal
    range rounds with absolute error 2^-25 = 2^-39 of the maximum per element; twice that is allowed."""
    wabs_taps = np.asarray(wabs_taps, dtype=np.float64)
    Cout, Cin = wabs_taps.shape
    nch = -(-Cin // chunk)
    wk = np.stack([wabs_taps[:, k * chunk:(k + 1) * chunk].sum(axis=1) for k in range(nch)], axis=1)      # [Cout, nchunks]
    blk = 2.0 ** -38 * prefix_max(x, chunk) @ wk.T
    if scale is not None:
        blk = blk * np.abs(np.asarray(scale, dtype=np.float64))[None, :]
    return blk


def f16_bound(S, want, K, block=0.0):
    """|got - want| <= (2^-21 + 4 sqrt(K) 2^-24) S + 2^-22 |want| + BLOCK, S = sum |x| |w| |scale| (the `_bound` of
    tests/test_heads_gpu.py and tests/test_decoder_gpu.py, their 2^-22 |want| of the affine's roundings, and block_term)"""
    return (2.0 ** -21 + 4.0 * K ** 0.5 * 2.0 ** -24) * S + 2.0 ** -22 * np.abs(want) + block
