"""What the scene tests share (test infrastructure, like right_view_cases.py): seeded tiles of the two kinds, the sequential per-pixel
restatement of the blend in plain loops, and the checks with their bounds.

The two kinds of input:
  exact   tile values are integer-valued floats in [-64, 64], logits in [-8, 8], ramps at most 16: every w * v and every partial sum is
          an integer below 2^24 (9 tiles x 256 x 64 < 2^18), so num and den are exact in fp32 and ONE correctly rounded division
          follows (under ONE tile the value is the tile's own, which is what (w v) / w gives here) -- the kernel, the fp32 composition and a float64 evaluation rounded to fp32 agree bit for bit
  float   tiles N(0, 20^2), logits N(0, 3^2), compared with the float64 evaluation: BOUND_ULPS * 2^-24 * max|v|, from at most 18
          roundings (9 products, 9 sums), each at most 2^-24 relative to sum w|v| / sum w <= max|v|, doubled for contraction
          differences.  Not tuned.
Labels are compared where the float64 top-2 margin of the blended logits exceeds twice that bound; at most 0.1 % of the pixels may
be excluded."""
import numpy as np
import torch

BOUND_ULPS = 32.0
MAX_EXCLUDED = 1e-3


def bound(*tensors):
    return BOUND_ULPS * 2.0 ** -24 * max(float(t.abs().max()) for t in tensors)


def make_tiles(plan, C, kind, seed=0):
    """(disparity tiles [n,th,tw], logit tiles [n,C,th,tw] or None) on the CPU, float32."""
    g = torch.Generator().manual_seed(seed)
    n, (th, tw) = len(plan), plan.size
    if kind == "exact":
        d = torch.randint(-64, 65, (n, th, tw), generator=g).float()
        lg = torch.randint(-8, 9, (n, C, th, tw), generator=g).float() if C else None
    else:
        d = torch.randn((n, th, tw), generator=g) * 20.0
        lg = torch.randn((n, C, th, tw), generator=g) * 3.0 if C else None
    return d, lg


def restate(plan, disp, logit=None, dtype=np.float32, rows=None, resident=None):
    """The blend pixel by pixel, tile by tile in ascending (ty, tx), every operation rounded to `dtype`.  Returns numpy arrays:
    disparity, spread [H,W] and logits [C,H,W] in `dtype`, label and count uint8; rows outside `rows` stay 0."""
    H, W, (th, tw), (ry, rx) = plan.height, plan.width, plan.size, plan.ramp
    f = dtype
    d = disp.numpy().astype(f)
    lg = None if logit is None else logit.numpy().astype(f)
    C = 0 if lg is None else lg.shape[1]
    y0, y1 = (0, H) if rows is None else rows
    out = {"disparity": np.zeros((H, W), f), "spread": np.zeros((H, W), f), "count": np.zeros((H, W), np.uint8)}
    if C:
        out["logits"], out["label"] = np.zeros((C, H, W), f), np.zeros((H, W), np.uint8)
    for y in range(y0, y1):
        for x in range(W):
            num, den, hi, lo, cnt, one, onel = f(0), f(0), f(-np.inf), f(np.inf), 0, f(np.nan), []
            nl = [f(0)] * C
            for ty, oy in enumerate(plan.origin_y):
                for tx, ox in enumerate(plan.origin_x):
                    i = ty * plan.ntx + tx
                    iy, ix = y - oy, x - ox
                    if not (0 <= iy < th and 0 <= ix < tw) or (resident is not None and not resident[i]):
                        continue
                    w = f(f(min(iy + 1, th - iy, ry)) * f(min(ix + 1, tw - ix, rx)))
                    v = d[i, iy, ix]
                    num, den = f(num + f(w * v)), f(den + w)
                    hi, lo, cnt = max(hi, v), min(lo, v), cnt + 1
                    one, onel = v, [lg[i, c, iy, ix] for c in range(C)]         # under ONE tile the value is the tile's own
                    for c in range(C):
                        nl[c] = f(nl[c] + f(w * lg[i, c, iy, ix]))
            out["disparity"][y, x], out["spread"][y, x], out["count"][y, x] = (one if cnt == 1 else f(num / den)), f(hi - lo), cnt
            if C:
                z = onel if cnt == 1 else [f(v / den) for v in nl]
                out["logits"][:, y, x] = z
                out["label"][y, x] = int(np.argmax(np.array(z)))
    return out


def as_f32(out64):
    """A float64 evaluation rounded to fp32 (integer maps unchanged)."""
    return {k: torch.from_numpy(v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in out64.items()}


def check_exact(got, want, what, rows=None):
    """torch.equal on every output of `want` that `got` has (tensors or numpy arrays), on `rows` only where given."""
    for k, w in want.items():
        if k not in got:
            continue
        g = got[k].cpu() if isinstance(got[k], torch.Tensor) else torch.from_numpy(got[k])
        w = w.cpu() if isinstance(w, torch.Tensor) else torch.from_numpy(w)
        if rows is not None:
            g, w = g[..., rows[0]:rows[1], :], w[..., rows[0]:rows[1], :]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype, g.shape, w.shape)
        assert torch.equal(g, w), f"{what} {k}: {(g != w).sum().item()} of {w.numel()} values differ"


def check_float(got, ref64, tiles, what):
    """`got` (fp32) against the float64 evaluation `ref64` (tensors): the bound on disparity, logits and spread, count equal, and the
    label rule.  `tiles`: (disparity tiles, logit tiles) for max|v|.  Prints each figure before it asserts."""
    bd = bound(tiles[0])
    for k, b in (("disparity", bd), ("spread", bd)) + ((("logits", bound(tiles[1])),) if "logits" in ref64 else ()):
        if k in got:
            err = float((got[k].cpu().double() - ref64[k].double()).abs().max())
            print(f"{what} {k}: max error {err:.3e}, bound {b:.3e}")
            assert err <= b, (what, k, err, b)
    if "count" in got:
        assert torch.equal(got["count"].cpu(), ref64["count"]), (what, "count")
    if "label" in got:
        z = ref64["logits"].double()
        top = z.topk(2, dim=0).values
        sure = (top[0] - top[1]) > 2 * bound(tiles[1])
        excluded = 1.0 - float(sure.double().mean())
        wrong = int(((got["label"].cpu() != ref64["label"]) & sure).sum())
        print(f"{what} label: {excluded:.5f} of the pixels excluded, {wrong} of the others differ")
        assert excluded <= MAX_EXCLUDED and wrong == 0, (what, excluded, wrong)
