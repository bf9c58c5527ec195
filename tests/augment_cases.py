"""What the augmentation tests share: the cases (the smallest shapes at which the kernel of csrc/augment.hip can still go wrong) and a
sequential per-pixel restatement of semstereo_amd/augment.py's eight steps in Python ints and numpy float32 scalars -- written apart from
the PyTorch composition, which it checks.  A case's raw arrays, parameters and restated sample are built once and shared."""
import functools

import numpy as np
import torch

NINE = ("left", "right", "disparity", "disparity_4", "disparity_8", "disparity_16", "label", "label_2", "label_4")
WHU_SIX = ("left", "right", "disparity", "disparity_4", "disparity_8", "disparity_16")
FOUR = ("left", "right", "disparity", "label")
NONE = (-1, -1, -1, -1)
TIE_K = 100                # the contrast tie: half the pixels of luma TIE_K, half TIE_K + 1

#: name -> B, image, crop, origin [B], vflip, swap, occluder (cy, sy, cx, sx), factors [B][2] as (left, right), keys, label / disparity
#: dtypes, maxdisp
CASES = {
    # every level, an odd x0 (the 12-byte group is not dword-aligned), each flag combination
    "levels_odd_origin": dict(B=3, image=(40, 52), crop=(32, 48), origin=[(5, 3)] * 3, vflip=[0, 1, 1], swap=[0, 0, 1],
                              occluder=[NONE, (10, 6, 20, 9), (25, 9, 40, 13)],
                              brightness=[(0.7, 1.5), (1.9, 0.55), (1.0, 1.3)], gamma=[(0.85, 1.15), (1.2, 0.8), (1.0, 0.93)],
                              contrast=[(0.8, 1.2), (1.13, 0.9), (1.05, 1.0)], saturation=[(0.2, 1.4), (1.0, 0.66), (0.0, 1.21)],
                              keys=NINE, label=torch.uint8, disparity=torch.float32, maxdisp=12),
    # widths that 4 does not divide: ragged quads forward and reversed
    "ragged_i64": dict(B=2, image=(23, 41), crop=(21, 37), origin=[(1, 2)] * 2, vflip=[0, 0], swap=[1, 0], occluder=[NONE, NONE],
                       brightness=[(1.2, 0.8), (0.6, 1.7)], gamma=[(1.1, 0.9), (0.8, 1.2)], contrast=[(0.9, 1.1), (1.2, 0.8)],
                       saturation=[(1.3, 0.4), (0.7, 1.0)], keys=FOUR, label=torch.int64, disparity=torch.float32, maxdisp=10),
    "ragged_f32": dict(B=2, image=(23, 41), crop=(21, 37), origin=[(1, 2)] * 2, vflip=[1, 0], swap=[1, 0], occluder=[NONE, (4, 3, 35, 5)],
                       brightness=[(1.2, 0.8), (0.6, 1.7)], gamma=[(1.1, 0.9), (0.8, 1.2)], contrast=[(0.9, 1.1), (1.2, 0.8)],
                       saturation=[(1.3, 0.4), (0.7, 1.0)], keys=FOUR, label=torch.float32, disparity=torch.float32, maxdisp=10),
    # a rectangle clipped by the crop's corner; one that starts and ends inside a quad; one covering the whole crop
    "occluder_clip": dict(B=2, image=(64, 80), crop=(48, 64), origin=[(7, 9), (16, 16)], vflip=[0, 0], swap=[0, 0],
                          occluder=[(44, 9, 60, 11), (20, 5, 22, 1)],
                          brightness=[(1.0, 1.4), (1.0, 0.7)], gamma=[(1.0, 1.1), (1.0, 0.9)], contrast=[(1.0, 1.1), (1.0, 0.85)],
                          saturation=[(1.0, 0.5), (1.0, 1.3)], keys=("left", "right"), label=torch.uint8, disparity=torch.float32, maxdisp=12),
    "occluder_whole": dict(B=2, image=(64, 80), crop=(48, 64), origin=[(0, 0), (16, 15)], vflip=[0, 1], swap=[0, 0],
                           occluder=[(24, 40, 32, 50), (10, 3, 6, 3)],
                           brightness=[(1.0, 1.4), (1.0, 0.7)], gamma=[(1.0, 1.1), (1.0, 0.9)], contrast=[(1.0, 1.1), (1.0, 0.85)],
                           saturation=[(1.0, 0.5), (1.0, 1.3)], keys=("left", "right"), label=torch.uint8, disparity=torch.float32, maxdisp=12),
    # several workgroups' partials per image (see partials_per_image), and the contrast tie in item 1's left view
    "several_workgroups": dict(B=2, image=(96, 128), crop=(96, 128), origin=[(0, 0)] * 2, vflip=[0, 0], swap=[0, 0],
                               occluder=[(50, 20, 60, 30), NONE],
                               brightness=[(1.1, 0.9), (1.0, 1.0)], gamma=[(0.9, 1.1), (1.0, 1.0)], contrast=[(1.2, 0.8), (1.2, 0.8)],
                               saturation=[(1.1, 0.6), (1.0, 1.0)], keys=("left", "right", "disparity", "disparity_4", "label"),
                               label=torch.uint8, disparity=torch.float32, maxdisp=12, tie=1),
    # WHU: an int32 disparity scaled by 1 / 256, no label, the swap
    "whu": dict(B=2, image=(32, 48), crop=(32, 48), origin=[(0, 0)] * 2, vflip=[0, 1], swap=[1, 1], occluder=[NONE, NONE],
                brightness=[(1.3, 0.9), (0.8, 1.1)], gamma=[(1.0, 1.1), (0.9, 1.0)], contrast=[(1.1, 0.9), (1.0, 1.2)],
                saturation=[(0.9, 1.2), (1.4, 0.1)], keys=WHU_SIX, label=None, disparity=torch.int32, maxdisp=12),
    # s = 0, s = 1.4 and b = 2.0 on images that contain 0 and 255
    "edge_values": dict(B=3, image=(16, 24), crop=(16, 24), origin=[(0, 0)] * 3, vflip=[0, 0, 0], swap=[0, 0, 0], occluder=[NONE] * 3,
                        brightness=[(1.0, 1.0), (1.0, 1.0), (2.0, 2.0)], gamma=[(1.0, 1.0)] * 3, contrast=[(1.0, 1.2), (0.8, 1.0), (1.0, 1.0)],
                        saturation=[(0.0, 0.0), (1.4, 1.4), (1.0, 1.4)], keys=FOUR, label=torch.uint8, disparity=torch.float32, maxdisp=12,
                        extremes=True),
}
GPU_CASES = tuple(CASES)


def partials_per_image(H, W, B):
    """Workgroups (and partial sums) per (item, view) of the luma pass, restated from the grid rule of csrc/augment.hip: one lane-trip per
    4 pixels, 256 lanes per workgroup, capped at min(1024, 2048 // (2 B))."""
    quads = (H * W + 3) // 4
    return max(1, min(-(-quads // 256), 1024, max(1, 2048 // (2 * B))))


@functools.lru_cache(maxsize=None)
def raw_of(name):
    """The raw batch of a case (CPU tensors; never modified: callers that move it build a new dictionary)."""
    c = CASES[name]
    B, (H, W) = c["B"], c["image"]
    g = torch.Generator().manual_seed(sorted(CASES).index(name) + 11)
    left = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    right = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    if c.get("extremes"):
        left[:, ::3, ::2], left[:, 1::3, 1::2], right[:, ::2, ::3], right[:, 1::2, ::5] = 0, 255, 255, 0
    if "tie" in c:
        grey = torch.full((H, W, 3), TIE_K, dtype=torch.uint8)
        grey.view(-1, 3)[1::2] = TIE_K + 1                                        # every second pixel: exactly half of them
        left[c["tie"]] = grey
    m = c["maxdisp"]
    d = torch.randint(-m - 2, m + 3, (B, H, W), generator=g).to(torch.float32) + torch.randint(0, 4, (B, H, W), generator=g) * 0.25
    raw = {"left_u8": left, "right_u8": right}
    raw["disparity"] = (d * 256).to(torch.int32) if c["disparity"] == torch.int32 else d
    if c["label"] is not None:
        raw["label"] = torch.randint(0, 6, (B, H, W), generator=g).to(c["label"])
    return raw


def params_of(name):
    from semstereo_amd.augment import AugmentParams
    c = CASES[name]
    return AugmentParams(c["crop"], c["image"], c["origin"], c["vflip"], c["swap"], c["occluder"], c["brightness"], c["gamma"],
                         c["contrast"], c["saturation"])


# ------------------------------------------------------------------------------------------------ the restatement
def luma(r, g, b):
    return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16


def blend(deg, x, f):
    t = np.float32(deg) + np.float32(f) * np.float32(x - deg)       # (numpy scalars: the product is rounded, then the sum)
    return int(min(max(t, np.float32(0)), np.float32(255)))


def view_codes():
    """float32 [3][256]: (u / 255 - mean) / std, in fp32 and in that order."""
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    return [[(np.float32(u) / np.float32(255) - np.float32(mean[c])) / np.float32(std[c]) for u in range(256)] for c in range(3)]


def right_maps(d, y, lo, hi):
    """right_view of one image, a raster-order loop (the last writer of a column is the largest x): (right_disparity, right_label)."""
    H, W = d.shape
    rd, rl = np.full((H, W), -999.0, dtype=np.float32), np.full((H, W), 5.0, dtype=np.float32)
    for h in range(H):
        for x in range(W):
            v = d[h, x]
            if np.float32(lo) <= v < np.float32(hi):
                t = np.round(np.float32(x) - v)                     # half to even
                if 0 <= t < W:
                    rd[h, int(t)] = v
                    if y is not None:
                        rl[h, int(t)] = y[h, x]
    return rd, rl


def restate(raw, c):
    """The sample of case dictionary `c` from numpy `raw`, pixel by pixel: {key: float32 array}."""
    left, right = raw["left_u8"].numpy(), raw["right_u8"].numpy()
    B, H, W, _ = left.shape
    (th, tw), keys = c["crop"], c["keys"]
    codes = view_codes()
    out = {k: [] for k in keys}
    disparity = raw["disparity"].numpy()
    scale = np.float32(1.0 / 256.0) if disparity.dtype == np.int32 else np.float32(1.0)
    label = raw["label"].numpy() if "label" in raw else None
    for i in range(B):
        (y0, x0), vflip, swap, (cy, sy, cx, sx) = c["origin"][i], c["vflip"][i], c["swap"][i], c["occluder"][i]

        def source(y, x):
            return y0 + (th - 1 - y if vflip else y), (W - 1 - (x0 + x) if swap else x0 + x)
        for v, key in enumerate(("left", "right")):
            if key not in keys:
                continue
            b, g, con, s = (c[n][i][v] for n in ("brightness", "gamma", "contrast", "saturation"))
            src = ((left, right)[v ^ 1] if swap else (left, right)[v])[i].tolist()
            G = [int((255 + 1 - 1e-3) * pow(e / 255.0, g)) for e in range(256)]
            T1 = [G[blend(0, u, b)] for u in range(256)]
            S = sum(luma(T1[p[0]], T1[p[1]], T1[p[2]]) for row in src for p in row)
            m = int(S / (H * W) + 0.5)
            T3 = [blend(m, T1[u], con) for u in range(256)]
            u4 = [[None] * tw for _ in range(th)]
            for y in range(th):
                for x in range(tw):
                    ys, xs = source(y, x)
                    u3 = [T3[p] for p in src[ys][xs]]
                    L3 = luma(*u3)
                    u4[y][x] = [blend(L3, u, s) for u in u3]
            if v == 1 and sy > 0 and sx > 0:
                colour = [sum(u4[y][x][ch] for y in range(th) for x in range(tw)) // (th * tw) for ch in range(3)]
                for y in range(max(cy - sy, 0), min(cy + sy, th)):
                    for x in range(max(cx - sx, 0), min(cx + sx, tw)):
                        u4[y][x] = colour
            out[key].append(np.array([[[codes[ch][u4[y][x][ch]] for x in range(tw)] for y in range(th)] for ch in range(3)], dtype=np.float32))
        d = disparity[i].astype(np.float32) * scale
        y_full = None if label is None else label[i].astype(np.float32)
        if swap and any(k.startswith(("disparity", "label")) for k in keys):
            d, y_full = right_maps(d, y_full, -c["maxdisp"], c["maxdisp"])
        for prefix, full in (("disparity", d), ("label", y_full)):
            names = [k for k in keys if k.startswith(prefix)]
            if not names:
                continue
            a = np.empty((th, tw), dtype=np.float32)
            for y in range(th):
                for x in range(tw):
                    a[y, x] = full[source(y, x)]
            for k in names:
                step = int(k.split("_")[1]) if "_" in k else 1
                out[k].append(np.array([[a[y * step, x * step] for x in range(tw // step)] for y in range(th // step)], dtype=np.float32))
    return {k: np.stack(v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def restated(name):
    return restate(raw_of(name), CASES[name])


@functools.lru_cache(maxsize=None)
def composed(name):
    """The PyTorch composition of a case on the CPU: the GPU tests' reference, computed once."""
    from semstereo_amd.augment import augment_sample
    c = CASES[name]
    return augment_sample(raw_of(name), params_of(name), c["keys"], maxdisp=c["maxdisp"])
