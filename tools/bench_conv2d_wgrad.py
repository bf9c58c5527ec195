#!/usr/bin/env python3
"""The weight gradient of the 2-D 3x3 convolutions that train on this repo's kernels, measured three ways in one process, warm,
alternating round by round:

  new      train.conv2d_k3_wgrad_hip: ss_conv2d_k3_wgrad_fwd (csrc/conv2d_wgrad.hip), one call for both sources of a Conv2x.conv2
  depth1   the depth-1 route, what runs at the parent commit and with engine.CONV2D_WGRAD_HIP off: conv3d_wgrad_hip on [B,C,1,H,W]
           volumes and the copy of its kd = 1 plane -- for a Conv2x.conv2 two calls, the slices and torch.cat
  stock    aten.convolution_backward with only the weight output (for a Conv2x.conv2 on the materialised concatenation, the
           torch.cat itself not timed)

on the layers of a training step at `--shapes` (input size x batch): the four Conv2x.conv2 shapes as two-source calls
((384+384)->768 @1/16, (256+256)->512 @1/8, (128+128)->256 @1/4, (64+64)->128 @1/2), concat_feature's two convs (128->64, 64->32 @1/4)
and segmenthead.conv1 (128->32 @1/2).  Per layer: median / min / max us over the rounds, TFLOP/s fp32-equivalent
(2 * B * H * W * Cin * Cout * 9 / time) and whether the new kernel was faster than each of the others in EVERY round.  Each round's
window is `--window-ms` of device time long.  --out FILE keeps the record as JSON.  Needs the GPU: there is no fall-back.

usage: python tools/bench_conv2d_wgrad.py [--shapes 1024x4,1024x1] [--rounds 5 --window-ms 100] [--out profiles/conv2d_wgrad_bench.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name, C0, C1, Cout, the map's level (1 / 2^level of the input)
LAYERS = (("Conv2x.conv2 (384+384)->768", 384, 384, 768, 4), ("Conv2x.conv2 (256+256)->512", 256, 256, 512, 3),
          ("Conv2x.conv2 (128+128)->256", 128, 128, 256, 2), ("Conv2x.conv2 (64+64)->128", 64, 64, 128, 1),
          ("concat_feature 128->64", 128, 0, 64, 2), ("concat_feature 64->32", 64, 0, 32, 2), ("segmenthead.conv1 128->32", 128, 0, 32, 1))
ARMS = ("new", "depth1", "stock")


def closed_form(torch, shape, salt):
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, device="cuda", dtype=torch.float32)
    return torch.sin(i * (0.61803 + 0.001 * salt) + salt).reshape(shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x4,1024x1")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=100.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.rounds >= 3, "at least three rounds: 'faster in every round' is decided on all of them"
    import torch
    import semstereo_amd as sa
    M, T = sa.modules, sa.train
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_conv2d_wgrad.py measures on the GPU and found none (there is no fall-back)")
    record = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_ms": args.window_ms, "shapes": {}}
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn, iters):
        ev0.record()
        for _ in range(iters):
            fn()
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1) * 1e3 / iters             # us per call

    def sized(fn):
        fn()
        torch.cuda.synchronize()
        return max(3, int(math.ceil(args.window_ms * 1e3 / max(timed(fn, 2), 1.0))))

    with torch.no_grad():
        for spec in args.shapes.split(","):
            size, B = (int(v) for v in spec.split("x"))
            rows = []
            print(f"== {size} x {size}, batch {B} ==")
            for k, (name, C0, C1, Cout, level) in enumerate(LAYERS):
                H = size >> level
                g, x = closed_form(torch, (B, Cout, H, H), 60 + k), closed_form(torch, (B, C0, H, H), 70 + k)
                rem = closed_form(torch, (B, C1, H, H), 80 + k) if C1 else None
                xcat = x if rem is None else torch.cat((x, rem), 1)
                w = closed_form(torch, (Cout, C0 + C1, 3, 3), 90 + k) * 0.05
                g5 = g.unsqueeze(2)
                if rem is None:
                    depth1 = lambda: M.conv3d_wgrad_hip(g5, x.unsqueeze(2), Cout, C0, 1)[:, :, 1].contiguous()
                else:
                    depth1 = lambda: torch.cat((M.conv3d_wgrad_hip(g5, x.unsqueeze(2), Cout, C0, 1)[:, :, 1],
                                                M.conv3d_wgrad_hip(g5, rem.unsqueeze(2), Cout, C1, 1)[:, :, 1]), 1)
                fns = {"new": lambda: T.conv2d_k3_wgrad_hip(g, x, rem), "depth1": depth1,
                       "stock": lambda: torch.ops.aten.convolution_backward(g, xcat, w, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                                                                            [False, True, False])}
                # the three agree before anything is timed
                a, b, c = fns["new"](), fns["depth1"](), fns["stock"]()[1]
                scale = float(c.abs().max())
                gaps = {"new_vs_depth1": float((a - b).abs().max()) / scale, "new_vs_stock": float((a - c).abs().max()) / scale}
                assert a.shape == b.shape == c.shape and gaps["new_vs_depth1"] < 1e-4, (name, gaps)      # (the stock gap is recorded only)
                del a, b, c
                iters = {arm: sized(fns[arm]) for arm in ARMS}
                times = {arm: [] for arm in ARMS}
                for _ in range(args.rounds):
                    for arm in ARMS:
                        times[arm].append(timed(fns[arm], iters[arm]))
                gflop = 2.0 * B * H * H * (C0 + C1) * Cout * 9 / 1e9
                row = {"layer": f"{name} @{H}x{H}", "sources": 2 if C1 else 1, "gflop": gflop, "max_gap_relative": gaps,
                       "workspace_bytes": T.conv2d_k3_wgrad_workspace_bytes(B, C0, C1, H, H, Cout)}
                for arm in ARMS:
                    t = times[arm]
                    row[arm] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t), "rounds_us": t,
                                "iters_per_round": iters[arm], "tflops_fp32_equivalent": gflop / statistics.median(t) * 1e3}
                for other in ("depth1", "stock"):
                    row[f"new_faster_than_{other}_in_every_round"] = all(n < o for n, o in zip(times["new"], times[other]))
                    row[f"new_slower_than_{other}_in_every_round"] = all(n > o for n, o in zip(times["new"], times[other]))
                    row[f"{other}_over_new"] = row[other]["median_us"] / row["new"]["median_us"]
                rows.append(row)
                print(f"{row['layer']:40s} " + "  ".join(f"{arm} {row[arm]['median_us']:8.1f} us ({row[arm]['tflops_fp32_equivalent']:6.1f} TFLOP/s)"
                                                         for arm in ARMS)
                      + f"  depth1/new {row['depth1_over_new']:.2f}  stock/new {row['stock_over_new']:.2f}")
                del g, x, rem, xcat, w, g5
                torch.cuda.empty_cache()
            record["shapes"][spec] = {"size": size, "batch": B, "layers": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
    print(json.dumps({"conv2d_k3_wgrad_us": {k: {r["layer"]: {arm: round(r[arm]["median_us"], 1) for arm in ARMS} for r in s["layers"]}
                                             for k, s in record["shapes"].items()}}))


if __name__ == "__main__":
    main()
