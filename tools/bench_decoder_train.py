#!/usr/bin/env python3
"""The 2-D decoder under autograd, measured (models/SemStereo.py:59-86, 207-211 in train(): FeatUp's four Conv2x on both views, the
spx chain's four Conv2x, spx2): forward + backward of every layer two ways in one process, warm, alternating round by round:

  hip      the twins with engine.DECODER_TRAIN_HIP on: train_decoder.conv2x_train / spx2_train (csrc/deconv2d_train.hip, the
           transposed and concat-free forward kernels, the 3x3 training seams of train.py, batch statistics in the BatchNorm kernels)
  torch    the same twins with the switch off: the stock PyTorch layers (ConvTranspose2d, Conv2d, BatchNorm2d, ReLU, torch.cat) and
           their autograd -- what runs at the parent commit

on closed-form pyramid features that require grad (the backbone trains), in train() mode, with a closed-form gradient on the outputs.
Per layer: median / min / max device time of one forward + backward over the rounds for both, the ratio and both spreads; each round's
window is `--window-ms` of device time long (its iteration count is fixed per layer and variant after the warm-up).  The record says
how many calls of a switch-on step kept the stock layers (none, unless `*_applies` declines a shape).  The last row is the thirteen calls
of a training step together; for it the peak
device memory of one forward + backward above what was allocated before it is reported too.  Per transposed layer the two gradient
kernels are also timed alone (TFLOP/s fp32-equivalent = 2 * positions * Cin * Cout * 16 / time), next to the depth-1 route of the 3x3
weight gradient through conv3d_wgrad_hip.  --out FILE keeps the record as JSON.  Needs the GPU: there is no fall-back.

usage: python tools/bench_decoder_train.py [--shapes 1024x4,1024x1] [--rounds 5 --window-ms 100] [--out profiles/decoder_train_bench.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHANS = (64, 128, 256, 384, 512)                # the backbone's maps at 1/2 .. 1/32 (models/SemStereo.py:62)
CHANS2 = (64, 128, 256, 384, 256)               # ... after chal_0 .. chal_4 (models/SemStereo.py:197)
# name -> (Cin, Cout, level of x: the map at 1 / 2^(level+1)); FeatUp's layers run on both views
FEATUP = (("deconv32_16", 512, 384, 4), ("deconv16_8", 768, 256, 3), ("deconv8_4", 512, 128, 2), ("deconv4_2", 256, 64, 1))
SPX = (("spx32_16", 256, 384, 4), ("spx16_8", 768, 256, 3), ("spx8_4", 512, 128, 2), ("spx4_2", 256, 64, 1))
VARIANTS = ("hip", "torch")


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
    assert args.rounds >= 3, "at least three rounds: 'slower in every round' is decided on all of them"
    import torch
    import semstereo_amd as sa
    E, M = sa.engine, sa.modules
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_decoder_train.py measures on the GPU and found none (there is no fall-back)")
    assert E.CONV_ENGINE == "f16x3" and E.TRAIN_HIP and E._decoder_hip_on()
    TD = __import__("semstereo_amd.train_decoder", fromlist=["x"])
    torch.manual_seed(0)
    layers = {name: M.Conv2x(ci, co, deconv=True).cuda().train() for name, ci, co, _ in FEATUP + SPX}
    layers["spx2"] = M.Spx2(128, 6).cuda().train()
    params = [p for m in layers.values() for p in m.parameters()]
    record = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_ms": args.window_ms,
              "shapes": {}}

    def step(variant, calls):
        """forward + backward of `calls` = [(module, inputs, gradient on the output)]"""
        E.DECODER_TRAIN_HIP = variant == "hip"
        try:
            for p in params:
                p.grad = None
            ys = []
            for m, xs, _ in calls:
                for x in xs:
                    x.grad = None
                ys.append(m(*xs))
            torch.autograd.backward(ys, [g for _, _, g in calls])
        finally:
            E.DECODER_TRAIN_HIP = False

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

    for spec in args.shapes.split(","):
        size, B = (int(v) for v in spec.split("x"))

        def fmap(C, level, salt):
            return closed_form(torch, (B, C, size >> (level + 1), size >> (level + 1)), salt).requires_grad_(True)

        def with_grad(m, xs, salt):
            with torch.no_grad():
                shape = tuple(m(*xs).shape)
            return (m, xs, closed_form(torch, shape, 40 + salt))

        entries = []
        for k, (name, ci, co, lv) in enumerate(FEATUP):
            calls = [with_grad(layers[name], (fmap(ci, lv, 10 * v + k), fmap(co, lv - 1, 10 * v + k + 5)), 10 * v + k) for v in range(2)]
            entries.append((f"{name} {ci}->{co} @{size >> (lv + 1)}x{size >> (lv + 1)} x2 views", calls))
        for k, (name, ci, co, lv) in enumerate(SPX):
            entries.append((f"{name} {ci}->{co} @{size >> (lv + 1)}x{size >> (lv + 1)}",
                            [with_grad(layers[name], (fmap(ci, lv, 20 + k), fmap(co, lv - 1, 25 + k)), 20 + k)]))
        entries.append((f"spx2 128->6 @{size >> 1}x{size >> 1}", [with_grad(layers["spx2"], (fmap(128, 0, 30),), 30)]))
        entries.append(("the thirteen calls of a training step", [c for _, calls in entries for c in calls]))
        inputs = [x for _, calls in entries[:-1] for _, xs, _ in calls for x in xs]

        iters, times, before_counts = {}, {name: {v: [] for v in VARIANTS} for name, _ in entries}, dict(M.PATH_COUNTS)
        stock_calls = {}                                       # calls of the switch-on step that kept the stock layers
        for name, calls in entries:                            # warm every shape both ways; size the windows
            for v in VARIANTS:
                d0 = M.PATH_COUNTS.get("decoder_train", 0)
                iters[name, v] = sized(lambda: step(v, calls))
                if v == "hip":
                    stock_calls[name] = len(calls) - (M.PATH_COUNTS.get("decoder_train", 0) - d0) // 3      # (sized() ran three steps)
        assert M.PATH_COUNTS.get("decoder_train", 0) > before_counts.get("decoder_train", 0), "the switch did not reach the HIP path"
        peak = {}
        for v in VARIANTS:                                      # peak memory of the thirteen calls above what is resident
            step(v, entries[-1][1])
            torch.cuda.synchronize()
            for p in params:
                p.grad = None
            for x in inputs:
                x.grad = None
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            step(v, entries[-1][1])
            torch.cuda.synchronize()
            peak[v] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        for _ in range(args.rounds):
            for name, calls in entries:
                for v in VARIANTS:
                    times[name][v].append(timed(lambda: step(v, calls), iters[name, v]))
        rows = []
        print(f"== {size} x {size}, batch {B} ==")
        for name, calls in entries:
            row = {"layer": name, "calls": len(calls), "calls_on_stock_layers_with_the_switch_on": stock_calls[name]}
            for v in VARIANTS:
                t = times[name][v]
                row[v] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t), "rounds_us": t, "iters_per_round": iters[name, v]}
                row[v + "_spread"] = (max(t) - min(t)) / statistics.median(t)
            row["torch_over_hip"] = row["torch"]["median_us"] / row["hip"]["median_us"]
            same = stock_calls[name] == row["calls"]           # every call on the stock layers: the same code both ways, nothing to decide
            row["hip_slower_in_every_round"] = None if same else all(h > t for h, t in zip(times[name]["hip"], times[name]["torch"]))
            row["hip_faster_in_every_round"] = None if same else all(h < t for h, t in zip(times[name]["hip"], times[name]["torch"]))
            rows.append(row)
            print(f"{name:44s} " + "  ".join(f"{v} {row[v]['median_us']:10.1f} us [{row[v]['min_us']:.1f}, {row[v]['max_us']:.1f}]" for v in VARIANTS)
                  + f"  torch/hip {row['torch_over_hip']:5.2f}" + ("  HIP SLOWER IN EVERY ROUND" if row["hip_slower_in_every_round"] else "")
                  + (f"  ({stock_calls[name]} of {row['calls']} calls kept the stock layers both ways)" if stock_calls[name] else ""))
        print(f"peak memory of the thirteen calls (forward + backward) above the resident tensors: hip {peak['hip']:.0f} MiB, torch {peak['torch']:.0f} MiB")

        # ---- the gradient kernels alone ----
        kernels = []
        with torch.no_grad():
            for name, ci, co, lv in SPX + (("spx2", 128, 6, 0),):
                H = size >> (lv + 1)
                x, g = closed_form(torch, (B, ci, H, H), 50), closed_form(torch, (B, co, 2 * H, 2 * H), 51)
                w = closed_form(torch, (ci, co, 4, 4), 52) * 0.05
                flop = 2.0 * B * H * H * ci * co * 16
                row = {"layer": f"{name} {ci}->{co} @{H}x{H}", "gflop": flop / 1e9}
                fns = {"wgrad_hip": lambda: TD.deconv2d_k4s2_wgrad_hip(x, g, co),
                       "dgrad_hip": lambda: TD.conv2d_k4s2_hip(g, TD.pack_conv2d_k4s2_weight(w), ci),
                       "wgrad_stock": lambda: torch.ops.aten.convolution_backward(g, x, w, None, [2, 2], [1, 1], [1, 1], True, [0, 0], 1, [False, True, False]),
                       "dgrad_stock": lambda: torch.ops.aten.convolution_backward(g, x, w, None, [2, 2], [1, 1], [1, 1], True, [0, 0], 1, [True, False, False])}
                if name != "spx2":                              # the Conv2x's 3x3 weight gradient: depth-1 volumes through the 3x3x3 kernel, per source
                    y, g3 = closed_form(torch, (B, co, 2 * H, 2 * H), 53), closed_form(torch, (B, 2 * co, 2 * H, 2 * H), 54)
                    w3 = closed_form(torch, (2 * co, co, 3, 3), 55) * 0.05
                    row["gflop_3x3_per_source"] = 2.0 * B * 4 * H * H * co * 2 * co * 9 / 1e9
                    fns["wgrad3x3_depth1_hip_per_source"] = lambda: M.conv3d_wgrad_hip(g3.unsqueeze(2), y.unsqueeze(2), 2 * co, co, 1)
                    fns["wgrad3x3_stock_per_source"] = lambda: torch.ops.aten.convolution_backward(
                        g3, y, w3, None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1, [False, True, False])
                for key, fn in fns.items():
                    n = sized(fn)
                    t = [timed(fn, n) for _ in range(args.rounds)]
                    gf = row["gflop_3x3_per_source"] if "3x3" in key else row["gflop"]
                    row[key] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t),
                                "tflops_fp32_equivalent": gf / statistics.median(t) * 1e3}
                kernels.append(row)
                print(f"{row['layer']:28s} " + "  ".join(f"{k} {row[k]['median_us']:.0f} us ({row[k]['tflops_fp32_equivalent']:.1f} TFLOP/s)" for k in fns))
                del x, g, w
        record["shapes"][spec] = {"size": size, "batch": B, "layers": rows, "peak_mib_thirteen_calls": peak, "gradient_kernels": kernels}
        del entries, inputs
        for p in params:
            p.grad = None
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
    print(json.dumps({"decoder_train_thirteen_calls_us": {k: {v: s["layers"][-1][v]["median_us"] for v in VARIANTS} for k, s in record["shapes"].items()}}))


if __name__ == "__main__":
    main()
