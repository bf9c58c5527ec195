#!/usr/bin/env python3
"""The segmentation heads and the chal_* projections under autograd, measured (models/SemStereo.py:254-265 in train(): head_l, head_r,
chal_0 .. chal_4 on the left pyramid, chal_1 / chal_2 on the right one): forward + backward of every layer two ways in one process,
warm, alternating round by round:

  hip      the twins with engine.HEADS_TRAIN_HIP on: train_heads.seghead_train / proj_train (csrc/seghead_train.hip, the 3x3 / 1x1
           training seams of train.py, batch statistics in the BatchNorm kernels)
  torch    the same twins with the switch off: the stock PyTorch layers (Conv2d, BatchNorm2d, ReLU, F.interpolate) and their autograd

on closed-form pyramid features that require grad (the backbone trains), in train() mode, with a closed-form gradient on the outputs.
Per layer: median / min / max device time of one forward + backward over the rounds for both, the ratio and both spreads; each round's
window is `--window-ms` of device time long (its iteration count is fixed per layer and variant after the warm-up).  A projection of
fewer than train_heads.PROJ_MIN_POSITIONS positions keeps the stock layers with the switch on too (the record says which calls did;
--min-positions 0 measures every layer on HIP).  The last row is the nine calls of a training step together (both heads, seven
projections); for it the peak device memory of one forward + backward above what was allocated before it is reported too.  --out FILE
keeps the record as JSON.  Needs the GPU: there is no fall-back.

usage: python tools/bench_heads_train.py [--shapes 1024x4,1024x1] [--rounds 5 --window-ms 100] [--min-positions 0] [--out profiles/heads_train_bench.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHAL_IN = (128, 256, 512, 768, 512)
CHAL_OUT = (64, 128, 256, 384, 256)
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
    ap.add_argument("--min-positions", type=int, default=-1, help="train_heads.PROJ_MIN_POSITIONS for the run (default: the module's)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.rounds >= 3, "at least three rounds: 'slower in every round' is decided on all of them"
    import torch
    import semstereo_amd as sa
    E, M = sa.engine, sa.modules
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_heads_train.py measures on the GPU and found none (there is no fall-back)")
    assert E.CONV_ENGINE == "f16x3" and E.TRAIN_HIP and E._heads_hip_on()
    TH = __import__("semstereo_amd.train_heads", fromlist=["x"])
    if args.min_positions >= 0:
        TH.PROJ_MIN_POSITIONS = args.min_positions
    torch.manual_seed(0)
    head_l, head_r = M.segmenthead(128, 32, 6, 2).cuda().train(), M.segmenthead(128, 32, 6, 2).cuda().train()
    chals = [M.ChalProjection(ci, co).cuda().train() for ci, co in zip(CHAL_IN, CHAL_OUT)]
    params = [p for m in [head_l, head_r] + chals for p in m.parameters()]
    record = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_ms": args.window_ms,
              "min_positions": TH.PROJ_MIN_POSITIONS, "shapes": {}}

    def step(variant, calls):
        """forward + backward of `calls` = [(module, input, gradient on the output)]"""
        E.HEADS_TRAIN_HIP = variant == "hip"
        try:
            for p in params:
                p.grad = None
            ys = []
            for m, x, _ in calls:
                x.grad = None
                ys.append(m(x))
            torch.autograd.backward(ys, [g for _, _, g in calls])
        finally:
            E.HEADS_TRAIN_HIP = False

    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(variant, calls, iters):
        ev0.record()
        for _ in range(iters):
            step(variant, calls)
        ev1.record()
        ev1.synchronize()
        return ev0.elapsed_time(ev1) * 1e3 / iters             # us per forward + backward

    for spec in args.shapes.split(","):
        size, B = (int(v) for v in spec.split("x"))
        L = [closed_form(torch, (B, c, size >> (k + 1), size >> (k + 1)), k).requires_grad_(True) for k, c in enumerate(CHAL_IN)]
        R = [closed_form(torch, (B, c, size >> (k + 1), size >> (k + 1)), 10 + k).requires_grad_(True) for k, c in enumerate(CHAL_IN)]

        def with_grad(m, x, salt):
            with torch.no_grad():
                shape = tuple(m(x).shape)
            return (m, x, closed_form(torch, shape, 20 + salt))
        Bn, Cin, H, W = L[0].shape
        entries = [(f"head_l {Cin}->32->6 @{H}x{W} (+ x2 up-sampling)", [with_grad(head_l, L[0], 0)])]
        for k, c in enumerate(chals):
            Bn, Cin, H, W = L[k].shape
            if k in (1, 2):
                entries.append((f"chal_{k} {Cin}->{CHAL_OUT[k]} @{H}x{W} x2 views", [with_grad(c, L[k], k), with_grad(c, R[k], 5 + k)]))
            else:
                entries.append((f"chal_{k} {Cin}->{CHAL_OUT[k]} @{H}x{W}", [with_grad(c, L[k], k)]))
        entries.append(("the nine calls of a training step", [with_grad(head_r, R[0], 9)] + [c for _, calls in entries for c in calls]))

        iters, times, before_counts = {}, {name: {v: [] for v in VARIANTS} for name, _ in entries}, dict(M.PATH_COUNTS)
        stock_calls = {}                                       # calls of the switch-on step that kept the stock layers (below the threshold)
        for name, calls in entries:                            # warm every shape both ways; size the windows
            for v in VARIANTS:
                t0 = M.PATH_COUNTS["torch"]
                step(v, calls)
                if v == "hip":
                    stock_calls[name] = M.PATH_COUNTS["torch"] - t0
                torch.cuda.synchronize()
                t = window(v, calls, 2)
                iters[name, v] = max(3, int(math.ceil(args.window_ms * 1e3 / max(t, 1.0))))
        assert M.PATH_COUNTS.get("hip_train", 0) > before_counts.get("hip_train", 0), "the switch did not reach the HIP path"
        peak = {}
        for v in VARIANTS:                                      # peak memory of the nine calls above what is resident
            step(v, entries[-1][1])
            torch.cuda.synchronize()
            for p in params:
                p.grad = None
            for x in L + R:
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
                    times[name][v].append(window(v, calls, iters[name, v]))
        rows = []
        print(f"== {size} x {size}, batch {B} ==")
        for name, _ in entries:
            row = {"layer": name, "calls": len(dict(entries)[name]), "calls_on_stock_layers_with_the_switch_on": stock_calls[name]}
            for v in VARIANTS:
                t = times[name][v]
                row[v] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t), "rounds_us": t, "iters_per_round": iters[name, v]}
                row[v + "_spread"] = (max(t) - min(t)) / statistics.median(t)
            row["torch_over_hip"] = row["torch"]["median_us"] / row["hip"]["median_us"]
            same = stock_calls[name] == row["calls"]           # every call below the threshold: the same code both ways, nothing to decide
            row["hip_slower_in_every_round"] = None if same else all(h > t for h, t in zip(times[name]["hip"], times[name]["torch"]))
            row["hip_faster_in_every_round"] = None if same else all(h < t for h, t in zip(times[name]["hip"], times[name]["torch"]))
            rows.append(row)
            print(f"{name:52s} " + "  ".join(f"{v} {row[v]['median_us']:9.1f} us [{row[v]['min_us']:.1f}, {row[v]['max_us']:.1f}]" for v in VARIANTS)
                  + f"  torch/hip {row['torch_over_hip']:5.2f}" + ("  HIP SLOWER IN EVERY ROUND" if row["hip_slower_in_every_round"] else "")
                  + (f"  ({stock_calls[name]} of {row['calls']} calls below the threshold: stock layers both ways)" if stock_calls[name] else ""))
        print(f"peak memory of the nine calls (forward + backward) above the resident tensors: hip {peak['hip']:.0f} MiB, torch {peak['torch']:.0f} MiB")
        record["shapes"][spec] = {"size": size, "batch": B, "layers": rows, "peak_mib_nine_calls": peak}
        del L, R, entries
        for p in params:
            p.grad = None
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
    print(json.dumps({"heads_train_nine_calls_us": {k: {v: s["layers"][-1][v]["median_us"] for v in VARIANTS} for k, s in record["shapes"].items()}}))


if __name__ == "__main__":
    main()
