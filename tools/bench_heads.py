#!/usr/bin/env python3
"""The segmentation heads and the chal_* projections, measured (models/SemStereo.py:254-265: head_l, head_r, chal_0 .. chal_4 on the
left pyramid, chal_1 / chal_2 on the right one): every layer two ways in one process, warm, alternating round by round:

  hip      the kernels the twins run in inference: engine.run_seghead (csrc/seghead_f16s.hip: logits in one pass + the x2 up-sampling)
           and engine.run_conv2d_k1 (csrc/proj2d_f16s.hip; chal_1 / chal_2: both views in one launch)
  torch    the same layer on the stock PyTorch modules (Conv2d, BatchNorm2d, ReLU, F.interpolate): what runs without
           accelerate(heads=True), i.e. at the parent commit

on closed-form pyramid features (the five maps FeatUp hands on, 1/2 .. 1/32).  Per layer: median / min / max device time over the
rounds for both, the ratio and both spreads; for hip the bytes the layer has to move (input once, output once) over the time.  The
last row is the nine calls of an eval forward together: on the stock layers head_l, head_r and seven projections; on HIP head_l (the
result of head_r is never read, so the twin never launches it) and the seven projections in five launches.  --out FILE keeps the
record as JSON.

usage: python tools/bench_heads.py [--shapes 1024x1,1024x4,2048x1] [--rounds 5 --iters 10] [--only hip] [--out profiles/heads_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHAL_IN = (128, 256, 512, 768, 512)
CHAL_OUT = (64, 128, 256, 384, 256)


def closed_form(torch, shape, salt):
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, device="cuda", dtype=torch.float32)
    return torch.sin(i * (0.61803 + 0.001 * salt) + salt).reshape(shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x1,1024x4,2048x1")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--miopen-find", action="store_true", help="torch.backends.cudnn.benchmark for the torch legs")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.rounds >= 3, "at least three rounds: the default of a layer is decided on all of them"
    import torch
    import torch.nn.functional as F
    import semstereo_amd as sa
    E, M = sa.engine, sa.modules
    assert torch.cuda.is_available() and E.CONV_ENGINE == "f16x3"
    torch.backends.cudnn.benchmark = args.miopen_find         # (off: PyTorch's default, MIOpen's immediate mode -- what a script gets)
    torch.manual_seed(0)
    head_l, head_r = M.segmenthead(128, 32, 6, 2).cuda().eval(), M.segmenthead(128, 32, 6, 2).cuda().eval()
    chals = [M.ChalProjection(ci, co).cuda().eval() for ci, co in zip(CHAL_IN, CHAL_OUT)]
    variants = [v for v in ("hip", "torch") if not args.only or v == args.only]
    record = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters, "shapes": {}}

    def stock_head(h, x):
        x = F.relu(h.conv1.bn(h.conv1.conv(x)))
        return F.interpolate(h.conv2(x), size=[x.shape[-2] * 2, x.shape[-1] * 2], mode="bilinear", align_corners=False)

    def stock_chal(c, x):
        return c[1](c[0](x))

    for spec in args.shapes.split(","):
        size, B = (int(v) for v in spec.split("x"))
        L = [closed_form(torch, (B, c, size >> (k + 1), size >> (k + 1)), k) for k, c in enumerate(CHAL_IN)]
        R = [closed_form(torch, (B, c, size >> (k + 1), size >> (k + 1)), 10 + k) for k, c in enumerate(CHAL_IN)]
        entries = []          # (name, bytes the layer must move, {variant: callable})
        with torch.no_grad():
            Bn, Cin, H, W = L[0].shape
            entries.append((f"head_l {Cin}->32->6 @{H}x{W} (+ x2 up-sampling)", 4 * Bn * H * W * (Cin + 6 + 6 + 24), {
                "hip": (lambda: E.run_seghead(head_l, head_l, L[0])),
                "torch": (lambda: stock_head(head_l, L[0]))}))
            for k, c in enumerate(chals):
                Bn, Cin, H, W = L[k].shape
                Co = CHAL_OUT[k]
                if k in (1, 2):
                    entries.append((f"chal_{k} {Cin}->{Co} @{H}x{W} x2 views", 2 * 4 * Bn * H * W * (Cin + Co), {
                        "hip": (lambda c=c, k=k: E.run_conv2d_k1(c, "chal", c[0], c[1], L[k], False, xb=R[k])),
                        "torch": (lambda c=c, k=k: (stock_chal(c, L[k]), stock_chal(c, R[k])))}))
                else:
                    entries.append((f"chal_{k} {Cin}->{Co} @{H}x{W}", 4 * Bn * H * W * (Cin + Co), {
                        "hip": (lambda c=c, k=k: E.run_conv2d_k1(c, "chal", c[0], c[1], L[k], False)),
                        "torch": (lambda c=c, k=k: stock_chal(c, L[k]))}))
            layer_fns = [fns for _, _, fns in entries]
            entries.append(("the nine calls of an eval forward", sum(b for _, b, _ in entries), {
                "hip": (lambda: [fns["hip"]() for fns in layer_fns]),
                "torch": (lambda: [stock_head(head_r, R[0])] + [fns["torch"]() for fns in layer_fns])}))

            times = {name: {v: [] for v in variants} for name, _, _ in entries}
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for name, _, fns in entries:                      # warm: weight packing, MIOpen's search
                for v in variants:
                    for _ in range(2):
                        out = fns[v]()
                        assert out is not None and (not isinstance(out, list) or all(o is not None for o in out)), (name, v)
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for name, _, fns in entries:
                    for v in variants:
                        ev0.record()
                        for _ in range(args.iters):
                            fns[v]()
                        ev1.record()
                        ev1.synchronize()
                        times[name][v].append(ev0.elapsed_time(ev1) * 1e3 / args.iters)      # us per call
        rows = []
        print(f"== {size} x {size}, batch {B} ==")
        for name, nbytes, _ in entries:
            row = {"layer": name, "mbytes_min": nbytes / 1e6}
            for v in variants:
                t = times[name][v]
                row[v] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t), "rounds_us": t}
            if "hip" in row:
                row["hip_gbytes_per_s"] = nbytes / row["hip"]["median_us"] / 1e3
            if len(variants) == 2:
                row["torch_over_hip"] = row["torch"]["median_us"] / row["hip"]["median_us"]
                row["hip_slower_in_every_round"] = all(h > t for h, t in zip(times[name]["hip"], times[name]["torch"]))
                row["torch_spread"] = (row["torch"]["max_us"] - row["torch"]["min_us"]) / row["torch"]["median_us"]
                row["hip_spread"] = (row["hip"]["max_us"] - row["hip"]["min_us"]) / row["hip"]["median_us"]
            rows.append(row)
            print(f"{name:52s} " + "  ".join(f"{v} {row[v]['median_us']:9.1f} us [{row[v]['min_us']:.1f}, {row[v]['max_us']:.1f}]" for v in variants)
                  + (f"  torch/hip {row['torch_over_hip']:5.2f}{'  HIP SLOWER IN EVERY ROUND' if row['hip_slower_in_every_round'] else ''}" if len(variants) == 2 else "")
                  + (f"  {row['hip_gbytes_per_s']:7.1f} GB/s of the bytes it must move" if "hip" in row else ""))
        record["shapes"][spec] = {"size": size, "batch": B, "layers": rows}
        del L, R, entries, layer_fns
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
    print(json.dumps({"heads_nine_calls_us": {k: {v: v_["layers"][-1][v]["median_us"] for v in variants} for k, v_ in record["shapes"].items()}}))


if __name__ == "__main__":
    main()
