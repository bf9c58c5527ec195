#!/usr/bin/env python3
"""The sparse concat volume of a training step, measured (models/SemStereo.py:316-318 under autograd: `att_topk * cat(left broadcast,
warp(right))`): forward + backward of that op pair alone, two ways in one process, warm, alternating round by round:

  one_launch  train.concat_volume_sampled: ss_concat_sampled_fwd + ss_concat_sampled_bwd (at a quarter-resolution width that is no
              multiple of 64: with train.CONCAT_VOLUME_ANY_WIDTH on)
  statements  what segment.py runs where the one-launch form declines: ops.SpatialTransformer_grid, torch.cat and the multiply under
              autograd, with their three backwards

on [B, 32, H/4, W/4] concat-feature maps that require grad, 24 distinct integer candidates per pixel (oracle.detdata), a gate in
(0, 1) that requires grad and a fixed gradient on the volume.  Per shape and arm: median / min / max over the rounds of the
device-event time of one forward + backward, and torch.cuda.max_memory_allocated of the arm's windows (inputs and the volume's
gradient resident in both).  --out FILE keeps the record as JSON.  Needs the GPU: there is no fall-back.

usage: python tools/bench_concat_train.py [--shapes 896x896x1,896x896x4,640x640x1,640x640x4,1024x1024x1,1024x1024x4] [--rounds 5 --steps 10]
                                          [--margin 16] [--arms one_launch,statements] [--out profiles/concat_anywidth_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="896x896x1,896x896x4,640x640x1,640x640x4,1024x1024x1,1024x1024x4", help="image HxWxB")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="forward + backward pairs per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--margin", type=int, default=16)
    ap.add_argument("--arms", default="one_launch,statements")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.rounds >= 5, "at least five rounds: 'slower in every round' is decided on all of them"
    import torch
    import semstereo_amd as sa
    from oracle import detdata as dd
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_concat_train.py measures on the GPU and found none (there is no fall-back)")
    sa._lib.load()
    T, ops = sa.train, sa.ops
    T.CONCAT_VOLUME_ANY_WIDTH = True
    arms = args.arms.split(",")
    assert set(arms) <= {"one_launch", "statements"}, arms
    C, nd = 32, 24
    res = {"op": "models/SemStereo.py:316-318, forward + backward", "channels": C, "candidates": nd, "margin": args.margin,
           "rounds": args.rounds, "steps_per_round": args.steps, "device": torch.cuda.get_device_name(0), "shapes": {}}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for shape in args.shapes.split(","):
        Hi, Wi, B = (int(v) for v in shape.split("x"))
        H, W = Hi // 4, Wi // 4
        left = dd.t_normalish((B, C, H, W), 881).cuda().requires_grad_(True)
        right = dd.t_normalish((B, C, H, W), 882).cuda().requires_grad_(True)
        d = dd.distinct_sorted_candidates(B, nd, H, W, 32, 883).cuda()
        att = dd.t_uniform((B, 1, nd, H, W), 884, 0.0, 1.0).cuda().requires_grad_(True)
        seed = torch.randn(B, 2 * C, nd, H, W, device="cuda", generator=torch.Generator(device="cuda").manual_seed(885))
        if "one_launch" in arms:
            assert T.concat_volume_applies(left, right, d, att), shape

        def step(arm):
            for t in (left, right, att):
                t.grad = None
            if arm == "one_launch":
                vol = T.concat_volume_sampled(left, right, d, att, margin=args.margin)
            else:
                right_w, left_b = ops.SpatialTransformer_grid(left, right, d)
                vol = att * torch.cat((left_b, right_w), dim=1)
            vol.backward(seed)

        grads = {}
        for arm in arms:
            for _ in range(args.warmup):
                step(arm)
            torch.cuda.synchronize()
            grads[arm] = [t.grad.clone() for t in (left, right, att)]
        rec = {"maps": [B, C, H, W], "volume_mib": B * 2 * C * nd * H * W * 4 / 2 ** 20}
        if len(arms) == 2:      # the two arms computed the same gradients (max |difference| over max |statements|)
            rec["gradients_one_launch_vs_statements"] = {
                k: float((a - b).abs().max() / b.abs().max()) for k, a, b in zip(("left", "right", "att"), grads["one_launch"], grads["statements"])}
        del grads
        ms = {arm: [] for arm in arms}
        peak = {arm: 0 for arm in arms}
        for _ in range(args.rounds):
            for arm in arms:
                for t in (left, right, att):
                    t.grad = None
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                e0.record()
                for _ in range(args.steps):
                    step(arm)
                e1.record()
                torch.cuda.synchronize()
                ms[arm].append(e0.elapsed_time(e1) / args.steps)
                peak[arm] = max(peak[arm], torch.cuda.max_memory_allocated())
        for arm in arms:
            rec[arm] = {"ms": {"median": statistics.median(ms[arm]), "min": min(ms[arm]), "max": max(ms[arm]), "rounds": ms[arm]},
                        "peak_allocated_mib": peak[arm] / 2 ** 20}
        if len(arms) == 2:
            ratios = [a / b for a, b in zip(ms["one_launch"], ms["statements"])]
            rec["one_launch_over_statements"] = {"of_medians": rec["one_launch"]["ms"]["median"] / rec["statements"]["ms"]["median"], "per_round": ratios}
            rec["one_launch_slower_in_every_round"] = all(r > 1.0 for r in ratios)
        res["shapes"][shape] = rec
        print(shape, json.dumps(rec), flush=True)
        del left, right, d, att, seed
        torch.cuda.empty_cache()
        if args.out:                                            # (kept up to date: what was measured before a later failure stays)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
