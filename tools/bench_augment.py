#!/usr/bin/env python3
"""Training augmentation, measured (semstereo_amd/augment.py, csrc/augment.hip) on 1024 x 1024 raw items, batch 4 and 1, with a
512 x 1024 crop and with the whole image as the crop, the five keys a training script reads (left, right, disparity, disparity_4,
label), in one process, the variants alternating round by round:

  hip      augment_sample on csrc/augment.hip
  torch    the same call with engine.AUGMENT_HIP off: the PyTorch composition on the device
  prepare  prepare_sample with the same keys on a raw batch of the OUTPUT size: what an un-augmented batch costs
  copy     ss_tool_copy_fwd moving as many bytes as the three passes must (half read, half written)

Two recipes: "kitti" (no flips, item 0 with an occluder: three launches) and "us3d" (every second item swapped and flipped, item 0 with
an occluder: right_view's launch as well).  Per shape, recipe and variant: device-event time, host time to issue a call and wall time per
call for every round, their medians, the algorithmic bytes and hip's fraction of the copy's rate in the same run.
`hip_slower_than_torch_in_any_round` is the routing rule's input: it must be false at every shape.  --once runs three hip calls of one
shape and leaves: the program of a `rocprofv3 --kernel-trace --stats` run, which gives the kernels' own times.

usage: python tools/bench_augment.py [--batches 4,1] [--rounds 7 --window-ms 100] [--out profiles/augment_bench.json] [--once]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIVE = ("left", "right", "disparity", "disparity_4", "label")
MAXDISP = 64


def algorithmic_bytes(B, H, W, th, tw, occluders):
    """What the three passes must move, from the shapes alone: both raw views read whole for the luma sums; the crop of one view per
    flagged item read for the occluder's sums; the crops read and both views, the disparity, disparity_4 and the label written."""
    n, c = B * H * W, B * th * tw
    return 2 * 3 * n + occluders * 3 * th * tw + 2 * c * (3 + 12) + c * (4 + 4) + 2 * 4 * (c // 16) + c * (1 + 4)


def params_of(sa, recipe, B, H, W, th, tw):
    draw = sa.Augmentation(crop=(th, tw), seed=5).draw(B, H, W)
    flips = [i % 2 == 0 for i in range(B)] if recipe == "us3d" else [False] * B
    occluder = [[th // 2, 80, tw // 2, 60]] + [[-1] * 4] * (B - 1)
    return sa.AugmentParams((th, tw), (H, W), draw.origin, flips, flips, occluder, draw.brightness, draw.gamma,
                            draw.contrast, draw.saturation)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4,1")
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20, help="least calls per timed window")
    ap.add_argument("--window-ms", type=float, default=100.0, help="work per timed window")
    ap.add_argument("--once", action="store_true", help="three hip calls at batch 4 with the 512 x 1024 crop, recipe us3d, and nothing else")
    ap.add_argument("--out", default=None, help="write the whole record to this JSON file")
    args = ap.parse_args()
    H, W = args.height, args.width

    import torch
    import semstereo_amd as sa
    from semstereo_amd._lib import call
    assert torch.cuda.is_available(), "bench_augment.py needs the MI355X"
    sa._lib.load()
    dev = torch.device("cuda")

    def batch(B, h, w):
        g = torch.Generator(device=dev).manual_seed(97)
        return {"left_u8": torch.randint(0, 256, (B, h, w, 3), generator=g, device=dev, dtype=torch.uint8),
                "right_u8": torch.randint(0, 256, (B, h, w, 3), generator=g, device=dev, dtype=torch.uint8),
                "disparity": 2 * MAXDISP * torch.rand(B, h, w, generator=g, device=dev) - MAXDISP,
                "label": torch.randint(0, 6, (B, h, w), generator=g, device=dev, dtype=torch.uint8)}

    if args.once:
        raw, P = batch(4, H, W), params_of(sa, "us3d", 4, H, W, H // 2, W)
        for _ in range(3):
            sa.augment_sample(raw, P, FIVE, maxdisp=MAXDISP)
        torch.cuda.synchronize()
        return

    def composition(fn):
        def wrapper():
            sa.engine.AUGMENT_HIP = False
            try:
                return fn()
            finally:
                sa.engine.AUGMENT_HIP = True
        return wrapper

    res = {"workload": f"{H}x{W} raw items, keys {FIVE}", "rounds": args.rounds, "window_ms": args.window_ms, "shapes": {}}
    worst = False
    for B in [int(b) for b in args.batches.split(",")]:
        raw = batch(B, H, W)
        for th, tw in ((H // 2, W), (H, W)):
            plain = batch(B, th, tw)
            for recipe in ("kitti", "us3d"):
                P = params_of(sa, recipe, B, H, W, th, tw)
                nbytes = algorithmic_bytes(B, H, W, th, tw, 1)
                src = torch.empty(nbytes // 2 // 16 * 16, dtype=torch.uint8, device=dev)
                dst = torch.empty_like(src)
                hip = lambda: sa.augment_sample(raw, P, FIVE, maxdisp=MAXDISP)                               # noqa: E731
                variants = {"hip": hip, "torch": composition(hip), "prepare": lambda: sa.prepare_sample(plain, True, FIVE),
                            "copy": lambda: call("ss_tool_copy_fwd", src.data_ptr(), dst.data_ptr(), src.numel())}
                a, b = variants["hip"](), variants["torch"]()
                differing = {k: int((a[k].view(torch.int32) != b[k].view(torch.int32)).sum()) for k in a}
                iters = {}
                for name, fn in variants.items():
                    for _ in range(3):
                        fn()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(5):
                        fn()
                    torch.cuda.synchronize()
                    iters[name] = int(min(max(args.window_ms / (1e3 * (time.perf_counter() - t0) / 5), args.iters), 2000))
                times = {v: {"device_ms": [], "host_issue_ms": [], "wall_ms": []} for v in variants}
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for _ in range(args.rounds):
                    for name, fn in variants.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        e0.record()
                        for _ in range(iters[name]):
                            fn()
                        e1.record()
                        t1 = time.perf_counter()
                        torch.cuda.synchronize()
                        t2 = time.perf_counter()
                        times[name]["device_ms"].append(e0.elapsed_time(e1) / iters[name])
                        times[name]["host_issue_ms"].append(1e3 * (t1 - t0) / iters[name])
                        times[name]["wall_ms"].append(1e3 * (t2 - t0) / iters[name])
                r = {name: dict({k: {"median": statistics.median(x), "min": min(x), "max": max(x), "rounds": x} for k, x in t.items()},
                                iters_per_round=iters[name]) for name, t in times.items()}
                hip_ms, tor_ms = r["hip"]["device_ms"], r["torch"]["device_ms"]
                r["values_differing_from_the_composition"] = differing
                r["bytes"] = nbytes
                r["hip_slower_than_torch_in_any_round"] = any(h > t for h, t in zip(hip_ms["rounds"], tor_ms["rounds"]))
                r["torch_over_hip_device"] = tor_ms["median"] / hip_ms["median"]
                r["hip_over_prepare_device"] = hip_ms["median"] / r["prepare"]["device_ms"]["median"]
                r["hip_GBs"] = nbytes / (hip_ms["median"] * 1e-3) / 1e9
                r["copy_GBs"] = 2 * src.numel() / (r["copy"]["device_ms"]["median"] * 1e-3) / 1e9
                r["hip_fraction_of_copy_rate"] = r["hip_GBs"] / r["copy_GBs"]
                worst = worst or r["hip_slower_than_torch_in_any_round"]
                key = f"B{B}_crop{th}x{tw}_{recipe}"
                res["shapes"][key] = r
                line = f"{key:28s}" + "".join(f" {n} {r[n]['device_ms']['median']:.4f} ms" for n in variants)
                line += f" | hip issue {r['hip']['host_issue_ms']['median']:.4f} ms, torch/hip {r['torch_over_hip_device']:.1f}"
                line += f", hip/prepare {r['hip_over_prepare_device']:.2f}, {r['hip_GBs']:.0f} GB/s = {r['hip_fraction_of_copy_rate']:.2f} of the copy's"
                line += f" {r['copy_GBs']:.0f}; differing {sum(differing.values())}"
                print(line + (" | HIP SLOWER THAN THE COMPOSITION IN A ROUND" if r["hip_slower_than_torch_in_any_round"] else ""), flush=True)
                del src, dst
            del plain
        del raw
        torch.cuda.empty_cache()
    res["hip_slower_than_torch_in_any_round_at_any_shape"] = worst
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"bench_augment": {k: r["hip"]["device_ms"]["median"] for k, r in res["shapes"].items()},
                      "hip_slower_than_torch_in_any_round_at_any_shape": worst}))


if __name__ == "__main__":
    main()
