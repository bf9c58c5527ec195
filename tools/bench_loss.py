#!/usr/bin/env python3
"""The training objective, measured (main_us3d.py:199-208; models/loss.py): forward + backward of disparity + label + LRSC loss at
1024 x 1024, batch 1 and 4, three ways in one process, alternating round by round:

  hip        semstereo_amd.train_objective on csrc/loss.hip (range masks inside the kernel)
  fallback   the same call with engine.LOSS_HIP off: the PyTorch composition without boolean indexing
  user       the objective as a training script writes it without this package: boolean-mask indexing, nn.CrossEntropyLoss, softmax /
             one_hot Dice, meshgrid / gather warping -- written here from the definitions; this is what runs at the parent commit

Per variant: device-event time per call, host time to issue a call, wall time per call (median, min, max over the rounds), and for `hip`
the algorithmic bytes of the shapes and the fraction of 8 TB/s they make of the device time.  --out FILE keeps the whole record as JSON.

usage: python tools/bench_loss.py [--batches 1,4] [--height 1024 --width 1024] [--rounds 7 --iters 100] [--only hip] [--out FILE]
       rocprofv3 --kernel-trace --stats -d <dir> -- python3 tools/bench_loss.py --batches 4 --only hip --rounds 2      (per-kernel times)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TBS = 8.0


def algorithmic_bytes(B, H, W, label_bytes=8):
    """What the three kernels must move, from the shapes alone: fp32 tensors, `label_bytes` per label."""
    n, n4 = B * H * W, B * (H // 4) * (W // 4)
    disp_read = 2 * (n + n4) * 8                      # four terms: estimate + ground truth
    disp = {"fwd_read": disp_read, "bwd_read": disp_read, "bwd_write": 2 * (n + n4) * 4}
    label = {"fwd_read": n * (24 + label_bytes), "bwd_read": n * (24 + label_bytes), "bwd_write": n * 24}
    lrsc = {k: v + (n * 4 if k.endswith("read") else 0) for k, v in label.items()}
    out = {"disparity": disp, "label": label, "lrsc": lrsc}
    out["total"] = sum(sum(v.values()) for v in out.values())
    return out


def user_objective(torch, F, nn):
    """The composition a script runs today (models/loss.py's definitions, restated)."""
    def dice(logits, target, eps=1e-6):
        p = F.softmax(logits, dim=1).float()[:, :-1]
        t = F.one_hot(target.to(torch.int64), logits.shape[1]).permute(0, 3, 1, 2).float()[:, :-1]
        inter, sets = 2 * (p * t).sum(), p.sum() + t.sum()
        sets = torch.where(sets == 0, inter, sets)
        return (inter + eps) / (sets + eps)

    def objective(ests, z, zr, gt, gt4, y, maxdisp, attn):
        m, m4 = (gt < maxdisp) & (gt >= -maxdisp), (gt4 < maxdisp) & (gt4 >= -maxdisp)
        disp_loss = sum(w * F.smooth_l1_loss(e[k], g[k]) for e, g, k, w in zip(ests, (gt, gt4, gt, gt4), (m, m4, m, m4), (1.0, 0.6, 0.5, 0.3)))
        label_loss = (nn.CrossEntropyLoss(ignore_index=5)(z, y.long()) + 1 - dice(z, y)) * (1.6 if attn else 2.4)
        b, h, w = y.shape
        x = torch.arange(w, device=y.device).view(1, 1, w).expand(b, h, w)
        xs = torch.clamp(x - ests[0], min=0, max=w - 1).long()
        lrsc = nn.CrossEntropyLoss(ignore_index=-1)(zr, torch.gather(y, 2, xs).long())
        return disp_loss + label_loss + lrsc, disp_loss, label_loss, lrsc
    return objective


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--maxdisp", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--only", default=None, help="one of hip, fallback, user (profiling runs)")
    ap.add_argument("--out", default=None, help="write the whole record to this JSON file")
    args = ap.parse_args()
    H, W, md = args.height, args.width, args.maxdisp
    batches = [int(b) for b in args.batches.split(",")]
    for B in batches:
        by = algorithmic_bytes(B, H, W)
        print(f"batch {B}: algorithmic bytes {by['total'] / 1e6:.0f} MB per forward + backward "
              + ", ".join(f"{k} {sum(v.values()) / 1e6:.0f}" for k, v in by.items() if k != "total"), flush=True)

    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    import semstereo_amd as sa
    assert torch.cuda.is_available(), "bench_loss.py needs the MI355X"
    sa._lib.load()
    dev = torch.device("cuda")
    user = user_objective(torch, F, nn)

    def hip(*a):
        return sa.train_objective(*a)

    def fallback(*a):
        sa.engine.LOSS_HIP = False
        try:
            return sa.train_objective(*a)
        finally:
            sa.engine.LOSS_HIP = True
    variants = {"hip": hip, "fallback": fallback, "user": user}
    if args.only:
        variants = {args.only: variants[args.only]}
    res = {"workload": f"{H}x{W} maxdisp={md}: forward + backward of disparity (4 terms) + label + LRSC loss", "rounds": args.rounds,
           "iters_per_round": args.iters, "by_batch": {}}
    for B in batches:
        g = torch.Generator(device=dev).manual_seed(91)
        rnd = lambda *s: torch.rand(*s, generator=g, device=dev)                     # noqa: E731
        gt, gt4 = (rnd(B, H, W) * 2 - 1) * 1.25 * md, (rnd(B, H // 4, W // 4) * 2 - 1) * 1.25 * md      # the range mask keeps 80 %
        ests = [((gt if i % 2 == 0 else gt4) + 3 * (rnd(*(gt if i % 2 == 0 else gt4).shape) - 0.5)).requires_grad_(True) for i in range(4)]
        z, zr = (4 * (rnd(B, 6, H, W) - 0.5)).requires_grad_(True), (4 * (rnd(B, 6, H, W) - 0.5)).requires_grad_(True)
        y = torch.randint(0, 6, (B, H, W), generator=g, device=dev)
        leaves = ests + [z, zr]

        def call(fn):
            for t in leaves:
                t.grad = None
            out = fn(ests, z, zr, gt, gt4, y, md, False)
            out[0].backward()
            return out

        values = {}
        for name, fn in variants.items():
            for _ in range(3):
                values[name] = [float(v.detach()) for v in call(fn)]
        torch.cuda.synchronize()
        times = {name: {"device_ms": [], "host_issue_ms": [], "wall_ms": []} for name in variants}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.rounds):
            for name, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                for _ in range(args.iters):
                    call(fn)
                e1.record()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                times[name]["device_ms"].append(e0.elapsed_time(e1) / args.iters)
                times[name]["host_issue_ms"].append(1e3 * (t1 - t0) / args.iters)
                times[name]["wall_ms"].append(1e3 * (t2 - t0) / args.iters)
        rec = {"kept_by_the_mask": float(((gt < md) & (gt >= -md)).float().mean()), "bytes": algorithmic_bytes(B, H, W), "variants": {}}
        for name, t in times.items():
            v = {k: {"median": statistics.median(x), "min": min(x), "max": max(x)} for k, x in t.items()}
            v["loss_disp_label_lrsc"] = values[name]
            if name == "hip":
                v["fraction_of_8TBs"] = rec["bytes"]["total"] / (v["device_ms"]["median"] * 1e-3) / (PEAK_TBS * 1e12)
            rec["variants"][name] = v
            print(f"batch {B} {name:9s} device {v['device_ms']['median']:.3f} ms [{v['device_ms']['min']:.3f}, {v['device_ms']['max']:.3f}]  "
                  f"host issue {v['host_issue_ms']['median']:.3f} ms [{v['host_issue_ms']['min']:.3f}, {v['host_issue_ms']['max']:.3f}]  "
                  f"wall {v['wall_ms']['median']:.3f} ms [{v['wall_ms']['min']:.3f}, {v['wall_ms']['max']:.3f}]"
                  + (f"  {v['fraction_of_8TBs']:.3f} of 8 TB/s" if name == "hip" else ""), flush=True)
        res["by_batch"][str(B)] = rec
        del ests, z, zr, y, gt, gt4, leaves
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"bench_loss": {b: {n: v["device_ms"]["median"] for n, v in r["variants"].items()} for b, r in res["by_batch"].items()}}))


if __name__ == "__main__":
    main()
