#!/usr/bin/env python3
"""The evaluation step's metrics, measured (main_us3d.py:225-263; utils/metrics.py): EPE + D1 + Thres1 + Thres2 (+ Thres3 with --whu) of
one estimate, the confusion matrix and its scores at 1024 x 1024, batch 1 and 4 (the reference's test_batch_size), three ways in one
process, alternating round by round:

  hip        semstereo_amd.eval_metrics on csrc/metrics.hip (range mask inside the kernel), values staying on the device
  fallback   the same call with engine.METRICS_HIP off: the PyTorch composition without boolean indexing and without .cpu()
  user       what an evaluation script runs without this package, written here from the definitions: the per-image loop with the ratio
             test on the host, boolean-mask indexing, logits.cpu().numpy() + argmax + bincount (with `int` where the reference writes the
             removed `np.int`), the scores in numpy

Per variant: device-event time per call, host time to issue a call, wall time per call (median, min, max over the rounds), and for `hip`
the algorithmic bytes of the shapes and the fraction of 8 TB/s they make of the device time.  --out FILE keeps the whole record as JSON.

usage: python tools/bench_metrics.py [--batches 1,4] [--height 1024 --width 1024] [--rounds 7 --iters 50] [--whu] [--only hip] [--out FILE]
       rocprofv3 --kernel-trace --stats -d <dir> -- python3 tools/bench_metrics.py --batches 4 --only hip --rounds 2      (per-kernel times)
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


def algorithmic_bytes(B, H, W, n_est=1, mask_bytes=0, label_bytes=8):
    """What the two kernels must move, from the shapes alone."""
    n = B * H * W
    out = {"disparity": n * (4 * n_est + 4 + mask_bytes), "confusion": n * (24 + label_bytes)}
    out["total"] = out["disparity"] + out["confusion"]
    return out


def user_metrics(torch, np, thresholds):
    """The evaluation metrics as a script computes them today (utils/metrics.py's definitions, restated)."""
    def per_image(fn, est, gt, mask):
        vals = []
        for i in range(gt.shape[0]):
            if mask[i].float().mean() / (gt[i] > 0).float().mean() < 0.1:          # a host wait per image and metric
                continue
            vals.append(fn(est[i][mask[i]], gt[i][mask[i]]))                        # boolean indexing: a nonzero, another wait
        return torch.stack(vals).mean() if vals else torch.tensor(0, dtype=torch.float32, device=gt.device)

    def epe(e, g):
        return (e - g).abs().mean()

    def d1(e, g):
        err = (g - e).abs()
        return ((err > 3) & (err / g.abs() > 0.05)).float().mean()

    def thres(t):
        return lambda e, g: ((g - e).abs() > t).float().mean()

    def confusion(logits, labels, n):
        pred = np.asarray(np.argmax(logits.cpu().numpy().transpose(0, 2, 3, 1), axis=3), dtype=np.uint8)
        gt = np.asarray(labels.cpu().numpy()[:, :logits.shape[-2], :logits.shape[-1]], dtype=int)
        count = np.bincount((gt * n + pred).astype("int32").flatten(), minlength=n * n)
        return count[:n * n].reshape(n, n).astype(np.float64)

    def metrics(ests, z, gt, y, maxdisp, num_classes=6):
        mask = (gt < maxdisp) & (gt >= -maxdisp)
        out = {"D1": [per_image(d1, e, gt, mask) for e in ests], "EPE": [per_image(epe, e, gt, mask) for e in ests]}
        for t in thresholds:
            out[f"Thres{t:g}"] = [per_image(thres(t), e, gt, mask) for e in ests]
        m = confusion(z, y, num_classes - 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            diag, rows, cols = np.diag(m), m.sum(1), m.sum(0)
            cpa, iou = diag / rows, diag / (rows + cols - diag)
            out["PA"], out["MPA"], out["mIoU"] = [diag.sum() / m.sum()], [np.nanmean(cpa)], [np.nanmean(iou)]
        out2 = {}
        for i in range(num_classes - 1):
            out2["CPA" + str(i)], out2["IoU" + str(i)] = [cpa[i]], [iou[i]]
        return out, out2
    return metrics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--maxdisp", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--whu", action="store_true", help="Thres3 as well (main_whu.py)")
    ap.add_argument("--only", default=None, help="one of hip, fallback, user (profiling runs)")
    ap.add_argument("--out", default=None, help="write the whole record to this JSON file")
    args = ap.parse_args()
    H, W, md = args.height, args.width, args.maxdisp
    thresholds = (1.0, 2.0, 3.0) if args.whu else (1.0, 2.0)
    batches = [int(b) for b in args.batches.split(",")]
    for B in batches:
        by = algorithmic_bytes(B, H, W)
        print(f"batch {B}: algorithmic bytes {by['total'] / 1e6:.1f} MB per call, disparity {by['disparity'] / 1e6:.1f}, "
              f"confusion {by['confusion'] / 1e6:.1f}", flush=True)

    import numpy as np
    import torch
    import semstereo_amd as sa
    assert torch.cuda.is_available(), "bench_metrics.py needs the MI355X"
    sa._lib.load()
    dev = torch.device("cuda")
    user = user_metrics(torch, np, thresholds)

    def hip(ests, z, gt, y, m):
        return sa.eval_metrics(ests, z, gt, y, m, thresholds=thresholds)

    def fallback(ests, z, gt, y, m):
        sa.engine.METRICS_HIP = False
        try:
            return sa.eval_metrics(ests, z, gt, y, m, thresholds=thresholds)
        finally:
            sa.engine.METRICS_HIP = True
    variants = {"hip": hip, "fallback": fallback, "user": user}
    if args.only:
        variants = {args.only: variants[args.only]}
    res = {"workload": f"{H}x{W} maxdisp={md}: EPE + D1 + Thres{'1,2,3' if args.whu else '1,2'} of one estimate, confusion matrix, scores",
           "rounds": args.rounds, "iters_per_round": args.iters, "by_batch": {}}
    for B in batches:
        g = torch.Generator(device=dev).manual_seed(93)
        rnd = lambda *s: torch.rand(*s, generator=g, device=dev)                     # noqa: E731
        gt = (rnd(B, H, W) * 2 - 1) * 1.25 * md                                      # the range mask keeps 80 %
        ests = [gt + 6 * (rnd(B, H, W) - 0.5)]
        z = 4 * (rnd(B, 6, H, W) - 0.5)
        y = torch.randint(0, 6, (B, H, W), generator=g, device=dev)

        def call(fn):
            return fn(ests, z, gt, y, md)

        values = {}
        for name, fn in variants.items():
            for _ in range(3):
                out, out2 = call(fn)
            values[name] = {k: float(out[k][0]) for k in out}
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
            v["values"] = values[name]
            if name == "hip":
                v["fraction_of_8TBs"] = rec["bytes"]["total"] / (v["device_ms"]["median"] * 1e-3) / (PEAK_TBS * 1e12)
            rec["variants"][name] = v
            print(f"batch {B} {name:9s} device {v['device_ms']['median']:.3f} ms [{v['device_ms']['min']:.3f}, {v['device_ms']['max']:.3f}]  "
                  f"host issue {v['host_issue_ms']['median']:.3f} ms [{v['host_issue_ms']['min']:.3f}, {v['host_issue_ms']['max']:.3f}]  "
                  f"wall {v['wall_ms']['median']:.3f} ms [{v['wall_ms']['min']:.3f}, {v['wall_ms']['max']:.3f}]"
                  + (f"  {v['fraction_of_8TBs']:.3f} of 8 TB/s" if name == "hip" else ""), flush=True)
        if "hip" in rec["variants"]:
            for other in ("fallback", "user"):
                if other in rec["variants"]:
                    rec[f"wall_{other}_over_hip"] = rec["variants"][other]["wall_ms"]["median"] / rec["variants"]["hip"]["wall_ms"]["median"]
                    print(f"batch {B} wall {other} / hip = {rec[f'wall_{other}_over_hip']:.2f}", flush=True)
        res["by_batch"][str(B)] = rec
        del ests, z, y, gt
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"bench_metrics": {b: {n: v["wall_ms"]["median"] for n, v in r["variants"].items()} for b, r in res["by_batch"].items()}}))


if __name__ == "__main__":
    main()
