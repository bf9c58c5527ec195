#!/usr/bin/env python3
"""The joint stereo-semantic record, measured: the per-image record of one and of four estimates (range mask, int64 labels, six logits)
at 1024 x 1024 with batch 1 and 4 and at 2048 x 2048 with batch 1, four ways in one process, alternating round by round:

  hip      semstereo_amd.joint_metrics.joint_metrics on csrc/joint_metrics.hip: one launch plus its finish
  torch    the same call with engine.JOINT_METRICS_HIP off: the PyTorch composition on the device (no boolean indexing, no .cpu())
  today    what a user writes without it: the class map and six boolean masks mask & (label == c), six
           disparity_metrics(..., mask_img=...) calls on csrc/metrics.hip and SegmentationMetric.addBatch -- the per-class table only;
           the gated confusion matrix has no such spelling
  copy     ss_tool_copy_fwd moving as many bytes as the record must read (half read, half written): the rate a streaming kernel reaches here

Per shape, estimate count and variant: device-event time, host time to issue a call and wall time per call (median, min, max over the
rounds); for `hip` the algorithmic bytes, their rate, and that rate as a fraction of the copy's in the same run.  --out FILE keeps the
whole record as JSON.

usage: python tools/bench_joint_metrics.py [--shapes 1x1024x1024,4x1024x1024,1x2048x2048] [--ests 1,4] [--rounds 7 --iters 30] [--only hip]
                                           [--out FILE]
       rocprofv3 --kernel-trace --stats -d <dir> -- python3 tools/bench_joint_metrics.py --only hip --rounds 2      (per-kernel times)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def algorithmic_bytes(B, H, W, n_est, label_bytes=8):
    """What the kernel must read, from the shapes alone (range mask: no mask tensor; the record it writes is a few KB)."""
    return B * H * W * (4 * n_est + 4 + 24 + label_bytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x1024x1024,4x1024x1024,1x2048x2048")
    ap.add_argument("--ests", default="1,4")
    ap.add_argument("--maxdisp", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--only", default=None, help="one of hip, torch, today, copy (profiling runs)")
    ap.add_argument("--out", default=None, help="write the whole record to this JSON file")
    args = ap.parse_args()
    md = args.maxdisp
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    n_ests = [int(v) for v in args.ests.split(",")]

    import torch
    import semstereo_amd as sa
    from semstereo_amd._lib import call
    assert torch.cuda.is_available(), "bench_joint_metrics.py needs the MI355X"
    sa._lib.load()
    dev = torch.device("cuda")
    J = sa.joint_metrics.joint_metrics
    res = {"workload": f"joint record, range mask maxdisp={md}, int64 labels, thresholds (1, 2), tau 3", "rounds": args.rounds,
           "iters_per_round": args.iters, "cases": {}}
    for B, H, W in shapes:
        g = torch.Generator(device=dev).manual_seed(93)
        rnd = lambda *s: torch.rand(*s, generator=g, device=dev)                     # noqa: E731
        gt = (rnd(B, H, W) * 2 - 1) * 1.25 * md                                      # the range mask keeps 80 %
        all_ests = [gt + 6 * (rnd(B, H, W) - 0.5) for _ in range(max(n_ests))]
        z = 4 * (rnd(B, 6, H, W) - 0.5)
        y = torch.randint(0, 6, (B, H, W), generator=g, device=dev)
        src = torch.empty(algorithmic_bytes(B, H, W, max(n_ests)) // 2 // 16 * 16, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        for n_est in n_ests:
            ests = all_ests[:n_est]
            nbytes = algorithmic_bytes(B, H, W, n_est)

            def hip():
                return J(ests, z, gt, y, maxdisp=md)

            def composition():
                sa.engine.JOINT_METRICS_HIP = False
                try:
                    return J(ests, z, gt, y, maxdisp=md)
                finally:
                    sa.engine.JOINT_METRICS_HIP = True

            def today():
                mask = (gt < md) & (gt >= -md)
                inside = (y >= 0) & (y < 6)
                cls = torch.where(inside, y, torch.full_like(y, 6))
                out = [sa.disparity_metrics(ests, gt, mask=mask, mask_img=mask & (cls == c), return_record=True) for c in range(6)]
                m = sa.SegmentationMetric(5, fold=False)
                m.addBatch(z, y)
                return out, m

            def copy():
                call("ss_tool_copy_fwd", src.data_ptr(), dst.data_ptr(), nbytes // 2 // 16 * 16)
            variants = {"hip": hip, "torch": composition, "today": today, "copy": copy}
            if args.only:
                variants = {args.only: variants[args.only]}
            for fn in variants.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {name: {"device_ms": [], "host_issue_ms": [], "wall_ms": []} for name in variants}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(args.rounds):
                for name, fn in variants.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record()
                    for _ in range(args.iters):
                        fn()
                    e1.record()
                    t1 = time.perf_counter()
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    times[name]["device_ms"].append(e0.elapsed_time(e1) / args.iters)
                    times[name]["host_issue_ms"].append(1e3 * (t1 - t0) / args.iters)
                    times[name]["wall_ms"].append(1e3 * (t2 - t0) / args.iters)
            key = f"{B}x{H}x{W}/est{n_est}"
            rec = {"bytes": nbytes, "variants": {}}
            for name, t in times.items():
                v = {k: {"median": statistics.median(x), "min": min(x), "max": max(x)} for k, x in t.items()}
                v["rounds_wall_ms"] = t["wall_ms"]
                if name in ("hip", "copy"):
                    v["TB_per_s"] = nbytes / (v["device_ms"]["median"] * 1e-3) / 1e12
                rec["variants"][name] = v
                print(f"{key:22s} {name:6s} device {v['device_ms']['median']:.3f} ms [{v['device_ms']['min']:.3f}, {v['device_ms']['max']:.3f}]  "
                      f"host issue {v['host_issue_ms']['median']:.3f} ms  wall {v['wall_ms']['median']:.3f} ms "
                      f"[{v['wall_ms']['min']:.3f}, {v['wall_ms']['max']:.3f}]" + (f"  {v['TB_per_s']:.2f} TB/s" if "TB_per_s" in v else ""), flush=True)
            V = rec["variants"]
            if "hip" in V and "copy" in V:
                rec["hip_fraction_of_copy_rate"] = V["hip"]["TB_per_s"] / V["copy"]["TB_per_s"]
                # (a window of back-to-back calls: where the host needs as long to issue a call as the device to run it, the host sets the pace)
                rec["hip_bound_by"] = "host issue" if V["hip"]["host_issue_ms"]["median"] >= 0.9 * V["hip"]["device_ms"]["median"] else "device"
                print(f"{key:22s} hip at {rec['hip_fraction_of_copy_rate']:.2f} of the copy's rate; a call is bound by its {rec['hip_bound_by']} time",
                      flush=True)
            for other in ("torch", "today"):
                if "hip" in V and other in V:
                    rec[f"hip_slower_than_{other}_in_every_round"] = all(h > o for h, o in zip(times["hip"]["wall_ms"], times[other]["wall_ms"]))
                    rec[f"hip_slower_than_{other}_in_any_round"] = any(h > o for h, o in zip(times["hip"]["wall_ms"], times[other]["wall_ms"]))
                    rec[f"wall_{other}_over_hip"] = V[other]["wall_ms"]["median"] / V["hip"]["wall_ms"]["median"]
                    print(f"{key:22s} wall {other} / hip = {rec[f'wall_{other}_over_hip']:.2f}", flush=True)
            res["cases"][key] = rec
        del all_ests, z, y, gt, src, dst
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"bench_joint_metrics": {k: {n: v["wall_ms"]["median"] for n, v in r["variants"].items()} for k, r in res["cases"].items()}}))


if __name__ == "__main__":
    main()
