#!/usr/bin/env python3
"""right_view and lr_consistency, measured (semstereo_amd/data.py on csrc/right_view.hip) at 4 x 1024^2, 1 x 1024^2 and 1 x 2048^2 -- and at
16 x 1024^2, the one shape whose kernels outlast the host's issue of a call -- in one process, the variants alternating round by round:

  hip      the kernel
  torch    the same call with engine.DATA_HIP off: the PyTorch composition on the device (scatter_reduce_ 'amax' and two gathers)
  copy     ss_tool_copy_fwd moving as many bytes as the op must (half read, half written): the rate a streaming kernel reaches here

Ops: right_view (all three outputs from a float32 disparity and a uint8 label: 4 + 1 bytes read and 4 + 4 + 1 written per pixel),
lr_consistency (the bool map: 8 read, 1 written) and lr_consistency_diff (with the differences: 8 read, 5 written).  The disparity is a
smooth field plus steps on the half-pixel grid with no-data columns, so targets collide as they do on real ground truth.

Per op and variant: device-event time, host time to issue a call and wall time per call for every round (windows of --window-ms of
back-to-back calls), their medians, the algorithmic bytes, and for hip the bytes over the device-event time as a fraction of the copy's
rate in the same run -- for right_view that is the rate the LDS integer maximum sustains.  The device-event time of back-to-back calls
is the larger of the kernels' time and the host's issue time: where `host_issue_ms` is as large, the figure is the launch path's, not
the kernel's.  `hip_slower_than_torch_in_every_round` is the routing rule's input.  --out FILE keeps the whole record as JSON.

usage: python tools/bench_right_view.py [--shapes 4x1024x1024,1x1024x1024,1x2048x2048,16x1024x1024] [--rounds 7 --window-ms 100] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def algorithmic_bytes(B, H, W):
    """What each op must move, from the shapes alone (float32 disparities, a uint8 label, float32 and one-byte results)."""
    n = B * H * W
    return {"right_view": n * (4 + 1) + n * (4 + 4 + 1), "lr_consistency": n * 8 + n, "lr_consistency_diff": n * 8 + n * 5}


def disparity_field(torch, B, H, W):
    yy, xx = torch.meshgrid(torch.arange(float(H)), torch.arange(float(W)), indexing="ij")
    maps = []
    for b in range(B):
        smooth = 20 * torch.sin(xx / (37.0 + 9 * b)) * torch.cos(yy / 61.0) + 0.01 * (b + 1) * xx * 1024 / W
        steps = 14.0 * ((xx // (96 + 32 * b)) % 3) - 14.0
        maps.append(torch.round(2 * (smooth + steps)) / 2)
    d = torch.stack(maps)
    d[:, :, 10::11] = -999.0
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4x1024x1024,1x1024x1024,1x2048x2048,16x1024x1024")
    ap.add_argument("--maxdisp", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40, help="least calls per timed window")
    ap.add_argument("--window-ms", type=float, default=100.0, help="work per timed window")
    ap.add_argument("--out", default=None, help="write the whole record to this JSON file")
    args = ap.parse_args()

    import torch
    import semstereo_amd as sa
    from semstereo_amd._lib import call
    assert torch.cuda.is_available(), "bench_right_view.py needs the MI355X"
    sa._lib.load()
    D, dev, m = sa.data, torch.device("cuda"), args.maxdisp

    class composition:
        def __enter__(self):
            sa.engine.DATA_HIP = False

        def __exit__(self, *exc):
            sa.engine.DATA_HIP = True

    def off(fn):
        def wrapper():
            with composition():
                return fn()
        return wrapper

    res = {"workload": "right_view (right_disparity, right_label, left_visible) and lr_consistency; float32 disparity, uint8 label",
           "maxdisp": m, "rounds": args.rounds, "window_ms": args.window_ms, "by_shape": {}}
    for shape in args.shapes.split(","):
        B, H, W = (int(v) for v in shape.split("x"))
        disp = disparity_field(torch, B, H, W).to(dev)
        label = torch.randint(0, 6, (B, H, W), generator=torch.Generator().manual_seed(97), dtype=torch.uint8).to(dev)
        right = D.right_view(disp, maxdisp=m, want=("right_disparity",))["right_disparity"]
        by = algorithmic_bytes(B, H, W)
        src = torch.empty(max(by.values()) // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)

        def copy(nbytes):
            half = nbytes // 2 // 16 * 16
            return lambda: call("ss_tool_copy_fwd", src.data_ptr(), dst.data_ptr(), half)

        ops = {
            "right_view": {"hip": lambda: D.right_view(disp, label, maxdisp=m)},
            "lr_consistency": {"hip": lambda: D.lr_consistency(disp, right, 1.0, maxdisp=m)},
            "lr_consistency_diff": {"hip": lambda: D.lr_consistency(disp, right, 1.0, maxdisp=m, return_diff=True)},
        }
        for name, variants in ops.items():
            variants["torch"] = off(variants["hip"])
            variants["copy"] = copy(by[name])
        a, b = ops["right_view"]["hip"](), ops["right_view"]["torch"]()
        checks = {f"{k}_values_differing": int((a[k] != b[k]).sum()) for k in a}
        p, q = ops["lr_consistency_diff"]["hip"](), ops["lr_consistency_diff"]["torch"]()
        checks["consistent_values_differing"] = int((p[0] != q[0]).sum())
        checks["diff_values_differing"] = int((p[1] != q[1]).sum())
        checks["visible_share"] = float(a["left_visible"].float().mean())
        print(f"{shape}: hip against the composition on the device: {checks}", flush=True)
        iters = {}
        for op, variants in ops.items():
            for name, fn in variants.items():
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(10):
                    fn()
                torch.cuda.synchronize()
                per_call_ms = 1e3 * (time.perf_counter() - t0) / 10
                iters[op, name] = int(min(max(args.window_ms / per_call_ms, args.iters), 5000))
        torch.cuda.synchronize()
        times = {op: {v: {"device_ms": [], "host_issue_ms": [], "wall_ms": []} for v in variants} for op, variants in ops.items()}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.rounds):
            for op, variants in ops.items():
                for name, fn in variants.items():
                    n_it = iters[op, name]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record()
                    for _ in range(n_it):
                        fn()
                    e1.record()
                    t1 = time.perf_counter()
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    times[op][name]["device_ms"].append(e0.elapsed_time(e1) / n_it)
                    times[op][name]["host_issue_ms"].append(1e3 * (t1 - t0) / n_it)
                    times[op][name]["wall_ms"].append(1e3 * (t2 - t0) / n_it)
        rec = {"bytes": by, "checks": checks, "ops": {}}
        for op, variants in times.items():
            r = {}
            for name, t in variants.items():
                r[name] = {k: {"median": statistics.median(x), "min": min(x), "max": max(x), "rounds": x} for k, x in t.items()}
                r[name]["iters_per_round"] = iters[op, name]
            hip, tor = r["hip"]["device_ms"], r["torch"]["device_ms"]
            r["hip_slower_than_torch_in_every_round"] = all(h > t for h, t in zip(hip["rounds"], tor["rounds"]))
            r["torch_over_hip_device"] = tor["median"] / hip["median"]
            r["hip_GBs"] = by[op] / (hip["median"] * 1e-3) / 1e9
            r["copy_GBs"] = (by[op] // 2 // 16 * 16 * 2) / (r["copy"]["device_ms"]["median"] * 1e-3) / 1e9
            r["hip_fraction_of_copy_rate"] = r["hip_GBs"] / r["copy_GBs"]
            rec["ops"][op] = r
            line = f"{shape} {op:20s}" + "".join(f" {n} {v['device_ms']['median']:.4f} ms" for n, v in r.items() if isinstance(v, dict))
            line += f" | hip issue {r['hip']['host_issue_ms']['median']:.4f} ms, torch/hip {r['torch_over_hip_device']:.2f}"
            line += f", {r['hip_GBs']:.0f} GB/s = {r['hip_fraction_of_copy_rate']:.2f} of the copy's {r['copy_GBs']:.0f}"
            print(line + (" | HIP SLOWER IN EVERY ROUND" if r["hip_slower_than_torch_in_every_round"] else ""), flush=True)
        res["by_shape"][shape] = rec
        del disp, label, right, src, dst, ops
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"bench_right_view": {s: {op: r["hip"]["device_ms"]["median"] for op, r in rec["ops"].items()}
                                           for s, rec in res["by_shape"].items()}}))


if __name__ == "__main__":
    main()
