#!/usr/bin/env python3
"""fill_disparity and refine_disparity, measured (semstereo_amd/refine.py on csrc/disparity_refine.hip) at 4 x 1024^2, 1 x 2048^2,
16 x 1024^2 and 1 x 4096^2 (a mosaic: W = 4096, so a thread's chunk is 16 columns) in one process, the variants alternating round by
round:

  hip      the kernel
  torch    the same call with engine.REFINE_HIP off: the PyTorch composition on the device (per class a cummax and a cummin, gathers)
  copy     ss_tool_copy_fwd moving as many bytes as the op must (half read, half written): the rate a streaming kernel reaches here

Ops, both with a uint8 label and the default outputs ("disparity", "kind"): fill_disparity (4 + 1 bytes read and 4 + 1 written per
pixel) and refine_disparity (4 + 4 + 1 read, 4 + 1 written).  The disparity is a smooth field plus steps on the half-pixel grid with
no-data columns and rows, the right map its own right view with every third column half a pixel off, the label 64 x 64 blocks.

Per op and variant: device-event time, host time to issue a call and wall time per call for every round (windows of --window-ms of
back-to-back calls), their medians, the algorithmic bytes, and for hip the bytes over the device-event time as a fraction of the copy's
rate in the same run.  The device-event time of back-to-back calls is the larger of the kernel's time and the host's issue time: where
`host_issue_ms` is as large, the figure is the launch path's, not the kernel's -- the kernel's own time is in the kernel trace
(--trace-table).  `hip_slower_than_torch_in_every_round` is the routing rule's input.  --out FILE keeps the whole record as JSON.

usage: python tools/bench_refine.py [--shapes 4x1024x1024,1x2048x2048,16x1024x1024,1x4096x4096] [--rounds 7 --window-ms 100] [--only hip,copy] [--out FILE]
       python tools/bench_refine.py --trace-table SHAPE=kernel_trace.csv [SHAPE=...]      (per-kernel medians of rocprofv3 --kernel-trace records)
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def algorithmic_bytes(B, H, W):
    """What each op must move, from the shapes alone (float32 disparities, a uint8 label, a float32 and a one-byte result)."""
    n = B * H * W
    return {"fill_disparity": n * (4 + 1) + n * (4 + 1), "refine_disparity": n * (4 + 4 + 1) + n * (4 + 1)}


def disparity_field(torch, B, H, W):
    yy, xx = torch.meshgrid(torch.arange(float(H)), torch.arange(float(W)), indexing="ij")
    maps = []
    for b in range(B):
        smooth = 20 * torch.sin(xx / (37.0 + 9 * b)) * torch.cos(yy / 61.0) + 0.01 * (b + 1) * xx * 1024 / W
        steps = 14.0 * ((xx // (96 + 32 * b)) % 3) - 14.0
        maps.append(torch.round(2 * (smooth + steps)) / 2)
    d = torch.stack(maps)
    d[:, :, 10::11] = -999.0
    d[:, 7::113] = -999.0
    return d


def trace_table(pairs):
    """Per shape and kernel: calls, median and minimum dispatch duration in us from rocprofv3's kernel_trace.csv."""
    print(f"{'shape':14s} {'kernel':40s} {'calls':>6s} {'median us':>10s} {'min us':>8s}")
    for pair in pairs:
        shape, path = pair.split("=", 1)
        by = {}
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                for name in ("disparity_refine_k", "copy16_kernel", "right_view_k"):
                    if name in row["Kernel_Name"]:
                        by.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        for name in sorted(by):
            if by[name]:
                print(f"{shape:14s} {name:40s} {len(by[name]):6d} {statistics.median(by[name]):10.2f} {min(by[name]):8.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4x1024x1024,1x2048x2048,16x1024x1024,1x4096x4096")
    ap.add_argument("--maxdisp", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5, help="least calls per timed window")
    ap.add_argument("--window-ms", type=float, default=100.0, help="work per timed window")
    ap.add_argument("--only", default="hip,torch,copy", help="the variants to run")
    ap.add_argument("--out", default=None, help="write the whole record to this JSON file")
    ap.add_argument("--trace-table", nargs="+", default=None, metavar="SHAPE=CSV")
    args = ap.parse_args()
    if args.trace_table:
        return trace_table(args.trace_table)

    import torch
    import semstereo_amd as sa
    from semstereo_amd._lib import call
    assert torch.cuda.is_available(), "bench_refine.py needs the MI355X"
    sa._lib.load()
    dev, m, only = torch.device("cuda"), args.maxdisp, args.only.split(",")

    class composition:
        def __enter__(self):
            sa.engine.REFINE_HIP = False

        def __exit__(self, *exc):
            sa.engine.REFINE_HIP = True

    def off(fn):
        def wrapper():
            with composition():
                return fn()
        return wrapper

    res = {"workload": "fill_disparity and refine_disparity (disparity, kind); float32 disparities, uint8 label", "maxdisp": m,
           "threshold": 0.25, "rounds": args.rounds, "window_ms": args.window_ms, "by_shape": {}}
    for shape in args.shapes.split(","):
        B, H, W = (int(v) for v in shape.split("x"))
        disp = disparity_field(torch, B, H, W).to(dev)
        g = torch.Generator().manual_seed(97)
        label = torch.randint(0, 6, (B, -(-H // 64), -(-W // 64)), generator=g, dtype=torch.uint8)
        label = label.repeat_interleave(64, dim=1).repeat_interleave(64, dim=2)[:, :H, :W].contiguous().to(dev)
        right = sa.right_view(disp, maxdisp=m, want=("right_disparity",))["right_disparity"] + 0.5 * (torch.arange(W, device=dev) % 3 == 0)
        by = algorithmic_bytes(B, H, W)
        src = torch.empty(max(by.values()) // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)

        def copy(nbytes):
            half = nbytes // 2 // 16 * 16
            return lambda: call("ss_tool_copy_fwd", src.data_ptr(), dst.data_ptr(), half)

        ops = {
            "fill_disparity": {"hip": lambda: sa.fill_disparity(disp, label, maxdisp=m)},
            "refine_disparity": {"hip": lambda: sa.refine_disparity(disp, right, label, threshold=0.25, maxdisp=m)},
        }
        for name, variants in ops.items():
            variants["torch"] = off(variants["hip"])
            variants["copy"] = copy(by[name])
            for v in [v for v in variants if v not in only]:
                del variants[v]
        checks = {}
        if "hip" in only and "torch" in only:
            for name, variants in ops.items():
                a, b = variants["hip"](), variants["torch"]()
                checks.update({f"{name}_{k}_values_differing": int((a[k].view(torch.uint8) != b[k].view(torch.uint8)).sum()) for k in a})
            kind = ops["refine_disparity"]["hip"]()["kind"]
            checks["refine_kind_shares"] = [float((kind == k).float().mean()) for k in range(4)]
            print(f"{shape}: hip against the composition on the device: {checks}", flush=True)
        iters = {}
        for op, variants in ops.items():
            for name, fn in variants.items():
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(5):
                    fn()
                torch.cuda.synchronize()
                per_call_ms = 1e3 * (time.perf_counter() - t0) / 5
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
            line = f"{shape} {op:18s}" + "".join(f" {n} {v['device_ms']['median']:.4f} ms" for n, v in r.items())
            if "hip" in r:
                hip = r["hip"]["device_ms"]
                r["hip_GBs"] = by[op] / (hip["median"] * 1e-3) / 1e9
                line += f" | hip issue {r['hip']['host_issue_ms']['median']:.4f} ms, {r['hip_GBs']:.0f} GB/s"
                if "torch" in r:
                    tor = r["torch"]["device_ms"]
                    r["hip_slower_than_torch_in_every_round"] = all(h > t for h, t in zip(hip["rounds"], tor["rounds"]))
                    r["torch_over_hip_device"] = tor["median"] / hip["median"]
                    line += f", torch/hip {r['torch_over_hip_device']:.1f}" + (" | HIP SLOWER IN EVERY ROUND" if r["hip_slower_than_torch_in_every_round"] else "")
                if "copy" in r:
                    r["copy_GBs"] = (by[op] // 2 // 16 * 16 * 2) / (r["copy"]["device_ms"]["median"] * 1e-3) / 1e9
                    r["hip_fraction_of_copy_rate"] = r["hip_GBs"] / r["copy_GBs"]
                    line += f" = {r['hip_fraction_of_copy_rate']:.2f} of the copy's {r['copy_GBs']:.0f}"
            rec["ops"][op] = r
            print(line, flush=True)
        res["by_shape"][shape] = rec
        del disp, label, right, src, dst, ops
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"bench_refine": {s: {op: r[only[0]]["device_ms"]["median"] for op, r in rec["ops"].items()}
                                       for s, rec in res["by_shape"].items()}}))


if __name__ == "__main__":
    main()
