#!/usr/bin/env python3
"""median_disparity, measured (semstereo_amd/refine.py on csrc/disparity_median.hip) at 4 x 1024^2, 1 x 2048^2, 16 x 1024^2 and
1 x 4096^2 in one process, the variants alternating round by round:

  hip      the kernel
  torch    the same call with engine.REFINE_HIP off: the PyTorch composition on the device ((2r + 1)^2 shifted views, one sort)
  copy     ss_tool_copy_fwd moving as many bytes as the op must (half read, half written): the rate a streaming kernel reaches here

Ops: radius 1 and 2, each with a uint8 label, with and without `where` (the `kind != 0` of the row fill), fill_holes on, the default
output ("disparity"): 4 + 1 (+ 1) bytes read and 4 written per pixel.  The input is fill_disparity's output of a smooth field plus
steps on the half-pixel grid with no-data columns and rows, the label 64 x 64 blocks.

Per op and variant: device-event time, host time to issue a call and wall time per call for every round (windows of --window-ms of
back-to-back calls), their medians, the algorithmic bytes, and for hip the bytes over the device-event time as a fraction of the copy's
rate in the same run.  The kernel works per pixel (a 19- or 99-exchange network) as well as per byte, so that fraction is a
measurement, not a target.  `hip_slower_than_torch_in_every_round` is the routing rule's input.  --out FILE keeps the whole record.

usage: python tools/bench_median.py [--shapes 4x1024x1024,1x2048x2048,16x1024x1024,1x4096x4096] [--rounds 7 --window-ms 100] [--only hip,copy] [--out FILE]
       python tools/bench_median.py --trace-table SHAPE=kernel_trace.csv [SHAPE=...]      (per-kernel medians of rocprofv3 --kernel-trace records)
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def algorithmic_bytes(B, H, W):
    """What each op must move, from the shapes alone (a float32 map and a uint8 label read, with `where` one byte more; a float32 map
    written)."""
    n = B * H * W
    return {f"r{r}{'_where' if w else ''}": n * (4 + 1 + w) + n * 4 for r in (1, 2) for w in (0, 1)}


def trace_table(pairs):
    """Per shape and kernel: calls, median and minimum dispatch duration in us from rocprofv3's kernel_trace.csv."""
    print(f"{'shape':14s} {'kernel':40s} {'calls':>6s} {'median us':>10s} {'min us':>8s}")
    for pair in pairs:
        shape, path = pair.split("=", 1)
        by = {}
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                for name in ("disparity_median_k<1>", "disparity_median_k<2>", "copy16_kernel", "disparity_refine_k"):
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
    from bench_refine import disparity_field
    assert torch.cuda.is_available(), "bench_median.py needs the MI355X"
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

    res = {"workload": "median_disparity (disparity) after fill_disparity; float32 map, uint8 label, fill_holes", "maxdisp": m,
           "rounds": args.rounds, "window_ms": args.window_ms, "by_shape": {}}
    for shape in args.shapes.split(","):
        B, H, W = (int(v) for v in shape.split("x"))
        g = torch.Generator().manual_seed(97)
        label = torch.randint(0, 6, (B, -(-H // 64), -(-W // 64)), generator=g, dtype=torch.uint8)
        label = label.repeat_interleave(64, dim=1).repeat_interleave(64, dim=2)[:, :H, :W].contiguous().to(dev)
        fill = sa.fill_disparity(disparity_field(torch, B, H, W).to(dev), label, maxdisp=m)
        disp, where = fill["disparity"], (fill["kind"] != 0).view(torch.uint8)
        by = algorithmic_bytes(B, H, W)
        src = torch.empty(max(by.values()) // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)

        def copy(nbytes):
            half = nbytes // 2 // 16 * 16
            return lambda: call("ss_tool_copy_fwd", src.data_ptr(), dst.data_ptr(), half)

        def op(r, w):
            return lambda: sa.median_disparity(disp, label, where=where if w else None, maxdisp=m, radius=r, fill_holes=True)

        ops = {name: {"hip": op(int(name[1]), name.endswith("_where"))} for name in by}
        for name, variants in ops.items():
            variants["torch"] = off(variants["hip"])
            variants["copy"] = copy(by[name])
            for v in [v for v in variants if v not in only]:
                del variants[v]
        checks = {}
        if "hip" in only and "torch" in only:
            for name, variants in ops.items():
                a, b = variants["hip"](), variants["torch"]()
                checks[f"{name}_values_differing"] = int((a["disparity"].view(torch.int32) != b["disparity"].view(torch.int32)).sum())
                checks[f"{name}_share_moved"] = float((a["disparity"].view(torch.int32) != disp.view(torch.int32)).float().mean())
                del a, b
            print(f"{shape}: hip against the composition on the device: {checks}", flush=True)
        iters = {}
        for name, variants in ops.items():
            for v, fn in variants.items():
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(5):
                    fn()
                torch.cuda.synchronize()
                per_call_ms = 1e3 * (time.perf_counter() - t0) / 5
                iters[name, v] = int(min(max(args.window_ms / per_call_ms, args.iters), 5000))
        torch.cuda.synchronize()
        times = {name: {v: {"device_ms": [], "host_issue_ms": [], "wall_ms": []} for v in variants} for name, variants in ops.items()}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.rounds):
            for name, variants in ops.items():
                for v, fn in variants.items():
                    n_it = iters[name, v]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record()
                    for _ in range(n_it):
                        fn()
                    e1.record()
                    t1 = time.perf_counter()
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    times[name][v]["device_ms"].append(e0.elapsed_time(e1) / n_it)
                    times[name][v]["host_issue_ms"].append(1e3 * (t1 - t0) / n_it)
                    times[name][v]["wall_ms"].append(1e3 * (t2 - t0) / n_it)
        rec = {"bytes": by, "checks": checks, "ops": {}}
        for name, variants in times.items():
            r = {}
            for v, t in variants.items():
                r[v] = {k: {"median": statistics.median(x), "min": min(x), "max": max(x), "rounds": x} for k, x in t.items()}
                r[v]["iters_per_round"] = iters[name, v]
            line = f"{shape} {name:10s}" + "".join(f" {n} {v['device_ms']['median']:.4f} ms" for n, v in r.items())
            if "hip" in r:
                hip = r["hip"]["device_ms"]
                r["hip_GBs"] = by[name] / (hip["median"] * 1e-3) / 1e9
                line += f" | hip issue {r['hip']['host_issue_ms']['median']:.4f} ms, {r['hip_GBs']:.0f} GB/s"
                if "torch" in r:
                    tor = r["torch"]["device_ms"]
                    r["hip_slower_than_torch_in_every_round"] = all(h > t for h, t in zip(hip["rounds"], tor["rounds"]))
                    r["torch_over_hip_device"] = tor["median"] / hip["median"]
                    line += f", torch/hip {r['torch_over_hip_device']:.1f}" + (" | HIP SLOWER IN EVERY ROUND" if r["hip_slower_than_torch_in_every_round"] else "")
                if "copy" in r:
                    r["copy_GBs"] = (by[name] // 2 // 16 * 16 * 2) / (r["copy"]["device_ms"]["median"] * 1e-3) / 1e9
                    r["hip_fraction_of_copy_rate"] = r["hip_GBs"] / r["copy_GBs"]
                    line += f" = {r['hip_fraction_of_copy_rate']:.2f} of the copy's {r['copy_GBs']:.0f}"
            rec["ops"][name] = r
            print(line, flush=True)
        res["by_shape"][shape] = rec
        del disp, label, where, fill, src, dst, ops
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"bench_median": {s: {op: r[only[0]]["device_ms"]["median"] for op, r in rec["ops"].items()}
                                       for s, rec in res["by_shape"].items()}}))


if __name__ == "__main__":
    main()
