#!/usr/bin/env python3
"""fill_disparity(axes="both"), measured (semstereo_amd/refine.py on csrc/disparity_fill2d.hip) at 4 x 1024^2, 1 x 2048^2, 16 x 1024^2
and 1 x 4096^2 in one process, the variants alternating round by round:

  both     the four launches of the two-axis fill
  torch    the same call with engine.REFINE_HIP off: the PyTorch composition on the device (per class a cummax and a cummin along both
           axes, gathers on the flattened image)
  rows     the axes="rows" call in the same run (csrc/disparity_refine.hip, one launch): what the second axis costs
  copy     ss_tool_copy_fwd moving the bytes a ONE-PASS kernel would move -- the inputs read once (4 + 1 bytes per pixel), the outputs
           written once (4 + 1): the rate a streaming kernel reaches here

The op is fill_disparity with a uint8 label and the default outputs ("disparity", "kind") on the blob fixture of tests/fill2d_cases.py
(blob_batch's recipe at any shape): a smooth field plus steps on the half-pixel grid, 12 x 12 hole blobs, rows without a source, one
600 x 610 hole in image 0, a label of 64 x 64 blocks.

Per variant: device-event time, host time to issue a call and wall time per call for every round (windows of --window-ms of
back-to-back calls), their medians; for `both` the algorithmic bytes over the device-event time as a fraction of the copy's rate in
the same run, and `both_slower_than_torch_in_every_round`, the routing rule's input.  `values_differing` counts the values in which
the kernels and the composition differ (it must be 0).  SS_TOOL_LIB=FILE runs on another build of the library (an A/B of the rows
call against the parent commit's row kernel: --only rows).  --out FILE keeps the whole record as JSON.

usage: python tools/bench_fill2d.py [--shapes 4x1024x1024,...] [--rounds 7 --window-ms 100] [--only both,rows,copy] [--out FILE]
       python tools/bench_fill2d.py --trace-table SHAPE=kernel_trace.csv [SHAPE=...]      (per-kernel medians of rocprofv3 --kernel-trace records)
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
KERNELS = ("fill2d_classify_k", "fill2d_scan_k", "fill2d_sweep_k", "fill2d_rows_k", "disparity_refine_k", "copy16_kernel")


def blob_field(torch, B, H, W):
    """tests/fill2d_cases.py: blob_batch's disparity at any shape."""
    yy, xx = torch.meshgrid(torch.arange(float(H)), torch.arange(float(W)), indexing="ij")
    maps = []
    for b in range(B):
        smooth = 20 * torch.sin(xx / (37.0 + 9 * (b % 4))) * torch.cos(yy / 61.0) + 0.01 * (b % 4 + 1) * xx * 1024 / W
        steps = 14.0 * ((xx // (96 + 32 * (b % 4))) % 3) - 14.0
        maps.append(torch.round(2 * (smooth + steps)) / 2)
    d = torch.stack(maps)
    yi, xi = yy.long(), xx.long()
    d[:, ((xi // 12 + 2 * (yi // 12)) % 7 == 0) | (((xi // 40) % 9 == 3) & ((yi // 24) % 2 == 0))] = -999.0
    d[:, 7::113] = -999.0
    d[0, 200:800, 200:810] = -999.0
    return d


def trace_table(pairs):
    """Per shape and kernel: calls, median and minimum dispatch duration in us from rocprofv3's kernel_trace.csv."""
    print(f"{'shape':14s} {'kernel':24s} {'calls':>6s} {'median us':>10s} {'min us':>8s}")
    for pair in pairs:
        shape, path = pair.split("=", 1)
        by = {}
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                for name in KERNELS:
                    if name in row["Kernel_Name"]:
                        by.setdefault(name, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        for name in KERNELS:
            if by.get(name):
                print(f"{shape:14s} {name:24s} {len(by[name]):6d} {statistics.median(by[name]):10.2f} {min(by[name]):8.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4x1024x1024,1x2048x2048,16x1024x1024,1x4096x4096")
    ap.add_argument("--maxdisp", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5, help="least calls per timed window")
    ap.add_argument("--window-ms", type=float, default=100.0, help="work per timed window")
    ap.add_argument("--only", default="both,torch,rows,copy", help="the variants to run")
    ap.add_argument("--out", default=None, help="write the whole record to this JSON file")
    ap.add_argument("--trace-table", nargs="+", default=None, metavar="SHAPE=CSV")
    args = ap.parse_args()
    if args.trace_table:
        return trace_table(args.trace_table)

    import torch
    import semstereo_amd as sa
    from semstereo_amd._lib import call
    if os.environ.get("SS_TOOL_LIB"):
        sa._lib.LIB_PATH = os.path.abspath(os.environ["SS_TOOL_LIB"])
    assert torch.cuda.is_available(), "bench_fill2d.py needs the MI355X"
    sa._lib.load()
    dev, m, only = torch.device("cuda"), args.maxdisp, args.only.split(",")

    def composition(fn):
        def wrapper():
            sa.engine.REFINE_HIP = False
            try:
                return fn()
            finally:
                sa.engine.REFINE_HIP = True
        return wrapper

    res = {"workload": 'fill_disparity (disparity, kind), axes="both" and "rows"; float32 disparity, uint8 label, the blob fixture',
           "library": os.path.basename(sa._lib.LIB_PATH), "maxdisp": m, "rounds": args.rounds, "window_ms": args.window_ms, "by_shape": {}}
    for shape in args.shapes.split(","):
        B, H, W = (int(v) for v in shape.split("x"))
        disp = blob_field(torch, B, H, W).to(dev)
        g = torch.Generator().manual_seed(9700)
        label = torch.randint(0, 6, (B, -(-H // 64), -(-W // 64)), generator=g, dtype=torch.uint8)
        label = label.repeat_interleave(64, dim=1).repeat_interleave(64, dim=2)[:, :H, :W].contiguous()
        label[:, :, 5::29] = 200
        label = label.to(dev)
        n = B * H * W
        nbytes = n * (4 + 1) + n * (4 + 1)
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        half = nbytes // 2 // 16 * 16
        variants = {"both": lambda: sa.fill_disparity(disp, label, maxdisp=m, axes="both")}
        variants["torch"] = composition(variants["both"])
        variants["rows"] = lambda: sa.fill_disparity(disp, label, maxdisp=m)
        variants["copy"] = lambda: call("ss_tool_copy_fwd", src.data_ptr(), dst.data_ptr(), half)
        for v in [v for v in variants if v not in only]:
            del variants[v]
        checks = {}
        if "both" in only and "torch" in only:
            keys = ("disparity", "kind", "source", "source_row")
            a = sa.fill_disparity(disp, label, maxdisp=m, axes="both", want=keys)
            b = composition(lambda: sa.fill_disparity(disp, label, maxdisp=m, axes="both", want=keys))()
            checks["values_differing"] = {k: int((a[k].view(torch.uint8) != b[k].view(torch.uint8)).sum()) for k in keys}
            checks["kind_shares"] = [float((a["kind"] == k).float().mean()) for k in range(4)]
            if "rows" in only:
                checks["kind_shares_rows"] = [float((variants["rows"]()["kind"] == k).float().mean()) for k in range(4)]
            print(f"{shape}: the kernels against the composition on the device: {checks}", flush=True)
            del a, b
        iters = {}
        for name, fn in variants.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            iters[name] = int(min(max(args.window_ms / (1e3 * (time.perf_counter() - t0) / 5), args.iters), 5000))
        times = {v: {"device_ms": [], "host_issue_ms": [], "wall_ms": []} for v in variants}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.rounds):
            for name, fn in variants.items():
                n_it = iters[name]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                for _ in range(n_it):
                    fn()
                e1.record()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                times[name]["device_ms"].append(e0.elapsed_time(e1) / n_it)
                times[name]["host_issue_ms"].append(1e3 * (t1 - t0) / n_it)
                times[name]["wall_ms"].append(1e3 * (t2 - t0) / n_it)
        r = {}
        for name, t in times.items():
            r[name] = {k: {"median": statistics.median(x), "min": min(x), "max": max(x), "rounds": x} for k, x in t.items()}
            r[name]["iters_per_round"] = iters[name]
        line = f"{shape}" + "".join(f" {k} {v['device_ms']['median']:.4f} ms" for k, v in r.items())
        if "both" in r:
            both = r["both"]["device_ms"]
            r["both_GBs"] = nbytes / (both["median"] * 1e-3) / 1e9
            line += f" | both issue {r['both']['host_issue_ms']['median']:.4f} ms, {r['both_GBs']:.0f} GB/s"
            if "torch" in r:
                tor = r["torch"]["device_ms"]
                r["both_slower_than_torch_in_every_round"] = all(h > t for h, t in zip(both["rounds"], tor["rounds"]))
                r["torch_over_both_device"] = tor["median"] / both["median"]
                line += f", torch/both {r['torch_over_both_device']:.1f}" + (" | KERNELS SLOWER IN EVERY ROUND" if r["both_slower_than_torch_in_every_round"] else "")
            if "rows" in r:
                r["both_over_rows_device"] = both["median"] / r["rows"]["device_ms"]["median"]
                line += f", both/rows {r['both_over_rows_device']:.2f}"
            if "copy" in r:
                r["copy_GBs"] = 2 * half / (r["copy"]["device_ms"]["median"] * 1e-3) / 1e9
                r["both_fraction_of_copy_rate"] = r["both_GBs"] / r["copy_GBs"]
                line += f" = {r['both_fraction_of_copy_rate']:.2f} of the copy's {r['copy_GBs']:.0f}"
                if "rows" in r:
                    r["rows_fraction_of_copy_rate"] = nbytes / (r["rows"]["device_ms"]["median"] * 1e-3) / 1e9 / r["copy_GBs"]
        print(line, flush=True)
        res["by_shape"][shape] = {"bytes": nbytes, "checks": checks, "variants": r}
        del disp, label, src, dst, variants
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"bench_fill2d": {s: {k: v["device_ms"]["median"] for k, v in rec["variants"].items() if isinstance(v, dict) and "device_ms" in v}
                                       for s, rec in res["by_shape"].items()}}))


if __name__ == "__main__":
    main()
