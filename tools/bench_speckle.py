#!/usr/bin/env python3
"""filter_speckles, measured (semstereo_amd/refine.py on csrc/disparity_speckle.hip) at 4 x 1024^2, 1 x 2048^2 and 1 x 4096^2 in one
process, the variants alternating round by round:

  hip      the four launches (tile-local union-find, merge across tile edges, fold of the counts, apply)
  torch    the same call with engine.REFINE_HIP off: the PyTorch composition on the device (label propagation with pointer jumping,
           one host wait per round)
  copy     ss_tool_copy_fwd moving as many bytes as the op must (half read, half written): the rate a streaming kernel reaches here

Inputs, each with a uint8 label (`planar`: 64 x 64 blocks; `constant`: one class), max_size 200, max_diff 1, the default outputs
("disparity", "speckle"):
  planar    a piecewise-planar map (tilted planes in blocks of 128 x 192 pixels, steps between them) with random blobs of 1 .. 500
            pixels moved by +-3 and holes (no-data columns, runs)
  constant  one value: ONE component per image, the worst case for the merge and the fold

Per input and variant: device-event time, host time to issue a call and wall time per call for every round (windows of --window-ms
of back-to-back calls), their medians, the algorithmic bytes (4 + 1 read, 4 + 1 written per pixel: what a one-pass kernel would
move; the four launches also write and read two int32 scratch planes), and for hip the bytes over the device-event time as a
fraction of the copy's rate in the same run -- a measurement, not a target.  `hip_slower_than_torch_in_every_round` is the routing
rule's input.  --out FILE keeps the whole record.

usage: python tools/bench_speckle.py [--shapes 4x1024x1024,1x2048x2048,1x4096x4096] [--rounds 7 --window-ms 100] [--only hip,copy] [--out FILE]
       python tools/bench_speckle.py --trace-table SHAPE=kernel_trace.csv [SHAPE=...]      (per-kernel medians of rocprofv3 --kernel-trace records)
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

KERNELS = ("speckle_local_k", "speckle_merge_k", "speckle_fold_k", "speckle_apply_k", "copy16_kernel")


def trace_table(pairs):
    """Per shape and kernel: calls, median and minimum dispatch duration in us from rocprofv3's kernel_trace.csv."""
    print(f"{'shape':24s} {'kernel':24s} {'calls':>6s} {'median us':>10s} {'min us':>8s}")
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
                print(f"{shape:24s} {name:24s} {len(by[name]):6d} {statistics.median(by[name]):10.2f} {min(by[name]):8.2f}")


def planar_map(torch, B, H, W, maxdisp, seed=98):
    """The `planar` input on the host: float32 [B,H,W]."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(float(H)), torch.arange(float(W)), indexing="ij")
    by, bx = -(-H // 128), -(-W // 192)
    coef = torch.rand(B, 3, by, bx, generator=g)
    up = lambda t: t.repeat_interleave(128, dim=1).repeat_interleave(192, dim=2)[:, :H, :W]          # noqa: E731
    d = (up(coef[:, 0]) - 0.5) * maxdisp + (up(coef[:, 1]) - 0.5) * 0.05 * (xx % 192) + (up(coef[:, 2]) - 0.5) * 0.05 * (yy % 128)
    blobs = max(1, B * H * W // 4000)
    for _ in range(blobs):                                              # rectangles of 1 .. 500 pixels, moved by +-3
        b, h, w = int(torch.randint(0, B, (1,), generator=g)), int(torch.randint(1, 21, (1,), generator=g)), int(torch.randint(1, 26, (1,), generator=g))
        y, x = int(torch.randint(0, H - h + 1, (1,), generator=g)), int(torch.randint(0, W - w + 1, (1,), generator=g))
        d[b, y:y + h, x:x + w] += 3.0 if torch.rand(1, generator=g) < 0.5 else -3.0
    d[:, :, 10::97] = -999.0
    d[torch.rand(B, H, -(-W // 7), generator=g).repeat_interleave(7, dim=2)[:, :, :W] < 0.02] = -999.0
    return d.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4x1024x1024,1x2048x2048,1x4096x4096")
    ap.add_argument("--maxdisp", type=int, default=64)
    ap.add_argument("--max-size", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5, help="least calls per timed window")
    ap.add_argument("--torch-iters", type=int, default=2, help="... of the composition")
    ap.add_argument("--window-ms", type=float, default=100.0, help="work per timed window")
    ap.add_argument("--only", default="hip,torch,copy", help="the variants to run")
    ap.add_argument("--inputs", default="planar,constant")
    ap.add_argument("--out", default=None, help="write the whole record to this JSON file")
    ap.add_argument("--trace-table", nargs="+", default=None, metavar="SHAPE=CSV")
    args = ap.parse_args()
    if args.trace_table:
        return trace_table(args.trace_table)

    import torch
    import semstereo_amd as sa
    from semstereo_amd._lib import call
    assert torch.cuda.is_available(), "bench_speckle.py needs the MI355X"
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

    res = {"workload": f"filter_speckles (disparity, speckle); float32 map, uint8 label, max_size {args.max_size}, max_diff 1", "maxdisp": m,
           "rounds": args.rounds, "window_ms": args.window_ms, "tile": list(sa.refine.SPECKLE_TILE), "by_shape": {}}
    for shape in args.shapes.split(","):
        B, H, W = (int(v) for v in shape.split("x"))
        n = B * H * W
        g = torch.Generator().manual_seed(97)
        label = torch.randint(0, 6, (B, -(-H // 64), -(-W // 64)), generator=g, dtype=torch.uint8)
        label = label.repeat_interleave(64, dim=1).repeat_interleave(64, dim=2)[:, :H, :W].contiguous().to(dev)
        maps = {"planar": lambda: planar_map(torch, B, H, W, m).to(dev), "constant": lambda: torch.full((B, H, W), 1.0, device=dev)}
        maps = {k: maps[k]() for k in args.inputs.split(",")}
        nbytes = n * (4 + 1) + n * (4 + 1)
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        half = nbytes // 2 // 16 * 16

        labels = {"planar": label, "constant": torch.full_like(label, 2)}

        def op(name, want=("disparity", "speckle")):
            return lambda: sa.filter_speckles(maps[name], labels[name], maxdisp=m, max_size=args.max_size, max_diff=1.0, want=want)

        ops = {name: {"hip": op(name)} for name in maps}
        for name, variants in ops.items():
            variants["torch"] = off(variants["hip"])
            variants["copy"] = lambda: call("ss_tool_copy_fwd", src.data_ptr(), dst.data_ptr(), half)
            for v in [v for v in variants if v not in only]:
                del variants[v]
        checks = {}
        for name, variants in ops.items():
            if "hip" in variants:
                a = op(name, sa.SPECKLE_KEYS)()
                checks[f"{name}_components"] = int((a["component"] == torch.arange(H * W, device=dev, dtype=torch.int32).view(1, H, W)).sum())
                checks[f"{name}_largest"] = int(a["size"].max())
                checks[f"{name}_share_removed"] = float(a["speckle"].float().mean())
                if "torch" in variants:
                    with composition():
                        b = op(name, sa.SPECKLE_KEYS)()
                    checks[f"{name}_values_differing"] = sum(int((a[k].view(torch.uint8) != b[k].view(torch.uint8)).sum()) for k in a)
                    del b
                del a
        print(f"{shape}: {checks}", flush=True)
        iters = {}
        for name, variants in ops.items():
            for v, fn in variants.items():
                for _ in range(1 if v == "torch" else 3):
                    fn()
                torch.cuda.synchronize()
                reps = 1 if v == "torch" else 5
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
                per_call_ms = 1e3 * (time.perf_counter() - t0) / reps
                iters[name, v] = int(min(max(args.window_ms / per_call_ms, args.torch_iters if v == "torch" else args.iters), 5000))
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
        rec = {"bytes": nbytes, "checks": checks, "ops": {}}
        for name, variants in times.items():
            r = {}
            for v, t in variants.items():
                r[v] = {k: {"median": statistics.median(x), "min": min(x), "max": max(x), "rounds": x} for k, x in t.items()}
                r[v]["iters_per_round"] = iters[name, v]
            line = f"{shape} {name:9s}" + "".join(f" {k} {v['device_ms']['median']:.4f} ms" for k, v in r.items())
            if "hip" in r:
                hip = r["hip"]["device_ms"]
                r["hip_GBs"] = nbytes / (hip["median"] * 1e-3) / 1e9
                line += f" | hip issue {r['hip']['host_issue_ms']['median']:.4f} ms, {r['hip_GBs']:.0f} GB/s"
                if "torch" in r:
                    tor = r["torch"]["device_ms"]
                    r["hip_slower_than_torch_in_every_round"] = all(h > t for h, t in zip(hip["rounds"], tor["rounds"]))
                    r["torch_over_hip_device"] = tor["median"] / hip["median"]
                    line += f", torch/hip {r['torch_over_hip_device']:.1f}" + (" | HIP SLOWER IN EVERY ROUND" if r["hip_slower_than_torch_in_every_round"] else "")
                if "copy" in r:
                    r["copy_GBs"] = 2 * half / (r["copy"]["device_ms"]["median"] * 1e-3) / 1e9
                    r["hip_fraction_of_copy_rate"] = r["hip_GBs"] / r["copy_GBs"]
                    line += f" = {r['hip_fraction_of_copy_rate']:.2f} of the copy's {r['copy_GBs']:.0f}"
            rec["ops"][name] = r
            print(line, flush=True)
        res["by_shape"][shape] = rec
        del maps, label, labels, src, dst, ops
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"bench_speckle": {s: {op: r[only[0]]["device_ms"]["median"] for op, r in rec["ops"].items()}
                                        for s, rec in res["by_shape"].items()}}))


if __name__ == "__main__":
    main()
