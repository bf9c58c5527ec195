#!/usr/bin/env python3
"""Scene inference, measured (semstereo_amd/scene.py on csrc/scene_tiles.hip): a 4096^2 scene, 1024^2 tiles, overlap 256 (25 tiles, 5
tile rows), C = 6 logit channels -- in one process, the variants alternating round by round:

  hip      the kernel
  torch    the same call with engine.SCENE_HIP off: the PyTorch composition on the device (slices, no boolean indexing)
  copy     ss_tool_copy_fwd moving as many bytes as the op must (half read, half written): the rate a streaming kernel reaches here

Ops: tile_views (all 25 windows of both views: 3 bytes read and 12 written per tile pixel and view), blend_scene (blend_tiles over the
whole mosaic, the default outputs disparity, label, spread: every tile's disparity and logits read once, 9 bytes written per mosaic
pixel) and blend_band (the same for the rows of band 1 alone: what SceneStereo issues per tile row).

Then the loop around a model: SceneStereo on that scene with tests/standin_model.StandInSemStereo after install + accelerate, against
the same number of bare model calls on pre-cut views through the same PairPipeline, each joined onto the calling stream -- device-event
time per scene; the difference over the number of tiles is what tiling costs per tile (windows, blending, joins, the bookkeeping).

Per op and variant: device-event time, host time to issue a call and wall time per call for every round (windows of --window-ms of
back-to-back calls), their medians, the algorithmic bytes, and for hip the bytes over the device-event time as a fraction of the copy's
rate in the same run.  `hip_slower_than_torch_in_every_round` is the routing rule's input.  --out FILE keeps the whole record as JSON.

Not measured here: scenes whose logits mosaic does not fit in memory, batch > 1, the copy of a host scene.

usage: python tools/bench_scene.py [--scene 4096 --tile 1024 --overlap 256] [--rounds 7 --window-ms 100] [--lanes 6] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

C = 6
WANT = ("disparity", "label", "spread")


def algorithmic_bytes(plan, band):
    """What each op must move, from the plan alone (uint8 scenes, float32 tiles, float32 disparity and spread, a uint8 label)."""
    (th, tw), H, W = plan.size, plan.height, plan.width
    inside = sum((min(y + th, H) - y) * (min(x + tw, W) - x) for y, x in plan.origins)
    y0, y1, rows = plan.bands[band]
    in_band = sum((min(plan.origin_y[k] + th, y1) - max(plan.origin_y[k], y0)) * (min(x + tw, W) - x) for k in rows for x in plan.origin_x)
    return {"tile_views": 2 * (3 * inside + 12 * len(plan) * th * tw), "blend_scene": 4 * (1 + C) * inside + 9 * H * W,
            "blend_band": 4 * (1 + C) * in_band + 9 * (y1 - y0) * W}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", type=int, default=4096)
    ap.add_argument("--tile", type=int, default=1024)
    ap.add_argument("--overlap", type=int, default=256)
    ap.add_argument("--lanes", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="least calls per timed window")
    ap.add_argument("--window-ms", type=float, default=100.0, help="work per timed window")
    ap.add_argument("--no-model", action="store_true", help="the two kernels only")
    ap.add_argument("--out", default=None, help="write the whole record to this JSON file")
    args = ap.parse_args()

    import torch
    import semstereo_amd as sa
    from semstereo_amd._lib import call
    assert torch.cuda.is_available(), "bench_scene.py needs the MI355X"
    sa._lib.load()
    dev, S = torch.device("cuda"), args.scene

    def off(fn):
        def wrapper():
            sa.engine.SCENE_HIP = False
            try:
                return fn()
            finally:
                sa.engine.SCENE_HIP = True
        return wrapper

    plan = sa.TilePlan(S, S, tile=args.tile, overlap=args.overlap)
    band = min(1, plan.nty - 1)
    g = torch.Generator().manual_seed(5)
    left = torch.randint(0, 256, (S, S, 3), generator=g, dtype=torch.uint8).to(dev)
    right = torch.roll(left, shifts=-5, dims=1)
    n, (th, tw) = len(plan), plan.size
    disp = (torch.randn((n, th, tw), generator=g) * 20.0).to(dev)
    logit = (torch.randn((n, C, th, tw), generator=g) * 3.0).to(dev)
    by = algorithmic_bytes(plan, band)
    src = torch.empty(max(by.values()) // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    mosaic = sa.blend_tiles(plan, disp, logit, want=WANT)

    def copy(nbytes):
        half = nbytes // 2 // 16 * 16
        return lambda: call("ss_tool_copy_fwd", src.data_ptr(), dst.data_ptr(), half)

    ops = {
        "tile_views": {"hip": lambda: sa.tile_views(left, right, plan.origins, plan.size)},
        "blend_scene": {"hip": lambda: sa.blend_tiles(plan, disp, logit, out=mosaic, want=WANT)},
        "blend_band": {"hip": lambda: sa.blend_tiles(plan, disp, logit, rows=plan.bands[band][:2], out=mosaic, want=WANT)},
    }
    for name, variants in ops.items():
        variants["torch"] = off(variants["hip"])
        variants["copy"] = copy(by[name])
    res = {"workload": f"{S} x {S} uint8 scene pair, tiles {plan.size}, overlap {plan.overlap}, ramp {plan.ramp}: {n} tiles in {plan.nty} "
                       f"tile rows, C = {C}; blend outputs {WANT}; band {band} = rows {plan.bands[band][:2]}",
           "rounds": args.rounds, "window_ms": args.window_ms, "bytes": by, "ops": {}}
    a, b = ops["tile_views"]["hip"](), ops["tile_views"]["torch"]()
    checks = {"views_values_differing": int((a[0] != b[0]).sum()) + int((a[1] != b[1]).sum())}
    p = {k: v.clone() for k, v in ops["blend_scene"]["hip"]().items()}
    q = off(lambda: sa.blend_tiles(plan, disp, logit, want=WANT))()
    checks.update({f"{k}_values_differing": int((p[k] != q[k]).sum()) for k in WANT})
    checks["pixels_under_one_tile"] = float((sa.blend_tiles(plan, disp, want=("count",))["count"] == 1).float().mean())
    res["checks"] = checks
    print(f"hip against the composition on the device: {checks}", flush=True)
    del a, b, p, q
    iters = {}
    for op, variants in ops.items():
        for name, fn in variants.items():
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            iters[op, name] = int(min(max(args.window_ms / (1e3 * (time.perf_counter() - t0) / 3), args.iters), 5000))
    times = {op: {v: {"device_ms": [], "host_issue_ms": [], "wall_ms": []} for v in variants} for op, variants in ops.items()}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn, n_it, into):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(n_it):
            fn()
        e1.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        into["device_ms"].append(e0.elapsed_time(e1) / n_it)
        into["host_issue_ms"].append(1e3 * (t1 - t0) / n_it)
        into["wall_ms"].append(1e3 * (t2 - t0) / n_it)

    for _ in range(args.rounds):
        for op, variants in ops.items():
            for name, fn in variants.items():
                timed(fn, iters[op, name], times[op][name])

    def summary(t):
        return {k: {"median": statistics.median(x), "min": min(x), "max": max(x), "rounds": x} for k, x in t.items()}

    for op, variants in times.items():
        r = {name: dict(summary(t), iters_per_round=iters[op, name]) for name, t in variants.items()}
        hip, tor = r["hip"]["device_ms"], r["torch"]["device_ms"]
        r["hip_slower_than_torch_in_every_round"] = all(h > t for h, t in zip(hip["rounds"], tor["rounds"]))
        r["torch_over_hip_device"] = tor["median"] / hip["median"]
        r["hip_GBs"] = by[op] / (hip["median"] * 1e-3) / 1e9
        r["copy_GBs"] = (by[op] // 2 // 16 * 16 * 2) / (r["copy"]["device_ms"]["median"] * 1e-3) / 1e9
        r["hip_fraction_of_copy_rate"] = r["hip_GBs"] / r["copy_GBs"]
        res["ops"][op] = r
        line = f"{op:12s}" + "".join(f" {k} {v['device_ms']['median']:.4f} ms" for k, v in r.items() if isinstance(v, dict))
        line += f" | hip issue {r['hip']['host_issue_ms']['median']:.4f} ms, torch/hip {r['torch_over_hip_device']:.2f}"
        line += f", {r['hip_GBs']:.0f} GB/s = {r['hip_fraction_of_copy_rate']:.2f} of the copy's {r['copy_GBs']:.0f}"
        print(line + (" | HIP SLOWER IN EVERY ROUND" if r["hip_slower_than_torch_in_every_round"] else ""), flush=True)
    del disp, logit, mosaic, src, dst
    torch.cuda.empty_cache()

    if not args.no_model:
        import standin_model
        net = standin_model.StandInSemStereo(64, sa.modules).to(dev).eval()
        previous = sa.install(standin_model)
        try:
            sa.accelerate(net)
            stereo = sa.SceneStereo(net, tile=args.tile, overlap=args.overlap, lanes=args.lanes)
            stereo(left, right)                                         # (weight packing, the lanes' allocator pools)
            pipe = stereo.pipe
            views = sa.tile_views(left, right, plan.origins, plan.size)

            def bare():
                held = []
                for i in range(n):
                    held.append((pipe(views[0][i:i + 1], views[1][i:i + 1]), pipe.last_event))
                for out, event in held:
                    pipe.join(out, event=event)

            variants = {"scene_stereo": lambda: stereo(left, right), "bare_model_calls": bare}
            for fn in variants.values():
                fn()
            t = {name: {"device_ms": [], "host_issue_ms": [], "wall_ms": []} for name in variants}
            for _ in range(args.rounds):
                for name, fn in variants.items():
                    timed(fn, 2, t[name])
            r = {name: dict(summary(x), iters_per_round=2) for name, x in t.items()}
            r["tiles"], r["lanes"], r["peak_resident_tile_rows"] = n, args.lanes, stereo.peak_resident_tile_rows
            r["tiling_ms_per_tile"] = (r["scene_stereo"]["device_ms"]["median"] - r["bare_model_calls"]["device_ms"]["median"]) / n
            r["tiling_share_of_scene"] = 1.0 - r["bare_model_calls"]["device_ms"]["median"] / r["scene_stereo"]["device_ms"]["median"]
            res["scene_stereo"] = r
            print(f"scene_stereo {r['scene_stereo']['device_ms']['median']:.2f} ms per scene, {n} bare model calls "
                  f"{r['bare_model_calls']['device_ms']['median']:.2f} ms: tiling costs {r['tiling_ms_per_tile']:.4f} ms per tile "
                  f"({100 * r['tiling_share_of_scene']:.2f} % of the scene); peak resident tile rows {stereo.peak_resident_tile_rows}", flush=True)
            stereo.close()
        finally:
            sa.uninstall(standin_model, previous)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"bench_scene": dict({op: r["hip"]["device_ms"]["median"] for op, r in res["ops"].items()},
                                          **({"scene_stereo_ms": res["scene_stereo"]["scene_stereo"]["device_ms"]["median"]}
                                             if "scene_stereo" in res else {}))}))


if __name__ == "__main__":
    main()
