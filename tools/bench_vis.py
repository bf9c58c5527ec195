#!/usr/bin/env python3
"""The evaluation step's image outputs, measured (main_us3d.py:252, :265-268; utils/visualization.py, utils/mask_vis.py,
utils/experiment.py:84-99) at 1024 x 1024, batch 4 (the reference's test_batch_size) and 1, in one process, the variants alternating
round by round:

  hip      semstereo_amd.visualization on csrc/vis.hip
  torch    the same call with engine.VIS_HIP off: the PyTorch composition on the device (no boolean indexing, no .cpu())
  script   the pictures as an evaluation script makes them today, written here from stock numpy and torch calls: a host copy of the whole
           batch, twenty boolean-mask passes over the error, argmax and a palette lookup into float64, F.one_hot for the true labels,
           and the min/max normalisation of the first image on the host
  copy     ss_tool_copy_fwd moving as many bytes as the op must (half read, half written): the rate a streaming kernel reaches here

Ops: error_image, feature_vis (logits, float32 out), label_vis (int64 labels), normalize_image ([B,3,H,W]), eval_images (two estimates;
hip and torch: the first image only, as save_images logs it; script: the whole batch, as the scripts compute it) and eval_images_whole
(first=None).  Per op and variant: device-event time, host time to issue a call and wall time per call for every round (windows of --window-ms of
back-to-back calls), their medians, the algorithmic bytes, and for hip the bytes over the device-event time as a fraction of the copy's
rate in the same run.  The device-event time of back-to-back calls is the larger of the kernels' time and the host's issue time: where
`host_issue_ms` is as large, the figure is the launch path's, not the kernel's.  `hip_slower_than_torch_in_every_round` is the
routing rule's input.  --out FILE keeps the whole record as JSON.

usage: python tools/bench_vis.py [--batches 4,1] [--height 1024 --width 1024] [--rounds 7 --window-ms 100 --script-iters 2] [--out FILE]
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
    """What each op must move, from the shapes alone (fp32 pictures, int64 labels, six channels of logits, a three-channel image)."""
    n = B * H * W
    return {"error_image": n * (4 + 4 + 12), "feature_vis": n * (24 + 12), "label_vis": n * (8 + 12),
            "normalize_image": 3 * n * (4 + 4 + 4)}                     # read for min / max, read again, write


def script_functions(torch, np):
    """The image outputs as a script computes them without this package."""
    import torch.nn.functional as F
    edges = np.array([0, 0.1875, 0.375, 0.75, 1.5, 3, 6, 12, 24, 48, np.inf]) / 3.0
    table = np.zeros((10, 5), dtype=np.float32)
    table[:, 0], table[:, 1] = edges[:-1], edges[1:]
    table[:, 2:] = np.array([[49, 54, 149], [69, 117, 180], [116, 173, 209], [171, 217, 233], [224, 243, 248], [254, 224, 144],
                             [253, 174, 97], [244, 109, 67], [215, 48, 39], [165, 0, 38]], dtype=np.float32) / 255.
    palette = np.array([[0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255]])

    def error_image(est, gt):
        g, e = gt.detach().cpu().numpy(), est.detach().cpu().numpy()
        ok = g > 0
        err = np.abs(g - e)
        err[~ok] = 0
        err[ok] = np.minimum(err[ok] / 3., (err[ok] / g[ok]) / 0.05)
        img = np.zeros(g.shape + (3,), dtype=np.float32)
        for row in table:
            img[(err >= row[0]) & (err < row[1])] = row[2:]
        img[~ok] = 0.
        for i, row in enumerate(table):
            img[:, :10, 20 * i:20 * (i + 1), :] = row[2:]
        return torch.from_numpy(np.ascontiguousarray(img.transpose(0, 3, 1, 2)))

    def feature_vis(z):
        cls = np.argmax(z.cpu().detach().numpy(), axis=1)
        out = np.zeros((z.shape[0], 3) + tuple(z.shape[2:]))
        out[:] = palette[cls].transpose(0, 3, 1, 2)
        return out

    def label_vis(y):
        return feature_vis(F.one_hot(y.to(torch.int64), 6).permute(0, 3, 1, 2).float())

    def normalize_image(v):
        v = v.data.cpu().numpy() if isinstance(v, torch.Tensor) else v
        if v.ndim == 3:
            v = v[:, np.newaxis]
        t = torch.from_numpy(v[:1]).float()
        lo, hi = float(t.min()), float(t.max())
        t = t.clamp(lo, hi).sub(lo).div(max(hi - lo, 1e-5))
        return t.expand(-1, 3, -1, -1) if t.shape[1] == 1 else t

    def eval_images(ests, z, gt, y, img):
        out = {"disp_est": ests, "disp_gt": gt, "imgL": img, "label": [label_vis(y)], "label_est": [feature_vis(z)],
               "errormap": [error_image(e, gt) for e in ests]}
        return {k: [normalize_image(t) for t in (v if isinstance(v, list) else [v])] for k, v in out.items()}
    return {"error_image": error_image, "feature_vis": feature_vis, "label_vis": label_vis, "normalize_image": normalize_image,
            "eval_images": eval_images}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4,1")
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40, help="least calls per timed window")
    ap.add_argument("--window-ms", type=float, default=100.0, help="work per timed window of the device variants")
    ap.add_argument("--script-iters", type=int, default=2)
    ap.add_argument("--no-script", action="store_true", help="leave the host baseline out (profiling runs)")
    ap.add_argument("--out", default=None, help="write the whole record to this JSON file")
    args = ap.parse_args()
    H, W = args.height, args.width

    import numpy as np
    import torch
    import semstereo_amd as sa
    from semstereo_amd._lib import call
    assert torch.cuda.is_available(), "bench_vis.py needs the MI355X"
    sa._lib.load()
    V, dev = sa.visualization, torch.device("cuda")
    script = script_functions(torch, np)

    class composition:
        def __enter__(self):
            sa.engine.VIS_HIP = False

        def __exit__(self, *exc):
            sa.engine.VIS_HIP = True

    def off(fn):
        def wrapper():
            with composition():
                return fn()
        return wrapper

    res = {"workload": f"{H}x{W}: error map, class colours of 6-channel logits and of int64 labels, normalisation of a 3-channel image, "
                       "eval_images with two estimates", "rounds": args.rounds, "window_ms": args.window_ms,
           "script_iters_per_round": args.script_iters, "by_batch": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        g = torch.Generator(device=dev).manual_seed(97)
        rnd = lambda *s: torch.rand(*s, generator=g, device=dev)                     # noqa: E731
        gt = 60 * (rnd(B, H, W) - 0.2)
        ests = [gt + s * torch.exp2(12 * rnd(B, H, W) - 6) * torch.clamp(0.05 * gt.abs(), min=3.0) for s in (1.0, -1.0)]
        z = 4 * (rnd(B, 6, H, W) - 0.5)
        y = torch.randint(0, 6, (B, H, W), generator=g, device=dev)
        img = rnd(B, 3, H, W)
        by = algorithmic_bytes(B, H, W)
        src = torch.empty(max(by.values()) // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)

        def copy(nbytes):
            half = nbytes // 2 // 16 * 16
            return lambda: call("ss_tool_copy_fwd", src.data_ptr(), dst.data_ptr(), half)

        ops = {
            "error_image": {"hip": lambda: V.disp_error_image(ests[0], gt), "script": lambda: script["error_image"](ests[0], gt)},
            "feature_vis": {"hip": lambda: V.feature_vis(z), "script": lambda: script["feature_vis"](z)},
            "label_vis": {"hip": lambda: V.label_vis(y), "script": lambda: script["label_vis"](y)},
            "normalize_image": {"hip": lambda: V.normalize_image(img), "script": lambda: script["normalize_image"](img)},
            "eval_images": {"hip": lambda: V.eval_images(ests, z, gt, y, imgL=img),
                            "script": lambda: script["eval_images"](ests, z, gt, y, img)},
            "eval_images_whole": {"hip": lambda: V.eval_images(ests, z, gt, y, imgL=img, first=None)},
        }
        for name, variants in ops.items():
            variants["torch"] = off(variants["hip"])
            if name in by:
                variants["copy"] = copy(by[name])
            if args.no_script:
                variants.pop("script", None)
        # the pictures of the variants agree before anything is timed (the compositions' division on the device is not pinned: a count)
        a, b = ops["error_image"]["hip"](), ops["error_image"]["torch"]()
        checks = {"error_image_hip_vs_torch_values_differing": int((a != b).sum()),
                  "feature_vis_hip_equals_torch": bool(torch.equal(ops["feature_vis"]["hip"](), ops["feature_vis"]["torch"]())),
                  "label_vis_hip_equals_torch": bool(torch.equal(ops["label_vis"]["hip"](), ops["label_vis"]["torch"]()))}
        if not args.no_script:
            checks["error_image_hip_equals_script"] = bool(torch.equal(a.cpu(), ops["error_image"]["script"]()))
            checks["feature_vis_hip_equals_script"] = bool(np.array_equal(ops["feature_vis"]["hip"]().cpu().numpy().astype(np.float64),
                                                                          ops["feature_vis"]["script"]()))
        print(f"batch {B}: {checks}", flush=True)
        # warm every variant of every op, and size its timed window: enough calls for --window-ms of work (the host baseline: --script-iters)
        iters = {}
        for op, variants in ops.items():
            for name, fn in variants.items():
                for _ in range(1 if name == "script" else 3):
                    fn()
                if name == "script":
                    iters[op, name] = args.script_iters
                    continue
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
            if "script" in r:
                r["script_over_hip_wall"] = r["script"]["wall_ms"]["median"] / r["hip"]["wall_ms"]["median"]
            if "copy" in r:
                r["hip_GBs"] = by[op] / (hip["median"] * 1e-3) / 1e9
                r["copy_GBs"] = (by[op] // 2 // 16 * 16 * 2) / (r["copy"]["device_ms"]["median"] * 1e-3) / 1e9
                r["hip_fraction_of_copy_rate"] = r["hip_GBs"] / r["copy_GBs"]
            rec["ops"][op] = r
            line = f"batch {B} {op:18s}" + "".join(f" {n} {v['device_ms']['median']:.4f} ms" for n, v in r.items() if isinstance(v, dict))
            line += f" | hip issue {r['hip']['host_issue_ms']['median']:.4f} ms, torch/hip {r['torch_over_hip_device']:.2f}"
            if "script" in r:
                line += f", script/hip (wall) {r['script_over_hip_wall']:.1f}"
            if "copy" in r:
                line += f", {r['hip_GBs']:.0f} GB/s = {r['hip_fraction_of_copy_rate']:.2f} of the copy's {r['copy_GBs']:.0f}"
            print(line + (" | HIP SLOWER IN EVERY ROUND" if r["hip_slower_than_torch_in_every_round"] else ""), flush=True)
        res["by_batch"][str(B)] = rec
        del ests, z, y, gt, img, src, dst, ops
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"bench_vis": {b: {op: r["hip"]["device_ms"]["median"] for op, r in rec["ops"].items()} for b, rec in res["by_batch"].items()}}))


if __name__ == "__main__":
    main()
