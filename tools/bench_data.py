#!/usr/bin/env python3
"""Sample preparation, measured (datasets/us3d_.py:70-215) at 1024 x 1024, batch 4 and 1, in one process, the variants alternating round
by round:

  hip      semstereo_amd.data on csrc/sample_prep.hip
  torch    the same call with engine.DATA_HIP off: the PyTorch composition on the device (no boolean indexing, no .item())
  copy     ss_tool_copy_fwd moving as many bytes as the op must (half read, half written): the rate a streaming kernel reaches here
  host     the preparation as the reference's __getitem__ forms it, written here from stock PIL / numpy / scipy / torch calls, per ITEM on
           one CPU thread: ToTensor + Normalize of both views, five nearest resizes, three convert("L"), a float64 mean and std, two
           float64 convolve2d (decode not included: the arrays are in memory).  Skipped where scipy or PIL is missing.

Ops: views (both), pyramid (disparity_4/8/16, label, label_2/4 from a float32 disparity and a uint8 label), gradients (luma + statistics
and gx / gy: two entry points), prepare_all (every key of the US3D training sample) and prepare_five (left, right, disparity,
disparity_4, label: what a training script reads).  Per op and variant: device-event time, host time to issue a call and wall time per
call for every round (windows of --window-ms of back-to-back calls), their medians, the algorithmic bytes, and for hip the bytes over
the device-event time as a fraction of the copy's rate in the same run.  The device-event time of back-to-back calls is the larger of
the kernels' time and the host's issue time: where `host_issue_ms` is as large, the figure is the launch path's, not the kernels'.
`hip_slower_than_torch_in_every_round` is the routing rule's input.  --out FILE keeps the whole record as JSON.

usage: python tools/bench_data.py [--batches 4,1] [--height 1024 --width 1024] [--rounds 7 --window-ms 100 --host-iters 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIVE = ("left", "right", "disparity", "disparity_4", "label")


def algorithmic_bytes(B, H, W):
    """What each op must move, from the shapes alone (uint8 views and label, float32 disparity and results)."""
    n = B * H * W
    disp_levels = n // 16 + n // 64 + n // 256
    label_levels = n // 4 + n // 16
    by = {"views": 2 * n * (3 + 12),
          "pyramid": 4 * disp_levels * 2 + (n + 4 * n) + 4 * label_levels,        # sampled reads and writes; the label read whole
          "gradients": n * (3 + 1 + 1 + 8)}                                        # RGB in, luma out and in again, gx and gy out
    by["prepare_all"] = by["views"] + by["pyramid"] + by["gradients"]
    by["prepare_five"] = by["views"] + 2 * 4 * (n // 16) + 5 * n
    return by


def host_item(torch, np):
    """One item as the reference's __getitem__ prepares it, or None where a library is missing."""
    try:
        import scipy.signal as sig
        from PIL import Image
    except ImportError:
        return None
    mean = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)

    def view(img):
        t = torch.from_numpy(np.array(img, dtype=np.uint8)).permute(2, 0, 1).contiguous().float().div(255)
        return t.sub_(mean).div_(std)

    def item(left_u8, right_u8, disparity, label):
        left_img, right_img = Image.fromarray(left_u8, "RGB"), Image.fromarray(right_u8, "RGB")
        label = np.ascontiguousarray(label, dtype=np.float32)
        img = (left_img.convert("L") - np.mean(left_img.convert("L"))) / np.std(left_img.convert("L"))
        gx = torch.Tensor(sig.convolve2d(img, np.array([[-1, 0, 1]]), "same")).unsqueeze(0)
        gy = torch.Tensor(sig.convolve2d(img, np.array([[-1], [0], [1]]), "same")).unsqueeze(0)
        out = {"left": view(left_img), "right": view(right_img), "disparity": disparity, "label": label, "gx": gx.float(), "gy": gy.float()}
        for k in (4, 8, 16):
            out[f"disparity_{k}"] = np.ascontiguousarray(disparity[::k, ::k])
        for k in (2, 4):
            out[f"label_{k}"] = np.ascontiguousarray(label[::k, ::k])
        return out
    return item


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4,1")
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40, help="least calls per timed window")
    ap.add_argument("--window-ms", type=float, default=100.0, help="work per timed window of the device variants")
    ap.add_argument("--host-iters", type=int, default=3, help="items per round of the host baseline")
    ap.add_argument("--no-host", action="store_true", help="leave the host baseline out (profiling runs)")
    ap.add_argument("--out", default=None, help="write the whole record to this JSON file")
    args = ap.parse_args()
    H, W = args.height, args.width

    import numpy as np
    import torch
    import semstereo_amd as sa
    from semstereo_amd._lib import call
    assert torch.cuda.is_available(), "bench_data.py needs the MI355X"
    sa._lib.load()
    D, dev = sa.data, torch.device("cuda")

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

    res = {"workload": f"{H}x{W}: both views normalised, disparity_4/8/16 + label + label_2/4, gx / gy, and prepare_sample with all keys "
                       "and with the five a training script reads", "rounds": args.rounds, "window_ms": args.window_ms,
           "host_items_per_round": args.host_iters, "by_batch": {}}
    item = None if args.no_host else host_item(torch, np)
    for B in [int(b) for b in args.batches.split(",")]:
        g = torch.Generator(device=dev).manual_seed(97)
        left = torch.randint(0, 256, (B, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
        right = torch.randint(0, 256, (B, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
        disp = 120 * torch.rand(B, H, W, generator=g, device=dev) - 60
        label = torch.randint(0, 6, (B, H, W), generator=g, device=dev, dtype=torch.uint8)
        raw = {"left_u8": left, "right_u8": right, "disparity": disp, "label": label}
        by = algorithmic_bytes(B, H, W)
        src = torch.empty(max(by.values()) // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)

        def copy(nbytes):
            half = nbytes // 2 // 16 * 16
            return lambda: call("ss_tool_copy_fwd", src.data_ptr(), dst.data_ptr(), half)

        ops = {
            "views": {"hip": lambda: D.normalize_views(left, right)},
            "pyramid": {"hip": lambda: D.nearest_pyramid(disp, label)},
            "gradients": {"hip": lambda: D.image_gradients(left)},
            "prepare_all": {"hip": lambda: D.prepare_sample(raw, True)},
            "prepare_five": {"hip": lambda: D.prepare_sample(raw, True, keys=FIVE)},
        }
        for name, variants in ops.items():
            variants["torch"] = off(variants["hip"])
            variants["copy"] = copy(by[name])
        a, b = ops["prepare_all"]["hip"](), ops["prepare_all"]["torch"]()
        checks = {f"{k}_values_differing": int((a[k].view(torch.int32) != b[k].view(torch.int32)).sum()) for k in a}
        print(f"batch {B}: hip against the composition on the device: {checks}", flush=True)
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
        host_ms = []
        cpu = {k: v[0].cpu().numpy() for k, v in raw.items()}
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
            if item is not None:
                threads = torch.get_num_threads()
                torch.set_num_threads(1)
                t0 = time.perf_counter()
                for _ in range(args.host_iters):
                    item(cpu["left_u8"], cpu["right_u8"], cpu["disparity"], cpu["label"])
                host_ms.append(1e3 * (time.perf_counter() - t0) / args.host_iters)
                torch.set_num_threads(threads)
        rec = {"bytes": by, "checks": checks, "ops": {}}
        if host_ms:
            rec["host_ms_per_item_one_thread"] = {"median": statistics.median(host_ms), "min": min(host_ms), "max": max(host_ms), "rounds": host_ms}
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
            line = f"batch {B} {op:13s}" + "".join(f" {n} {v['device_ms']['median']:.4f} ms" for n, v in r.items() if isinstance(v, dict))
            line += f" | hip issue {r['hip']['host_issue_ms']['median']:.4f} ms, torch/hip {r['torch_over_hip_device']:.2f}"
            line += f", {r['hip_GBs']:.0f} GB/s = {r['hip_fraction_of_copy_rate']:.2f} of the copy's {r['copy_GBs']:.0f}"
            print(line + (" | HIP SLOWER IN EVERY ROUND" if r["hip_slower_than_torch_in_every_round"] else ""), flush=True)
        if host_ms:
            print(f"batch {B} host preparation, one item on one CPU thread: {statistics.median(host_ms):.1f} ms "
                  f"(prepare_all on the kernels, per item: {rec['ops']['prepare_all']['hip']['device_ms']['median'] / B:.4f} ms)", flush=True)
        res["by_batch"][str(B)] = rec
        del left, right, disp, label, raw, src, dst, ops
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"bench_data": {b: {op: r["hip"]["device_ms"]["median"] for op, r in rec["ops"].items()} for b, rec in res["by_batch"].items()}}))


if __name__ == "__main__":
    main()
