#!/usr/bin/env python3
"""The training step of a WHOLE reference-shaped model two ways, measured: its own forward() untouched (after `install()` +
`accelerate()`: the reference-named HIP ops and the module twins under the statements of models/SemStereo.py:273-324) against the
routed one (`accelerate(model, fuse_forward=True, fuse_training=True)`: install.fused_training_forward, i.e. train.attention_tail and
train.concat_volume_sampled in place of those statements).

  model    tests/heads_model.HeadsStandIn: the twins of the 3-D stack, the real FeatUp / Conv2x / Spx2 / segmenthead / ChalProjection
           classes with the reference's channel counts, a closed-form stand-in pyramid for the backbone (neither timm nor the reference
           is needed); unit-gain random weights (bench.init_unit_gain)
  step     forward in train() + semstereo_amd.train_objective + backward + fused-Adam step (main_us3d.py:186-222), 1024 x 1024,
           maxdisp 64, batch 1 and 4
  arms     `untouched` and `routed`, each on its own copy of the model with its own optimizer, alternating round by round in ONE
           process; every (batch, switches) configuration runs in a child process of its own under a time limit, and the tool stops
           at the first child that fails or runs out of time
  switches the decoder / heads training switches (SS_DECODER_TRAIN_HIP, SS_HEADS_TRAIN_HIP) off (the default) and on

Per configuration and arm: median / min / max over the rounds of the device-event time per step, peak allocated memory during the
arm's windows (both copies' weights and optimizer states are resident throughout), the ratio routed / untouched per round, and
-- from one extra step per arm under a dispatch logger -- every ATen operator that ran on a 5-D tensor (a volume) with the source
line that called it, so that a statement of :273-324 still running as PyTorch operators shows up by name.

usage: python tools/bench_train_route.py [--batches 1,4] [--rounds 5 --steps 3] [--out profiles/train_route_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

ARMS = ("untouched", "routed")
#: operators that move no data (views, allocations, queries): not listed
_VIEWS = {"view", "_unsafe_view", "unsqueeze", "squeeze", "expand", "permute", "transpose", "slice", "select", "alias", "detach", "as_strided",
          "reshape", "_reshape_alias", "unbind", "split", "split_with_sizes", "t", "empty", "empty_like", "empty_strided", "new_empty",
          "new_empty_strided", "result_type", "is_same_size", "sym_size", "sym_stride", "sym_numel", "lift_fresh", "unfold", "narrow"}


def worker(args):
    import copy
    import traceback

    import torch
    from torch.utils._python_dispatch import TorchDispatchMode
    from torch.utils._pytree import tree_flatten

    import bench
    import heads_model
    import semstereo_amd as sa
    import standin_model
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_train_route.py measures on the GPU and found none (there is no fall-back)")
    sa._lib.load()
    E, M = sa.engine, sa.modules
    dev = torch.device("cuda")
    B, H, W, md = args.batch, args.height, args.width, args.maxdisp
    base = heads_model.HeadsStandIn(md, M, twins=True, head_twins=True)
    bench.init_unit_gain(base, 1234)
    nets = {"untouched": copy.deepcopy(base).to(dev).train(), "routed": copy.deepcopy(base).to(dev).train()}
    del base
    sa.install(standin_model)                                   # the op library in the globals the untouched forward() reads
    sa.accelerate(nets["untouched"])
    sa.accelerate(nets["routed"], fuse_forward=True, fuse_training=True)
    opts = {k: torch.optim.Adam(n.parameters(), lr=1e-3, betas=(0.9, 0.999), fused=True) for k, n in nets.items()}
    g = torch.Generator(device=dev).manual_seed(77)
    left = torch.randn(B, 3, H, W, generator=g, device=dev)
    right = torch.roll(left, shifts=-5, dims=3) + 0.05 * torch.randn(B, 3, H, W, generator=g, device=dev)
    gt, gt4 = [(torch.rand(B, H // q, W // q, generator=g, device=dev) * 2 - 1) * 1.25 * md for q in (1, 4)]       # the range mask keeps 80 %
    labels = torch.randint(0, 6, (B, H, W), generator=g, device=dev)

    def step(arm):
        net, opt = nets[arm], opts[arm]
        opt.zero_grad(set_to_none=True)
        outs, lab, lab_r = net(left, right)
        loss = sa.train_objective(outs, lab, lab_r, gt, gt4, labels, md, False)[0]
        loss.backward()
        opt.step()
        return loss

    class VolumeOps(TorchDispatchMode):
        """every ATen operator that touches a 5-D tensor: (operator, calling line of this repo) -> [calls, bytes of the largest operand]"""

        def __init__(self):
            super().__init__()
            self.seen = {}

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            name = str(func)                                    # "aten.mul.Tensor"
            if name.split(".")[1 if name.count(".") else 0] not in _VIEWS:
                vols = [t for t in tree_flatten((args, kwargs, out))[0] if isinstance(t, torch.Tensor) and t.dim() == 5]
                if vols:
                    where = "(autograd backward)"
                    for fr in reversed(traceback.extract_stack(limit=24)):
                        if (os.sep + "semstereo_amd" + os.sep in fr.filename or os.sep + "tests" + os.sep in fr.filename) and fr.name != "__torch_dispatch__":
                            where = f"{os.path.relpath(fr.filename, ROOT)}:{fr.lineno}"
                            break
                    e = self.seen.setdefault(f"{name} @ {where}", [0, 0])
                    e[0] += 1
                    e[1] += max(t.numel() * t.element_size() for t in vols)
            return out

    rec = {"batch": B, "switches": {"decoder_train_hip": bool(E.DECODER_TRAIN_HIP), "heads_train_hip": bool(E.HEADS_TRAIN_HIP)},
           "rounds": args.rounds, "steps_per_round": args.steps}
    counts = {}
    for arm in ARMS:                                            # warm both arms: weight packing, allocator pools, clocks
        before = dict(M.PATH_COUNTS)
        calls = nets[arm].calls
        t0, n = time.perf_counter(), 0
        while n < args.warmup or time.perf_counter() - t0 < args.warmup_seconds:
            loss = step(arm)
            n += 1
            torch.cuda.synchronize()
        counts[arm] = {k: (M.PATH_COUNTS.get(k, 0) - before.get(k, 0)) / n for k in sorted(set(M.PATH_COUNTS) | set(before))
                       if M.PATH_COUNTS.get(k, 0) != before.get(k, 0)}
        counts[arm]["own_forward_calls"] = (nets[arm].calls - calls) / n
        assert bool(torch.isfinite(loss)), (arm, float(loss))
    assert counts["routed"]["own_forward_calls"] == 0 and counts["routed"].get("train_route") == 1, counts
    assert counts["untouched"]["own_forward_calls"] == 1 and "train_route" not in counts["untouched"], counts
    ms = {arm: [] for arm in ARMS}
    peak = {arm: 0 for arm in ARMS}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.rounds):
        for arm in ARMS:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            e0.record()
            for _ in range(args.steps):
                loss = step(arm)
            e1.record()
            torch.cuda.synchronize()
            ms[arm].append(e0.elapsed_time(e1) / args.steps)
            peak[arm] = max(peak[arm], torch.cuda.max_memory_allocated())
            assert bool(torch.isfinite(loss)), (arm, float(loss))
    for arm in ARMS:
        for o in opts.values():
            o.zero_grad(set_to_none=True)
        resident = torch.cuda.memory_allocated()
        with VolumeOps() as log:
            step(arm)
        torch.cuda.synchronize()
        ops_seen = sorted(log.seen.items(), key=lambda kv: -kv[1][1])
        rec[arm] = {"ms_per_step": {"median": statistics.median(ms[arm]), "min": min(ms[arm]), "max": max(ms[arm]), "rounds": ms[arm]},
                    "peak_allocated_gb": peak[arm] / 2 ** 30, "resident_before_a_step_gb": resident / 2 ** 30,
                    "path_counts_per_step": counts[arm],
                    "aten_ops_on_5d_tensors": {k: {"calls": v[0], "mib": v[1] / 2 ** 20} for k, v in ops_seen},
                    "aten_ops_on_5d_tensors_total_mib": sum(v[1] for _, v in ops_seen) / 2 ** 20}
    ratios = [r / u for r, u in zip(ms["routed"], ms["untouched"])]
    rec["routed_over_untouched"] = {"of_medians": rec["routed"]["ms_per_step"]["median"] / rec["untouched"]["ms_per_step"]["median"],
                                    "per_round": ratios}
    rec["routed_slower_in_any_round"] = any(r > 1.0 for r in ratios)
    rec["peak_allocated_routed_minus_untouched_gb"] = rec["routed"]["peak_allocated_gb"] - rec["untouched"]["peak_allocated_gb"]
    rec["device"] = torch.cuda.get_device_name(0)
    rec["conv_engine"] = E.CONV_ENGINE
    with open(args.part, "w") as f:
        json.dump(rec, f)
    print(json.dumps({k: rec[k] for k in ("batch", "switches", "routed_over_untouched", "routed_slower_in_any_round")}), flush=True)
    for arm in ARMS:
        print(arm, json.dumps({k: rec[arm][k] for k in ("ms_per_step", "peak_allocated_gb", "aten_ops_on_5d_tensors_total_mib")}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1024)
    ap.add_argument("--maxdisp", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--warmup-seconds", type=float, default=1.5)
    ap.add_argument("--switches", default="off,on", help="the decoder / heads training switches: off, on or both")
    ap.add_argument("--step-timeout", type=float, default=240.0, help="seconds one (batch, switches) configuration may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_route_bench.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--batch", type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument("--part", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    assert args.rounds >= 5, "at least five rounds: 'slower in any round' is decided on all of them"
    if args.worker:
        worker(args)
        return
    res = {"workload": f"{args.height}x{args.width} maxdisp={args.maxdisp}: train() forward + train_objective + backward + fused Adam step of "
                       "tests/heads_model.HeadsStandIn (twins, real decoder / heads / projections, stand-in pyramid)",
           "arms": {"untouched": "install() + accelerate(): the model's own forward()", "routed": "accelerate(fuse_forward=True, fuse_training=True)"},
           "configs": {}}
    out = os.path.abspath(args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    for b in [int(v) for v in args.batches.split(",")]:
        for sw in args.switches.split(","):
            name = f"batch{b}/switches_{sw}"
            part = out + f".part_b{b}_{sw}"
            env = dict(os.environ, SS_DECODER_TRAIN_HIP="1" if sw == "on" else "0", SS_HEADS_TRAIN_HIP="1" if sw == "on" else "0")
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--batch", str(b), "--part", part, "--height", str(args.height),
                   "--width", str(args.width), "--maxdisp", str(args.maxdisp), "--rounds", str(args.rounds), "--steps", str(args.steps),
                   "--warmup", str(args.warmup), "--warmup-seconds", str(args.warmup_seconds)]
            print("==", name, flush=True)
            try:
                r = subprocess.run(cmd, env=env, timeout=args.step_timeout)
            except subprocess.TimeoutExpired:
                raise SystemExit(f"{name}: no result within {args.step_timeout:.0f} s -- stopped, nothing further is started")
            if r.returncode != 0:
                raise SystemExit(f"{name}: the worker ended with status {r.returncode} -- stopped, nothing further is started")
            with open(part) as f:
                res["configs"][name] = json.load(f)
            os.remove(part)
            with open(out, "w") as f:                           # (kept up to date: what was measured before a later failure stays)
                json.dump(res, f, indent=1)
    print(json.dumps({"train_route_routed_over_untouched": {k: v["routed_over_untouched"]["of_medians"] for k, v in res["configs"].items()}}))


if __name__ == "__main__":
    main()
