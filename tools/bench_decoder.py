#!/usr/bin/env python3
"""The reference's 2-D decoder, measured (models/SemStereo.py:59-86 FeatUp on both views, :267-271 the spx chain and spx2): every
transposed conv and every concat + 3x3 conv of it, two ways in one process, warm, alternating round by round:

  hip      the kernels the twins run in inference: engine.run_deconv2d (csrc/deconv2d_bf16s.hip; FeatUp: both views in one launch)
           and engine.run_conv2d_cat (the concat-free form of the 2-D conv)
  torch    the same layer on the stock PyTorch modules (ConvTranspose2d / torch.cat + Conv2d, BatchNorm2d, ReLU): what runs without
           accelerate(decoder=True), i.e. at the parent commit

on closed-form pyramid features (the five maps the backbone hands to FeatUp, 1/2 .. 1/32).  Per layer: median / min / max device
time over the rounds for both, the ratio, the torch path's run-to-run spread, and for hip the fp32-equivalent TFLOP/s and the
fraction of the 16-bit MFMA peak as issued (x3 products).  Totals per shape.  --out FILE keeps the record as JSON.

usage: python tools/bench_decoder.py [--shapes 1024x1,1024x4,2048x1] [--rounds 5 --iters 10] [--only hip] [--out profiles/decoder_bench.json]
       rocprofv3 --kernel-trace --stats -d <dir> -- python3 tools/bench_decoder.py --shapes 1024x1 --only hip --rounds 2
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_16BIT = 2.5e15          # dense fp16 / bf16 MFMA, nominal clock
CHANS = (64, 128, 256, 384, 512)
CHANS2 = (64, 128, 256, 384, 256)


def closed_form(torch, shape, salt):
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, device="cuda", dtype=torch.float32)
    return torch.sin(i * (0.61803 + 0.001 * salt) + salt).reshape(shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x1,1024x4,2048x1")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", default="")
    ap.add_argument("--miopen-find", action="store_true", help="torch.backends.cudnn.benchmark for the torch legs")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import semstereo_amd as sa
    E, M = sa.engine, sa.modules
    assert torch.cuda.is_available() and E.CONV_ENGINE == "f16x3"
    torch.backends.cudnn.benchmark = args.miopen_find         # (off: PyTorch's default, MIOpen's immediate mode -- what a script gets)
    torch.manual_seed(0)
    featup = M.FeatUp().cuda().eval()
    spx = {"spx32_16": M.Conv2x(256, 384, True), "spx16_8": M.Conv2x(768, 256, True), "spx8_4": M.Conv2x(512, 128, True),
           "spx4_2": M.Conv2x(256, 64, True)}
    for m in spx.values():
        m.cuda().eval()
    spx2 = M.Spx2(128, 6).cuda().eval()
    variants = [v for v in ("hip", "torch") if not args.only or v == args.only]
    record = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "iters": args.iters, "shapes": {}}

    def stock(bc, x):
        return F.relu(bc.bn(bc.conv(x)))

    for spec in args.shapes.split(","):
        size, B = (int(v) for v in spec.split("x"))
        L = [closed_form(torch, (B, c, size >> (k + 1), size >> (k + 1)), k) for k, c in enumerate(CHANS)]
        R = [closed_form(torch, (B, c, size >> (k + 1), size >> (k + 1)), 10 + k) for k, c in enumerate(CHANS)]
        S = [closed_form(torch, (B, c, size >> (k + 1), size >> (k + 1)), 20 + k) for k, c in enumerate(CHANS2)]
        entries = []          # (name, flops, {variant: callable}), built while the chain is walked once on the HIP path
        with torch.no_grad():
            xl, xr = L[4], R[4]
            for k, name in enumerate(("deconv32_16", "deconv16_8", "deconv8_4", "deconv4_2")):
                c2x = getattr(featup, name)
                a, b = c2x.conv1, c2x.conv2
                rl, rr = L[3 - k], R[3 - k]
                Bn, Cin, H, W = xl.shape
                Co = a.conv.out_channels
                entries.append((f"featup.{name}.conv1 {Cin}->{Co} @{H}x{W} x2 views", 2 * 2 * Bn * H * W * 16 * Cin * Co, {
                    "hip": (lambda a=a, xl=xl, xr=xr: E.run_deconv2d(a, "c2x", a.conv, a.bn, xl, True, xb=xr)),
                    "torch": (lambda a=a, xl=xl, xr=xr: (stock(a, xl), stock(a, xr)))}))
                y = E.run_deconv2d(a, "c2x", a.conv, a.bn, xl, True, xb=xr)
                yl, yr = y[:Bn], y[Bn:]
                C2 = b.conv.out_channels
                entries.append((f"featup.{name}.conv2 {2 * Co}->{C2} @{2 * H}x{2 * W} x2 views", 2 * 2 * Bn * 4 * H * W * 9 * 2 * Co * C2, {
                    "hip": (lambda b=b, yl=yl, yr=yr, rl=rl, rr=rr: E.run_conv2d_cat(b, "bc2d", b.conv, b.bn, yl, rl, True, xb=yr, remb=rr)),
                    "torch": (lambda b=b, yl=yl, yr=yr, rl=rl, rr=rr: (stock(b, torch.cat((yl, rl), 1)), stock(b, torch.cat((yr, rr), 1))))}))
                z = E.run_conv2d_cat(b, "bc2d", b.conv, b.bn, yl, rl, True, xb=yr, remb=rr)
                xl, xr = z[:Bn], z[Bn:]
            x = S[4]
            for k, name in enumerate(("spx32_16", "spx16_8", "spx8_4", "spx4_2")):
                a, b = spx[name].conv1, spx[name].conv2
                rem = S[3 - k]
                Bn, Cin, H, W = x.shape
                Co, C2 = a.conv.out_channels, b.conv.out_channels
                entries.append((f"{name}.conv1 {Cin}->{Co} @{H}x{W}", 2 * Bn * H * W * 16 * Cin * Co, {
                    "hip": (lambda a=a, x=x: E.run_deconv2d(a, "c2x", a.conv, a.bn, x, True)),
                    "torch": (lambda a=a, x=x: stock(a, x))}))
                y = E.run_deconv2d(a, "c2x", a.conv, a.bn, x, True)
                entries.append((f"{name}.conv2 {2 * Co}->{C2} @{2 * H}x{2 * W}", 2 * Bn * 4 * H * W * 9 * 2 * Co * C2, {
                    "hip": (lambda b=b, y=y, rem=rem: E.run_conv2d_cat(b, "bc2d", b.conv, b.bn, y, rem, True)),
                    "torch": (lambda b=b, y=y, rem=rem: stock(b, torch.cat((y, rem), 1)))}))
                x = E.run_conv2d_cat(b, "bc2d", b.conv, b.bn, y, rem, True)
            Bn, Cin, H, W = x.shape
            entries.append((f"spx2 {Cin}->6 @{H}x{W}", 2 * Bn * H * W * 16 * Cin * 6, {
                "hip": (lambda x=x: E.run_deconv2d(spx2, "spx2", spx2[0], None, x, False)),
                "torch": (lambda x=x: spx2[0](x))}))

            times = {name: {v: [] for v in variants} for name, _, _ in entries}
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for name, _, fns in entries:                      # warm: weight packing, MIOpen's search
                for v in variants:
                    for _ in range(2):
                        out = fns[v]()
                        assert out is not None, (name, v)
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for name, _, fns in entries:
                    for v in variants:
                        ev0.record()
                        for _ in range(args.iters):
                            fns[v]()
                        ev1.record()
                        ev1.synchronize()
                        times[name][v].append(ev0.elapsed_time(ev1) * 1e3 / args.iters)      # us per call
        rows, total = [], {v: 0.0 for v in variants}
        print(f"== {size} x {size}, batch {B} ==")
        for name, flops, _ in entries:
            row = {"layer": name, "gflop": flops / 1e9}
            for v in variants:
                t = times[name][v]
                row[v] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t)}
                total[v] += statistics.median(t)
            if "hip" in row:
                row["hip_tflops_fp32_equiv"] = flops / row["hip"]["median_us"] / 1e6
                row["hip_frac_16bit_peak_issued"] = 3 * flops / (row["hip"]["median_us"] * 1e-6) / PEAK_16BIT
            if len(variants) == 2:
                row["torch_over_hip"] = row["torch"]["median_us"] / row["hip"]["median_us"]
                row["torch_spread"] = (row["torch"]["max_us"] - row["torch"]["min_us"]) / row["torch"]["median_us"]
                row["hip_spread"] = (row["hip"]["max_us"] - row["hip"]["min_us"]) / row["hip"]["median_us"]
            rows.append(row)
            print(f"{name:58s} " + "  ".join(f"{v} {row[v]['median_us']:9.1f} us [{row[v]['min_us']:.1f}, {row[v]['max_us']:.1f}]" for v in variants)
                  + (f"  torch/hip {row['torch_over_hip']:5.2f}" if len(variants) == 2 else "")
                  + (f"  {row['hip_tflops_fp32_equiv']:6.1f} TFLOP/s fp32-eq, {row['hip_frac_16bit_peak_issued']:.3f} of 16-bit peak" if "hip" in row else ""))
        print("total: " + "  ".join(f"{v} {total[v] / 1e3:.3f} ms" for v in variants)
              + (f"  torch/hip {total['torch'] / total['hip']:.2f}" if len(variants) == 2 else ""))
        record["shapes"][spec] = {"size": size, "batch": B, "layers": rows, "total_us": total}
        del L, R, S, entries
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
    print(json.dumps({"decoder_total_us": {k: v["total_us"] for k, v in record["shapes"].items()}}))


if __name__ == "__main__":
    main()
