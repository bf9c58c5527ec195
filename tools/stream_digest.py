#!/usr/bin/env python3
"""SHA-256 digests of everything the streaming kernels return (csrc/loss.hip, metrics.hip, joint_metrics.hip, vis.hip,
sample_prep.hip), on deterministic inputs: two builds that print the same JSON compute the same bits.  A digest covers an output's dtype,
shape and raw bytes, so the 32- and 64-bit words of floats count as they are, NaN patterns included.  The JSON has one digest per shape
and function, taken over the digests of all its outputs; --each lists every output's own, to find the one that differs.

Functions: model_loss_train / model_loss_test / model_label_loss / LRSC_loss with their gradients, train_objective, disparity_metrics
with its record, the confusion matrix (SegmentationMetric.addBatch, twice: the accumulating form), joint_metrics, disp_error_image,
feature_vis, label_vis, normalize_image and prepare_sample with all keys.  Shapes B x H x W, each the smallest that reaches a path:
  2x5x7      the scalar path and row tails            2x8x16     the 16-byte path
  2x33x36    more than one workgroup per image        1x520x512  more than 256 workgroups: a finish thread takes a second trip
  2x8x16+1   contiguous tensors whose storage starts one element past a 16-byte boundary
  2x16x48    prepare_sample only: the pyramid kernel takes H and W divisible by 16
Labels are int64, uint8 and float32, with values outside [0, 6) and, as floats, NaN and inf.  "paths" in the output counts the calls
that took the kernels and those that took the PyTorch composition (the pyramids of the other shapes do).

usage: python tools/stream_digest.py [--each] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("2x5x7", 2, 5, 7, 0), ("2x8x16", 2, 8, 16, 0), ("2x33x36", 2, 33, 36, 0), ("1x520x512", 1, 520, 512, 0), ("2x8x16+1", 2, 8, 16, 1))
PREP_ONLY = (("2x16x48", 2, 16, 48, 0),)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the JSON object to this file as well")
    ap.add_argument("--each", action="store_true", help="one digest per output (2082 of them), not one per shape and function")
    args = ap.parse_args()

    import numpy as np
    import torch
    import semstereo_amd as sa
    from oracle import detdata
    from semstereo_amd import _host, data, joint_metrics, losses, metrics, visualization
    assert torch.cuda.is_available(), "stream_digest.py needs the MI355X"
    sa._lib.load()
    dev = torch.device("cuda")
    digests = {}

    def put(key, t):
        if t is None:
            return
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(t)
        a = t.detach().cpu().contiguous()
        h = hashlib.sha256(f"{a.dtype}{tuple(a.shape)}".encode())
        h.update(a.reshape(-1).view(torch.uint8).numpy().tobytes())
        assert key not in digests, key
        digests[key] = h.hexdigest()

    def place(a, off):
        """The array on the device, contiguous; off = 1: its storage starts one element past a 16-byte boundary."""
        t = torch.from_numpy(np.ascontiguousarray(a))
        buf = torch.empty(t.numel() + off, dtype=t.dtype, device=dev)
        assert buf.data_ptr() % 16 == 0
        out = buf[off:].view(t.shape)
        out.copy_(t)
        return out

    def labels_of(kind, shape, salt):
        v = detdata.uniform(shape, salt, -2.0, 9.0)
        flat = v.reshape(-1)
        if kind == "f32":
            flat[3], flat[5], flat[6], flat[8] = np.nan, np.inf, -0.5, 5.999
            return v
        y = np.floor(v).astype(np.int64)
        if kind == "u8":
            y.reshape(-1)[4] = 200
            return (y & 255).astype(np.uint8)
        y.reshape(-1)[4], y.reshape(-1)[7] = 1 << 40, -(1 << 40)
        return y

    def run_case(name, B, H, W, off, prep_only):
        s = 1000 * (len(digests) + 1)
        u = lambda shape, k, lo=-1.0, hi=1.0: detdata.uniform(shape, s + k, lo, hi)              # noqa: E731
        raw = {"left_u8": place((u((B, H, W, 3), 1, 0, 256)).astype(np.uint8), off),
               "right_u8": place((u((B, H, W, 3), 2, 0, 256)).astype(np.uint8), off)}
        gt_np = u((B, H, W), 3, -80, 80)
        gt_np.reshape(-1)[2] = 0.0
        label_np = {k: labels_of(k, (B, H + 1, W + 3), s + 4) for k in ("i64", "u8", "f32")}
        # ---- sample preparation: every key that the shape has (level k of a map smaller than k is empty)
        def keys(kind, training):
            return [k for k in data.KEYS[kind, training] if not k.rsplit("_", 1)[-1].isdigit() or min(H, W) >= int(k.rsplit("_", 1)[-1])]
        for lk, y in label_np.items():
            y = place(y[:, :H, :W], off)
            for training in (True, False):
                r = dict(raw, disparity=place(gt_np, off), label=y)
                for k, v in data.prepare_sample(r, training, keys=keys("us3d", training)).items():
                    put(f"{name}/prepare_sample/{lk}/{'train' if training else 'test'}/{k}", v)
        r = dict(raw, disparity=place((gt_np * 256).astype(np.int32), off))
        for k, v in data.prepare_sample(r, True, keys=keys("whu", True)).items():
            put(f"{name}/prepare_sample/whu_i32/train/{k}", v)
        # (the same label map inside a wider one: the strided form of every label reader)
        wide = place(label_np["i64"], off)
        for k, v in data.prepare_sample(dict(raw, disparity=place(gt_np, off), label=wide[:, :H, :W]), True,
                                          keys=[k for k in keys("us3d", True) if k.startswith("label")]).items():
            put(f"{name}/prepare_sample/i64_strided/train/{k}", v)
        if prep_only:
            return
        # ---- inputs of the objective and the evaluation
        gt = place(gt_np, off)
        ests = [place(gt_np + u((B, H, W), 10 + i, -6, 6) * (1 + i), off) for i in range(4)]
        en = ests[1].cpu().numpy().copy()
        en.reshape(-1)[1] = np.nan
        ests_m = [ests[0], place(en, off), ests[2], ests[3]]                    # (what the metrics get: a NaN error among them)
        h4, w4 = max(1, H // 4), max(1, W // 4)
        gt4 = place(u((B, h4, w4), 20, -80, 80), off)
        ests4 = [place(gt4.cpu().numpy() + u((B, h4, w4), 21 + i, -2, 2), off) for i in range(2)]
        mask = place(u((B, H, W), 30) > -0.5, off)
        mask_img = place(u((B, H, W), 31) > 0.0, off)
        z_np = detdata.normalish((B, 6, H, W), s + 40)
        z = place(z_np, off)                                                   # (finite: the losses)
        z_np = z_np.copy()
        zf = z_np.reshape(B, 6, -1)
        zf[0, 2, 0] = zf[0, 1, 0] = zf[0].max() + 1                            # equal maxima, a NaN first, a NaN later, all NaN
        zf[0, 0, 1] = np.nan
        zf[0, 4, 2] = np.nan
        zf[0, :, 3] = np.nan
        zn = place(z_np, off)                                                  # (what the arg-max readers get)
        zr = place(detdata.normalish((B, 6, H, W), s + 41), off)
        disp = place(u((B, H, W), 42, -3.0, float(W)), off)
        disp.view(-1)[2] = float("nan")

        def grads(loss, leaves, key):
            put(f"{key}/loss", loss)
            for i, g in enumerate(torch.autograd.grad(loss, leaves)):
                put(f"{key}/grad{i}", g)

        def leaves(ts):
            return [t.detach().requires_grad_(True) for t in ts]
        # ---- losses
        e = leaves(ests)
        grads(losses.model_loss_train(e, [gt] * 4, [mask] * 4), e, f"{name}/model_loss_train")
        e = leaves(ests[:1])
        grads(losses.model_loss_test(e, [gt], [mask]), e, f"{name}/model_loss_test")
        for lk, y in label_np.items():
            y = place(y[:, :H, :W], off)
            e = leaves([z])
            grads(losses.model_label_loss(e[0], y, 6, False), e, f"{name}/model_label_loss/{lk}")
            e = leaves([zr])
            warped = torch.empty((B, H, W), dtype=torch.int64, device=dev)
            grads(losses.LRSC_loss(e[0], [disp], y, warped=warped), e, f"{name}/LRSC_loss/{lk}")
            put(f"{name}/LRSC_loss/{lk}/warped", warped)
            e = leaves([ests[0], ests4[0], ests[1], ests4[1], z, zr])
            out = losses.train_objective(e[:4], e[4], e[5], gt, gt4, y, 64, True)
            for i, v in enumerate(out[1:]):
                put(f"{name}/train_objective/{lk}/term{i}", v)
            grads(out[0], e, f"{name}/train_objective/{lk}")
        # ---- metrics
        for n in (1, 2, 3, 4):
            for form, kw in (("mask", dict(mask=mask, mask_img=mask_img)), ("range", dict(maxdisp=64, thresholds=(1.0, 2.0, 3.0)))):
                out, rec = metrics.disparity_metrics(ests_m[:n], gt, return_record=True, **kw)
                put(f"{name}/disparity_metrics/{n}/{form}/out", out)
                put(f"{name}/disparity_metrics/{n}/{form}/counts", rec["counts"])
                put(f"{name}/disparity_metrics/{n}/{form}/sums", rec["sums"])
        label_dev = {lk: place(y[:, :H, :W], off) for lk, y in label_np.items()}
        label_dev["i64_strided"] = wide
        for lk, y in label_dev.items():
            m = metrics.SegmentationMetric(6)
            m.addBatch(zn, y)
            m.addBatch(z, y)
            put(f"{name}/confusion/{lk}", m._joint)
            for n in (1, 2, 3, 4):
                for form, kw in (("mask", dict(mask=mask)), ("range", dict(maxdisp=64, thresholds=(1.0, 2.0, 3.0, 4.0), tau=2.5))):
                    for k, v in joint_metrics.joint_metrics(ests_m[:n], zn, gt, y, **kw).items():
                        put(f"{name}/joint_metrics/{lk}/{n}/{form}/{k}", v)
            for k, v in joint_metrics.joint_metrics(ests_m[:2], None, gt, y, maxdisp=64).items():
                put(f"{name}/joint_metrics/{lk}/2/no_logits/{k}", v)
            for dk, dt in (("f32", torch.float32), ("u8", torch.uint8)):
                put(f"{name}/label_vis/{lk}/{dk}", visualization.label_vis(y if lk != "i64_strided" else y[:, :H, :W], dt))
        # ---- pictures
        put(f"{name}/error_image", visualization.disp_error_image(ests[0], gt))
        put(f"{name}/error_image/nan", visualization.disp_error_image(ests_m[1], gt, legend=False))
        put(f"{name}/error_image/signed", visualization.disp_error_image(ests[2], gt, abs_thres=2.0, rel_thres=0.1, signed=True, valid_range=(-64.0, 64.0)))
        for dk, dt in (("f32", torch.float32), ("u8", torch.uint8)):
            put(f"{name}/feature_vis/6/{dk}", visualization.feature_vis(zn, dt))
            put(f"{name}/feature_vis/3/{dk}", visualization.feature_vis(place(z_np[:, :3], off), dt))
        put(f"{name}/normalize_image/3", visualization.normalize_image(place(u((B, 3, H, W), 50, -5, 9), off)))
        put(f"{name}/normalize_image/1", visualization.normalize_image(gt))
        put(f"{name}/normalize_image/const", visualization.normalize_image(torch.full((B, 2, H, W), 0.25, device=dev)))

    for case in CASES:
        run_case(*case, prep_only=False)
    for case in PREP_ONLY:
        run_case(*case, prep_only=True)
    torch.cuda.synchronize()
    groups = {}                                                                # shape / function -> the digests of all its outputs
    for key in sorted(digests):
        groups.setdefault("/".join(key.split("/")[:2]), hashlib.sha256()).update(f"{key} {digests[key]}\n".encode())
    res = {"digests": digests if args.each else {k: h.hexdigest() for k, h in groups.items()}, "outputs": len(digests),
           "paths": {k: v for k, v in sorted(_host.PATH_COUNTS.items()) if v}}
    text = json.dumps(res, indent=1, sort_keys=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text if not args.out else json.dumps({"stream_digest": {"outputs": len(digests), "paths": res["paths"],
                                                                  "all": hashlib.sha256(text.encode()).hexdigest()}}))


if __name__ == "__main__":
    main()
