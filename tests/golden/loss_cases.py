"""Closed-form inputs of the training-objective fixtures (tests/golden/loss.npz): shared by make_golden_loss.py, which feeds them to
the reference's own models/loss.py, and by the tests, which feed them to semstereo_amd.losses.  Values come from oracle.detdata, so
they are the same bits wherever they are built."""
import numpy as np
import torch

from oracle import detdata as dd

NCLS = 6
# name: batch, full size, quarter size, maxdisp of the range mask (main_us3d.py:199-200), terms of the disparity loss,
# attention_weights_only, seed
CASES = {
    "b2_48x80": dict(B=2, H=48, W=80, h4=12, w4=20, maxdisp=32, terms=4, attn=False, seed=7100),
    "b1_23x41": dict(B=1, H=23, W=41, h4=5, w4=11, maxdisp=32, terms=4, attn=False, seed=7200),
    "b2_16x32_noclass": dict(B=2, H=16, W=32, h4=4, w4=8, maxdisp=32, terms=4, attn=False, seed=7300),
    "attn_only": dict(B=1, H=20, W=36, h4=5, w4=9, maxdisp=32, terms=2, attn=True, seed=7400),
    "lrsc_edges": dict(B=1, H=8, W=32, h4=2, w4=8, maxdisp=32, terms=4, attn=False, seed=7500),
    "empty_nan": dict(B=1, H=8, W=12, h4=2, w4=3, maxdisp=32, terms=4, attn=False, seed=7600),
}
FUNCTIONS = ("train", "test", "label", "lrsc")


def _labels(shape, seed):
    return torch.from_numpy(np.minimum(np.floor(dd.uniform(shape, seed, 0.0, float(NCLS))), NCLS - 1).astype(np.int64))


def _edge_disparities(H, W):
    """Rows that push x - disp below 0 and above W - 1, disparities of +-1e-9 (x - 1e-9 is x in fp32 and just below x in float64, so the
    two truncate to different columns), exact integers of both signs, halves, and a smooth ramp."""
    x = np.arange(W, dtype=np.float64)
    rows = [np.full(W, 100.0), np.full(W, -100.0), np.full(W, 1e-9), np.full(W, -1e-9), x % 5, -(x % 4), (x % 3) + 0.5, 0.37 * x - 4.0]
    return torch.from_numpy(np.stack(rows[:H]).astype(np.float32)).unsqueeze(0)


def inputs(name):
    """float32 tensors: `ests` (the model's disparity outputs: full, quarter, full, quarter), `gt`, `gt4`, `logits`, `logits_r`, and
    int64 `labels`; `maxdisp`, `attn`."""
    c = CASES[name]
    B, H, W, h4, w4, s = c["B"], c["H"], c["W"], c["h4"], c["w4"], c["seed"]
    gt, gt4 = dd.t_uniform((B, H, W), s, -40.0, 40.0), dd.t_uniform((B, h4, w4), s + 1, -40.0, 40.0)
    labels = _labels((B, H, W), s + 2)
    if name == "b2_16x32_noclass":
        labels[labels == 3] = 4                       # class 3 absent
        labels[1] = NCLS - 1                          # one image all of the ignored class
    if name == "empty_nan":
        gt, gt4 = torch.full_like(gt, 100.0), torch.full_like(gt4, -100.0)      # nothing inside [-maxdisp, maxdisp)
        labels[:] = NCLS - 1                                                      # nothing but the ignored class
    ests = []
    for i in range(c["terms"]):
        g = gt if i % 2 == 0 else gt4
        ests.append(g + 1.5 * dd.t_normalish(tuple(g.shape), s + 10 + i))        # |est - gt| on both sides of smooth-L1's knee
    if name == "lrsc_edges":
        ests[0] = _edge_disparities(H, W)
    return dict(ests=ests, gt=gt, gt4=gt4, labels=labels, logits=2.0 * dd.t_normalish((B, NCLS, H, W), s + 3),
                logits_r=2.0 * dd.t_normalish((B, NCLS, H, W), s + 4), maxdisp=c["maxdisp"], attn=c["attn"])


def range_mask(gt, maxdisp):
    return (gt < maxdisp) & (gt >= -maxdisp)            # main_us3d.py:199-200


def run(lib, name, dtype, device="cpu", grads=True):
    """run_data on the inputs of case `name`."""
    return run_data(lib, inputs(name), dtype, device, grads)


def run_data(lib, d, dtype, device="cpu", grads=True):
    """The four functions of `lib` (the reference's models/loss.py, or semstereo_amd.losses) on the inputs `d`, as main_us3d.py:199-206
    calls them.  Returns {function: (loss, [gradients of the estimates or logits])} (detached, on the CPU)."""
    cast = lambda t: t.to(device=device, dtype=dtype)                       # noqa: E731
    gt, gt4, labels = cast(d["gt"]), cast(d["gt4"]), d["labels"].to(device)
    masks = [range_mask(gt, d["maxdisp"]), range_mask(gt4, d["maxdisp"])] * 2
    gts = [gt, gt4, gt, gt4]
    out = {}
    for fn in FUNCTIONS:
        leaves = [cast(t).detach().clone().requires_grad_(grads) for t in (d["ests"] if fn in ("train", "test") else [d["logits_r" if fn == "lrsc" else "logits"]])]
        if fn == "train":
            loss = lib.model_loss_train(leaves, gts, masks)
        elif fn == "test":
            loss = lib.model_loss_test(leaves, gts, masks)
        elif fn == "label":
            loss = lib.model_label_loss(leaves[0], labels, NCLS, d["attn"])
        else:
            loss = lib.LRSC_loss(leaves[0], [cast(d["ests"][0])], labels)
        if fn == "test":
            leaves = leaves[:1]                                                 # (model_loss_test reads the first output only)
        gr = []
        if grads:
            loss.backward()
            gr = [t.grad.detach().cpu() for t in leaves]
        out[fn] = (loss.detach().cpu(), gr)
    return out
