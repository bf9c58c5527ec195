"""Per-call checker of the training step (test tooling, imported by tests/test_train_calls_gpu.py and tools/err_train_step.py): every HIP
function a train() step calls is wrapped at the name its call site reads, and each call is compared with a float64 restatement of the
same operation ON THAT CALL'S OWN INPUTS.  A whole-step float64 comparison cannot do this at full size: ReLU flips and top-k picks turn
fp32 rounding into gradient differences of ~5e-3 (EXPERIMENTS.md F.7).  Per call, only continuous arithmetic goes to float64; the
discontinuities are decided like for like, from the HIP call itself:

  * BatchNorm + ReLU: the mask is the HIP forward's `y > 0`.  A float64 pre-activation on the other side of zero is counted, and allowed
    only within the seam's bound of zero.
  * top-k picks (_TopkCandidates): forced to the HIP picks.  Pixels whose float64 picks differ are counted, and allowed only where the
    float64 24th / 25th probabilities are within cases.DELTA24_REL.  (_RegressionTopk decides on its fp32 input, which float64 orders
    exactly: its picks are the same by construction.)
  * warp taps (_ConcatVolumeSampled, _SampleStrength, _WarpSampled): the coordinates keep grid_sample's fp32 normalise / unnormalise round
    trip, as the kernels form them (warp.hip); the bilinear weights and sums are float64.

Error of a call = max|hip - ref64| / max|ref64| per output (the scale the small-shape tests use); for activations and data gradients of
the convolutions also relative to the per-output-channel rms (reported, not asserted).  A call above its seam's bound passes only if the
same reference in float32 on the CPU, same inputs and decisions, misses float64 by at least 1/1.5 of the HIP error: conditioning, reported.
"""
import collections
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from golden import cases
from oracle import ops as oops

# ---- the seams ---------------------------------------------------------------------------------------------------------------------

#: functions of semstereo_amd/train_layers.py that _Conv3dK3 / _Deconv3dK3 reach through the module's globals
LEAF_SEAMS = ("_conv_k3_forward", "_deconv_k3_forward", "conv3d_wgrad_hip")
#: autograd Functions (module, class) whose forward and backward are HIP launches
FUNCTION_SEAMS = (
    ("train", "_BatchNormTrain"), ("train", "_ConvK1"), ("train", "_Conv2dK3"), ("train", "_DepthwisePatch"), ("train", "_ChannelGate"),
    ("train", "_WindowAttentionCore"), ("train", "_UpsampleSoftmaxRegression"), ("train", "_SampleStrength"), ("train", "_TopkCandidates"),
    ("train", "_ConcatVolumeSampled"), ("ops", "_GwcVolume"), ("ops", "_GroupNormalise"), ("ops", "_WarpSampled"), ("ops", "_RegressionTopk"),
)
#: what one train() step of the hot segment (features with gradients) must reach.  _BatchNormEval is not in it: it runs only under eval()
#: with autograd (tests/test_parity_gpu.py::test_training_kernels_vs_float64_autograd); nor _WarpSampled: the step's warps are the fused
#: tail and concat volume.
STEP_SEAMS = frozenset({
    "train_layers._conv_k3_forward", "train_layers._deconv_k3_forward", "train_layers.conv3d_wgrad_hip", "modules.conv3d_wgrad_hip",
    "train._BatchNormTrain", "train._ConvK1", "train._Conv2dK3", "train._DepthwisePatch", "train._ChannelGate", "train._WindowAttentionCore",
    "train._UpsampleSoftmaxRegression", "train._SampleStrength", "train._TopkCandidates", "train._ConcatVolumeSampled", "ops._GwcVolume",
    "ops._GroupNormalise", "ops._RegressionTopk",
})

#: bound per (seam, part) -- the bound the seam's small-shape test asserts (tests/test_parity_gpu.py), as max|err| / max|ref|.  Where that
#: test asserts atol + rtol * max|ref| on O(1) data, the bound is atol + rtol.  tests/test_bwd_paths_gpu.py holds _UpsampleSoftmaxRegression,
#: _SampleStrength (both forms of its backward), _TopkCandidates, _GwcVolume and _GroupNormalise to these same entries on every
#: shape-dependent path of their backward kernels (row buffers, the thread-per-element volume kernel, zero groups, NULL gradients).
BOUNDS = {
    "train_layers._conv_k3_forward": {"fwd": 2e-6},                          # test_conv3d_training_forward_dgrad_wgrad_in_hip
    "train_layers._deconv_k3_forward": {"fwd": 2e-6},                        # ... and test_deconv3d_training_...
    "train_layers.conv3d_wgrad_hip": {"fwd": 5e-6},
    "modules.conv3d_wgrad_hip": {"fwd": 5e-6},
    "train._BatchNormTrain": {"fwd": 2e-5, "bwd": 2e-5},                     # test_training_kernels_vs_float64_autograd
    "train._ConvK1": {"fwd": 2e-5, "bwd": 2e-5},
    "train._Conv2dK3": {"fwd": 2e-5, "bwd": 2e-5},
    "train._DepthwisePatch": {"fwd": 2e-5, "bwd": 2e-5},
    "train._ChannelGate": {"fwd": 2e-5, "bwd": 2e-5},
    "train._WindowAttentionCore": {"fwd": 2e-5, "bwd": 5e-5},
    "train._UpsampleSoftmaxRegression": {"fwd": 2e-5, "bwd": 2e-5},          # test_attention_tail_training_functions_vs_float64_autograd
    "train._SampleStrength": {"fwd": 2e-5, "bwd": 5e-5},
    "train._TopkCandidates": {"fwd": 2e-5, "bwd": 5e-5},
    "train._ConcatVolumeSampled": {"fwd": 4e-6, "bwd": 1.3e-5},              # test_concat_volume_training_one_launch_each_way
    "ops._GwcVolume": {"fwd": 2e-6, "bwd": 2e-5},                            # test_gwc*, test_backward_gwc_concat_regression
    "ops._GroupNormalise": {"fwd": 2e-5, "bwd": 2e-5},
    "ops._WarpSampled": {"fwd": 2e-6, "bwd": 4e-5},                          # test_backward_warp_*
    "ops._RegressionTopk": {"fwd": 2e-6, "bwd": 3e-6},
}
#: SS_CONV_ENGINE=f32 / bf16x6 (not the default f16x3): a 3x3x3 convolution over 128 input channels (K = 3456 products per output,
#: hourglass_att's coarsest levels) measures 2.1-2.6e-6 of max|ref| at every size from 6 x 8 x 8 up, 1e-5 of the channel rms, where
#: float32 on the CPU reaches 3-5e-7: the engines' fp32 accumulation along K, not a grid or shape effect (64 channels: 1.9e-6).  An open
#: finding of those two engines, held to this bound so that anything worse still fails; f16x3 and every other layer keep 2e-6.
K128_CONV_BOUND = {"f32": 3e-6, "bf16x6": 3e-6}
#: outputs whose rms-per-channel error is reported too: activations and data gradients of the convolutions
RMS_SEAMS = {"train_layers._conv_k3_forward", "train_layers._deconv_k3_forward"}


# ---- float64 references (device- and dtype-generic: the CPU tests run them in float64 against F.*, the checker on the GPU) ------------

def conv_ref(x, w, stride):
    return F.conv3d(x, w, None, stride, 1)


def deconv_ref(x, w):
    return F.conv_transpose3d(x, w, None, stride=2, padding=1, output_padding=1)


def wgrad_ref(grad_out, x, Cout, Cin, stride):
    return torch.nn.grad.conv3d_weight(x, (Cout, Cin, 3, 3, 3), grad_out, stride, 1)


def _cshape(x):
    return (1, -1) + (1,) * (x.dim() - 2)


def batchnorm_ref(x, weight, bias, eps, relu, residual, mask=None):
    """(y, mean, unbiased var) of BatchNorm on batch statistics [+ residual] [-> ReLU]; the ReLU keeps `mask` (a 0/1 tensor: the HIP
    forward's y > 0) where given, the sign of the pre-activation otherwise."""
    dims = [0] + list(range(2, x.dim()))
    n = x.numel() // x.shape[1]
    mean = x.mean(dims, keepdim=True)
    var = ((x - mean) ** 2).mean(dims, keepdim=True)
    z = (x - mean) / torch.sqrt(var + eps)
    if weight is not None:
        z = z * weight.reshape(_cshape(x))
    if bias is not None:
        z = z + bias.reshape(_cshape(x))
    if residual is not None:
        z = z + residual
    y = z
    if relu:
        y = z * (z > 0).to(z.dtype) if mask is None else z * mask.to(z.dtype)
    return y, mean.reshape(-1), (var * n / max(n - 1, 1)).reshape(-1), z


def k1_ref(x, w, bias):
    w = w.reshape(w.shape[0], w.shape[1], *([1] * (x.dim() - 2)))
    return (F.conv3d if x.dim() == 5 else F.conv2d)(x, w, bias)


def conv2d_k3_ref(x, w):
    return F.conv2d(x, w, None, 1, 1)


def patch_ref(x, w):
    return F.conv3d(x, w, None, 1, (0, 1, 1), 1, x.shape[1])


def gate_ref(att, cv):
    return torch.sigmoid(att).unsqueeze(2) * cv


def window_core_ref(qkv, bqkv, heads, block):
    """softmax(q k^T / sqrt(hd) [+ pad mask]) v per (window, head) of a [B,3C,D,H,W] qkv volume: H, W padded to window multiples with
    tokens whose q / k / v are the Linear's bias `bqkv` (the reference pads the volume before the Linear), the -1000 mask between real and
    pad tokens with the reference's `-0:` quirk (oracle/stack.py attention_block), cropped back."""
    B, C3, D, H0, W0 = qkv.shape
    C = C3 // 3
    hd = C // heads
    bd, bh, bw = block
    pad_r, pad_b = (bw - W0 % bw) % bw, (bh - H0 % bh) % bh
    H, W = H0 + pad_b, W0 + pad_r
    if pad_r or pad_b:
        full = bqkv.to(qkv.dtype).reshape(1, C3, 1, 1, 1).expand(B, C3, D, H, W)
        keep = torch.zeros((H, W), dtype=torch.bool, device=qkv.device)
        keep[:H0, :W0] = True
        qkv = torch.where(keep, F.pad(qkv, (0, pad_r, 0, pad_b)), full)
    nd, nh, nw = D // bd, H // bh, W // bw
    T = bd * bh * bw
    tok = qkv.reshape(B, C3, nd, bd, nh, bh, nw, bw).permute(0, 2, 4, 6, 3, 5, 7, 1).reshape(B, nd * nh * nw, T, C3)
    tok = tok.reshape(B, nd * nh * nw, T, 3, heads, hd).permute(3, 0, 1, 4, 2, 5)
    q, k, v = tok[0], tok[1], tok[2]
    logits = torch.matmul(q, k.transpose(-2, -1)) * (hd ** -0.5)
    if pad_r > 0 or pad_b > 0:
        is_pad = torch.zeros((H, W), dtype=qkv.dtype, device=qkv.device)
        is_pad[(H - pad_b) if pad_b > 0 else 0:, :] = 1
        is_pad[:, (W - pad_r) if pad_r > 0 else 0:] = 1
        flag = is_pad.reshape(nh, bh, nw, bw).permute(0, 2, 1, 3).reshape(nh * nw, bh * bw)
        differs = (flag.unsqueeze(1) != flag.unsqueeze(2)).to(qkv.dtype) * -1000.0
        logits = logits + differs.repeat(nd, bd, bd).reshape(1, nd * nh * nw, 1, T, T)
    y = torch.matmul(torch.softmax(logits, dim=-1), v)
    y = y.reshape(B, nd, nh, nw, heads, bd, bh, bw, hd).permute(0, 4, 8, 1, 5, 2, 6, 3, 7).reshape(B, C, D, H, W)
    return y[:, :, :, :H0, :W0]


def _values(rng, like):
    dmin, nd = rng
    return torch.arange(dmin, dmin + nd, dtype=like.dtype, device=like.device).reshape(1, nd, 1, 1)


def upsoft_ref(coarse, H, W, rng):
    """:279-285: trilinear 2x up-sampling, softmax over D, expectation and variance over the disparities of `rng` = (dmin, nd)."""
    up = F.interpolate(coarse, [rng[1], H, W], mode="trilinear")
    p = torch.softmax(up.squeeze(1), dim=1)
    vals = _values(rng, p)
    disp = (p * vals).sum(dim=1)
    var = (p * (vals - disp.unsqueeze(1)) ** 2).sum(dim=1, keepdim=True)
    return up, disp, var


def warp_coords32(d, H, W):
    """(ix, iy) of grid_sample(align_corners=True) at column w - d, row h, in fp32 through the normalise / unnormalise round trip exactly
    as warp.hip forms them (ix = ((w - d) / half_w - 1 + 1) * half_w, half_w = (float)((W - 1.0) / 2.0)) -- on the CPU, IEEE fp32."""
    d = d.detach().float().cpu()
    hw = torch.full_like(d, float(np.float32((W - 1.0) / 2.0)))
    hh = torch.full_like(d, float(np.float32((H - 1.0) / 2.0)))
    cols = torch.arange(W, dtype=torch.float32).reshape(1, 1, 1, W).expand_as(d)
    rows = torch.arange(H, dtype=torch.float32).reshape(1, 1, H, 1).expand_as(d)
    ix = ((cols - d) / hw - 1.0 + 1.0) * hw
    iy = (rows / hh - 1.0 + 1.0) * hh
    return ix, iy


def warp_ref(y, d, d_grad=None):
    """Bilinear samples of y [B,C,H,W] at (w - d, h) -> [B,C,nd,H,W], zeros outside: the taps and their floor from the fp32 coordinates
    (warp_coords32), weights and sums in y's dtype; differentiable in y, and in `d_grad` (d itself, carrying a gradient: dix/dd = -1)."""
    B, C, H, W = y.shape
    nd = d.shape[1]
    ix32, iy32 = warp_coords32(d, H, W)
    x0, y0 = ix32.floor(), iy32.floor()
    ix, iy = ix32.to(y), iy32.to(y)
    if d_grad is not None:
        ix = ix - (d_grad - d_grad.detach()).to(y.dtype)
    fx, fy = ix - x0.to(y), iy - y0.to(y)
    x0, y0 = x0.long().to(y.device), y0.long().to(y.device)
    flat = y.reshape(B, C, H * W)
    out = None
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):                 # nw, ne, sw, se
        xx, yy = x0 + dx, y0 + dy
        valid = ((xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)).to(y.dtype)
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).reshape(B, 1, nd * H * W).expand(B, C, nd * H * W)
        v = torch.gather(flat, 2, idx).reshape(B, C, nd, H, W)
        wgt = ((fx if dx else 1.0 - fx) * (fy if dy else 1.0 - fy) * valid).unsqueeze(1)
        out = v * wgt if out is None else out + v * wgt
    return out


def strength_ref(left, right, pred0, var, gamma, beta):
    """:286-293: softmax over the 5 propagated candidates of mean_c(left * warp(right)) * propagated sigmoid(beta + gamma * var)."""
    v = torch.sigmoid(beta + gamma * var)
    cand = oops.propagation(pred0.unsqueeze(1))
    rw = warp_ref(right, cand, cand)
    return torch.softmax((left.unsqueeze(2) * rw).mean(dim=1) * oops.propagation(v), dim=1)


def topk_ref(logits, strength, k, rng, samples):
    """:295-310 on the given picks `samples` [B,k,H,W] (disparities, ascending): (att_topk, pred_att, own float64 picks, 24th/25th gap)."""
    aw = (oops.propagation_prob(logits) * strength.unsqueeze(2)).sum(dim=1, keepdim=True)
    prob = torch.softmax(aw, dim=2)
    ind = (samples.detach().to(torch.int64) - int(rng[0])).unsqueeze(1).to(logits.device)
    att = torch.gather(prob, 2, ind)
    smp = samples.detach().to(logits)
    pred = (torch.softmax(torch.gather(aw, 2, ind).squeeze(1), dim=1) * smp).sum(dim=1)
    with torch.no_grad():
        srt, order = prob.squeeze(1).sort(dim=1, descending=True, stable=True)
        own = order[:, :k].sort(dim=1).values + int(rng[0])
        gap = ((srt[:, k - 1] - srt[:, k]) / srt[:, k - 1]) if prob.shape[2] > k else torch.ones_like(srt[:, 0])
    return att, pred, own, gap


def concat_ref(left, right, samples, att):
    """:316-318: att * cat(left broadcast over the candidates, warp(right) at the candidates) -> [B,2C,nd,H,W]."""
    B, C, H, W = right.shape
    nd = samples.shape[1]
    a = att.reshape(B, 1, nd, H, W)
    return torch.cat((left.unsqueeze(2).expand(B, C, nd, H, W), warp_ref(right, samples)), dim=1) * a


def gwc_ref(ref, tgt, rng, groups):
    """V[b,g,i,y,x] = mean over the group's channels of ref[..,x] * tgt[..,x-d], d = dmin + i, zero where x - d leaves the image."""
    B, C, H, W = ref.shape
    dmin, nd = rng
    planes = []
    for i in range(nd):
        d = dmin + i
        if abs(d) >= W:
            planes.append(ref.new_zeros((B, groups, H, W)))
            continue
        if d >= 0:
            p = (ref[..., d:] * tgt[..., :W - d]).reshape(B, groups, C // groups, H, W - d).mean(dim=2)
            planes.append(F.pad(p, (d, 0)))
        else:
            p = (ref[..., :W + d] * tgt[..., -d:]).reshape(B, groups, C // groups, H, W + d).mean(dim=2)
            planes.append(F.pad(p, (0, -d)))
    return torch.stack(planes, dim=2)


def group_normalise_ref(x, groups):
    B, C, H, W = x.shape
    v = x.reshape(B, groups, C // groups, H, W)
    return (v / (torch.linalg.vector_norm(v, 2, dim=2, keepdim=True) + 1e-05)).reshape(B, C, H, W)


def warp_sampled_ref(x, y, disp):
    nd = disp.shape[1]
    return warp_ref(y, disp, disp), x.unsqueeze(2).expand(x.shape[0], x.shape[1], nd, x.shape[2], x.shape[3])


def regression_topk_ref(cost, samples, k):
    return oops.regression_topk(cost, samples, k)


# ---- one Function's forward, restated: (outputs, decisions) from the call's inputs and its HIP outputs -----------------------------

def function_ref(name, args, hip_out):
    """Float64 (or whatever dtype `args` carry) restatement of Function `name`'s forward on `args` (the forward's arguments after ctx),
    with the HIP call's discontinuous decisions taken from `hip_out`.  -> (tuple of outputs aligned with hip_out (None where not
    compared), dict of decision counts)."""
    dec = {}
    if name == "train._BatchNormTrain":
        x, w, b, eps, relu, res = args[:6]
        mask = (hip_out[0] > 0) if relu else None
        y, mean, var_u, z = batchnorm_ref(x, w, b, eps, relu, res, None if mask is None else mask.to(x.device))
        if relu:
            with torch.no_grad():
                zz = z.detach()
                flip = (zz > 0) != mask.to(zz.device)
                tol = BOUNDS[name]["fwd"] * float(zz.abs().max())
                dec = {"flips": int(flip.sum()), "unexplained": int((flip & (zz.abs() > tol)).sum())}
        return (y, mean, var_u), dec
    if name == "train._ConvK1":
        return (k1_ref(*args),), dec
    if name == "train._Conv2dK3":
        return (conv2d_k3_ref(*args),), dec
    if name == "train._DepthwisePatch":
        return (patch_ref(*args),), dec
    if name == "train._ChannelGate":
        return (gate_ref(*args),), dec
    if name == "train._WindowAttentionCore":
        return (window_core_ref(*args),), dec
    if name == "train._UpsampleSoftmaxRegression":
        up, disp, var = upsoft_ref(*args)
        return (up, disp.reshape(hip_out[1].shape), var.reshape(hip_out[2].shape)), dec
    if name == "train._SampleStrength":
        return (strength_ref(*args),), dec
    if name == "train._TopkCandidates":
        logits, strength, k, rng = args
        att, pred, own, gap = topk_ref(logits, strength, k, rng, hip_out[1])
        with torch.no_grad():
            other = (own.to(hip_out[1].device) != hip_out[1].to(torch.int64)).any(dim=1)
            gap = gap.to(other.device)
            dec = {"flips": int(other.sum()), "unexplained": int((other & (gap >= cases.DELTA24_REL)).sum())}
        return (att.reshape(hip_out[0].shape), None, pred.reshape(hip_out[2].shape)), dec
    if name == "train._ConcatVolumeSampled":
        return (concat_ref(*args[:4]),), dec
    if name == "ops._GwcVolume":
        return (gwc_ref(*args),), dec
    if name == "ops._GroupNormalise":
        return (group_normalise_ref(*args),), dec
    if name == "ops._WarpSampled":
        return warp_sampled_ref(*args), dec
    if name == "ops._RegressionTopk":
        return (regression_topk_ref(*args),), dec
    raise KeyError(f"no reference for {name}")


# ---- metric -------------------------------------------------------------------------------------------------------------------------

def rel_err(a, ref, scale=None):
    """max|a - ref| / max|ref| (or / `scale`), in float64."""
    a, ref = a.detach(), ref.detach()
    if not ref.numel():
        return 0.0
    if a.device != ref.device:
        a = a.to(ref.device)
    d = float((a.double() - ref.double()).abs().max())
    return d / ((float(ref.double().abs().max()) if scale is None else scale) + 1e-300)


def rms_err(a, ref):
    """max over output channels (axis 1) of max|a - ref| / rms(ref) of that channel."""
    a, ref = a.detach().double().to(ref.device), ref.detach().double()
    dims = [0] + list(range(2, ref.dim()))
    d = (a - ref).abs().amax(dim=dims)
    rms = ref.pow(2).mean(dim=dims).sqrt()
    return float((d / (rms + 1e-300)).max())


def _shape_key(t):
    return "x".join(str(s) for s in t.shape) if isinstance(t, torch.Tensor) else str(t)


def _clone(a):
    return a.detach().clone() if isinstance(a, torch.Tensor) else a


def _cast(a, dtype, device, grad=False):
    if isinstance(a, torch.Tensor) and a.is_floating_point():
        t = a.detach().to(device=device, dtype=dtype)
        return t.requires_grad_(grad)
    if isinstance(a, torch.Tensor):
        return a.detach().to(device)
    return a


# ---- the recorder -------------------------------------------------------------------------------------------------------------------

class Recorder:
    """Wraps every seam (monkeypatch), checks each call in float64 as it happens, keeps the worst error per (seam, part, shape).
    `first_per_shape`: check only the first call per distinct (seam, part, input shapes) -- every call is still counted.
    `perturb`: {seam: fn(part, hip_outputs) -> hip_outputs} applied to the HIP result before it is checked and handed on (the
    checker's self-test); numbers only."""

    def __init__(self, sa, first_per_shape=False, perturb=None, ref_dtype=torch.float64):
        self.sa, self.first_per_shape, self.perturb, self.dtype = sa, first_per_shape, dict(perturb or {}), ref_dtype
        self.calls = collections.Counter()          # (seam, part) -> calls seen
        self.checked = collections.Counter()        # (seam, part) -> calls checked
        self.worst = {}                             # (seam, part, shape) -> entry
        self.findings = []                          # entries above their bound, not explained by conditioning
        self.conditioning = []                      # entries above their bound, explained by conditioning
        self.decisions = collections.Counter()      # seam -> decided differently (flips / other picks)
        self.unexplained = collections.Counter()    # seam -> decided differently where float64 is not within rounding of the edge
        self._seen = set()

    # -- installation --
    def install(self, monkeypatch):
        TL, M = self.sa.train_layers, self.sa.modules
        for name in LEAF_SEAMS:
            monkeypatch.setattr(TL, name, self._leaf("train_layers." + name, getattr(TL, name)))
        monkeypatch.setattr(M, "conv3d_wgrad_hip", self._leaf("modules.conv3d_wgrad_hip", M.conv3d_wgrad_hip))
        for modname, cls_name in FUNCTION_SEAMS:
            cls = getattr(getattr(self.sa, modname), cls_name)
            seam = f"{modname}.{cls_name}"
            monkeypatch.setattr(cls, "forward", staticmethod(self._fwd(seam, cls.forward)))
            monkeypatch.setattr(cls, "backward", staticmethod(self._bwd(seam, cls.backward)))
        return self

    def _want(self, seam, part, args):
        key = (seam, part) + tuple(_shape_key(a) for a in args if isinstance(a, torch.Tensor))
        self.calls[(seam, part)] += 1
        if self.first_per_shape and key in self._seen:
            return False
        self._seen.add(key)
        return True

    def _leaf(self, seam, real):
        rec = self

        def wrapped(*args):
            want = rec._want(seam, "fwd", args)
            ins = [_clone(a) for a in args] if want else None
            out = real(*args)
            if seam in rec.perturb:
                out = rec.perturb[seam]("fwd", out)
            if want:
                rec._check_leaf(seam, ins, out)
            return out
        wrapped.__wrapped__ = real
        return wrapped

    def _fwd(self, seam, real):
        rec = self

        def forward(ctx, *args):
            want = rec._want(seam, "fwd", args)
            ins = [_clone(a) for a in args]
            if seam == "train._BatchNormTrain" and len(args) > 6 and args[6] is not None:
                ins[6] = tuple(_clone(s) for s in args[6])               # running statistics before the kernel moves them
            out = real(ctx, *args)
            outs = out if isinstance(out, tuple) else (out,)
            if seam in rec.perturb:
                outs = rec.perturb[seam]("fwd", outs)
                out = outs if isinstance(out, tuple) else outs[0]
            ctx._tc = (ins, tuple(_clone(o) for o in outs))
            if want:
                rec._check_function_fwd(seam, ins, outs, args)
            return out
        forward.__wrapped__ = real
        return forward

    def _bwd(self, seam, real):
        rec = self

        def backward(ctx, *grads):
            ins, outs = ctx._tc
            want = rec._want(seam, "bwd", [a for a in ins if isinstance(a, torch.Tensor)])
            g_in = tuple(_clone(g) for g in grads)
            res = real(ctx, *grads)
            if seam in rec.perturb:
                res = tuple(rec.perturb[seam]("bwd", res))
            if want:
                rec._check_function_bwd(seam, ins, outs, g_in, res)
            del ctx._tc
            return res
        backward.__wrapped__ = real
        return backward

    # -- judging --
    def _judge(self, seam, part, shape, hip, ref, ref32_fn, rms=False, scale=None, bound=None):
        bound = BOUNDS[seam][part] if bound is None else bound
        e = rel_err(hip, ref, scale)
        entry = {"seam": seam, "part": part, "shape": shape, "err": e, "bound": bound,
                 "ref_max": float(ref.detach().abs().max()) if ref.numel() else 0.0, "hip_max": float(hip.detach().abs().max()) if hip.numel() else 0.0}
        if rms:
            entry["err_rms"] = rms_err(hip, ref)
        if e > bound:
            r32 = ref32_fn()
            e32 = rel_err(r32, ref, scale)
            entry["err_f32_cpu"] = e32
            if e32 >= e / 1.5:
                entry["conditioning"] = True
                self.conditioning.append(entry)
            else:
                self.findings.append(entry)
        k = (seam, part, shape)
        if k not in self.worst or e > self.worst[k]["err"]:
            self.worst[k] = entry
        return entry

    def _ref_dev(self, args):
        for a in args:
            if isinstance(a, torch.Tensor):
                return a.device
        return torch.device("cpu")

    def _check_leaf(self, seam, ins, out):
        self.checked[(seam, "fwd")] += 1
        name = seam.split(".", 1)[1]
        fn = {"_conv_k3_forward": conv_ref, "_deconv_k3_forward": deconv_ref, "conv3d_wgrad_hip": wgrad_ref}[name]
        dev = self._ref_dev(ins)
        with torch.no_grad():
            ref = fn(*[_cast(a, self.dtype, dev) for a in ins])
        shape = "/".join(_shape_key(a) for a in ins if isinstance(a, torch.Tensor)) + (f"/s{ins[2]}" if name == "_conv_k3_forward" else
                                                                                        f"/s{ins[4]}" if name == "conv3d_wgrad_hip" else "")

        def ref32():
            with torch.no_grad():
                return fn(*[_cast(a, torch.float32, "cpu") for a in ins])
        bound = None
        if name == "_conv_k3_forward" and ins[1].shape[1] >= 128:
            bound = K128_CONV_BOUND.get(self.sa.modules.CONV_ENGINE)
        self._judge(seam, "fwd", shape, out, ref, ref32, rms=seam in RMS_SEAMS, bound=bound)
        del ref

    def _check_function_fwd(self, seam, ins, outs, args):
        self.checked[(seam, "fwd")] += 1
        dev = self._ref_dev(ins)
        shape = "/".join(_shape_key(a) for a in ins if isinstance(a, torch.Tensor))
        with torch.no_grad():
            refs, dec = function_ref(seam, [_cast(a, self.dtype, dev) for a in ins], outs)
        self._decided(seam, dec)
        # (the batch mean is held to the channels' spread, not to its own size: a centred channel has a mean near zero)
        std = float(refs[2].clamp(min=0).sqrt().max()) if seam == "train._BatchNormTrain" else None
        for i, (h, r) in enumerate(zip(outs, refs)):
            if r is None or h is None:
                continue

            def ref32(i=i):
                with torch.no_grad():
                    return function_ref(seam, [_cast(a, torch.float32, "cpu") for a in ins], tuple(o.cpu() for o in outs))[0][i]
            scale = max(std, float(r.abs().max())) if (std is not None and i == 1) else None
            self._judge(seam, "fwd", f"{shape}/out{i}", h, r, ref32, scale=scale)
        if seam == "train._BatchNormTrain" and len(ins) > 6 and ins[6] is not None:
            self._check_running_stats(seam, ins, refs, args[6], shape, std)

    def _check_running_stats(self, seam, ins, refs, stats_after, shape, std):
        """running_mean / running_var as F.batch_norm moves them: (1 - m) * old + m * (batch mean, unbiased batch variance)."""
        rm0, rv0, _nbt0, mom = ins[6]
        m = float(mom)
        want_m = (1.0 - m) * rm0.double() + m * refs[1].to(rm0.device)
        want_v = (1.0 - m) * rv0.double() + m * refs[2].to(rv0.device)
        self._judge(seam, "fwd", f"{shape}/running_mean", stats_after[0], want_m, lambda: want_m.float(),
                    scale=max(std, float(want_m.abs().max())))
        self._judge(seam, "fwd", f"{shape}/running_var", stats_after[1], want_v, lambda: want_v.float())

    def _grads(self, seam, ins, outs, g_in, dtype, device, hip_res):
        """d(ref outputs)/d(inputs) contracted with the incoming gradients, for the inputs the HIP backward returned a gradient for."""
        need = [isinstance(a, torch.Tensor) and a.is_floating_point() and i < len(hip_res) and hip_res[i] is not None
                for i, a in enumerate(ins)]
        xs = [_cast(a, dtype, device, grad=n) for a, n in zip(ins, need)]
        if seam == "train._BatchNormTrain" and len(xs) > 6:
            xs[6] = None
        with torch.enable_grad():
            refs, _ = function_ref(seam, xs, tuple(o.to(device) if isinstance(o, torch.Tensor) else o for o in outs))
            pairs = [(r, g) for r, g in zip(refs, g_in) if r is not None and g is not None and r.requires_grad]
            leaves = [x for x, n in zip(xs, need) if n]
            if not pairs or not leaves:
                return [None] * len(ins)
            got = torch.autograd.grad([r for r, _ in pairs], leaves, [g.to(device=device, dtype=dtype) for _, g in pairs], allow_unused=True)
        it = iter(got)
        return [next(it) if n else None for n in need]

    def _check_function_bwd(self, seam, ins, outs, g_in, res):
        self.checked[(seam, "bwd")] += 1
        dev = self._ref_dev(ins)
        shape = "/".join(_shape_key(a) for a in ins if isinstance(a, torch.Tensor))
        refs = self._grads(seam, ins, outs, g_in, self.dtype, dev, res)
        cpu32 = {}
        for i, (h, r) in enumerate(zip(res, refs)):
            if h is None or r is None:
                continue

            def ref32(i=i):
                if "g" not in cpu32:
                    cpu32["g"] = self._grads(seam, [_cast(a, torch.float32, "cpu") if isinstance(a, torch.Tensor) else a for a in ins],
                                             tuple(o.cpu() if isinstance(o, torch.Tensor) else o for o in outs),
                                             tuple(None if g is None else g.cpu() for g in g_in), torch.float32, torch.device("cpu"), res)
                return cpu32["g"][i]
            self._judge(seam, "bwd", f"{shape}/grad{i}", h, r, ref32)

    def _decided(self, seam, dec):
        if dec:
            self.decisions[seam] += dec.get("flips", 0)
            self.unexplained[seam] += dec.get("unexplained", 0)

    # -- summary --
    def seams_checked(self):
        return {s for (s, _p), n in self.checked.items() if n > 0}

    def failures(self):
        """Seams with a call above its bound (not conditioning) or a decision the float64 value does not put within rounding of the edge."""
        bad = {e["seam"] for e in self.findings}
        bad |= {s for s, n in self.unexplained.items() if n > 0}
        return bad

    def report(self):
        per_seam = {}
        for (seam, part, shape), e in self.worst.items():
            s = per_seam.setdefault(seam, {"worst": 0.0, "bound": {}, "shapes": {}})
            s["bound"][part] = BOUNDS[seam][part]
            s["worst"] = max(s["worst"], e["err"])
            s["worst_over_bound"] = max(s.get("worst_over_bound", 0.0), e["err"] / e["bound"])
            s["shapes"][f"{part}:{shape}"] = {k: v for k, v in e.items() if k not in ("seam", "part", "shape")}
        for seam, s in per_seam.items():
            s["calls"] = {p: n for (sm, p), n in self.calls.items() if sm == seam}
            s["checked"] = {p: n for (sm, p), n in self.checked.items() if sm == seam}
            s["decided_differently"] = self.decisions.get(seam, 0)
            s["decided_differently_unexplained"] = self.unexplained.get(seam, 0)
        return {"seams": per_seam, "findings": self.findings, "conditioning": self.conditioning}


#: where the JSON report goes: $SS_TEST_REPORT_DIR/train_calls_report.json, by default test_reports/ at the repository root (git-ignored)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def report_path():
    return os.path.join(os.environ.get("SS_TEST_REPORT_DIR") or os.path.join(ROOT, "test_reports"), "train_calls_report.json")


def write_report(key, value, path=None):
    """Merge {key: value} into the JSON report (report_path())."""
    path = path or report_path()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data[key] = value
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True, default=str)
