"""Training side of the 2-D layers between the backbone and the hot segment (models/SemStereo.py:254-265): the segmentation heads
`head_l` / `head_r` and the projections `chal_0 .. chal_4` under autograd / in train(), forward and backward on this repo's kernels.

  seghead_train   segmenthead.forward (models/submodule.py:40-52): train.conv2d_k3 -> train.batchnorm_train(+ ReLU) -> `_SegheadTail`
                  (csrc/seghead_train.hip: Conv2d(32 -> C, 1x1, bias) + bilinear x2 in one launch, its three gradients in one more)
  proj_train      nn.Sequential(Conv2d(1x1, bias), BatchNorm2d): `_Proj2dK1` (ss_conv2d_k1_f16s_fwd forward and, on the transposed
                  weight, for the data gradient; ss_conv_k1_wgrad_fwd; ss_channel_sum_fwd) -> train.batchnorm_train

Opt-in: `engine.HEADS_TRAIN_HIP` (SS_HEADS_TRAIN_HIP=1), with `engine.TRAIN_HIP` and the heads' own switch on.  What the kernels are
not built for -- the geometry conditions of engine.seghead_applies / engine.run_conv2d_k1, an engine other than f16x3, CPU, float64,
non-contiguous inputs -- and a projection of fewer than `PROJ_MIN_POSITIONS` positions (measured slower than the stock layers in
every round there) keep the stock layers (`*_applies` below is False; the twins count PATH_COUNTS["torch"]).
"""
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from . import engine as E
from . import train as T
from ._host import bn_ok, count
from ._lib import ptr

#: a projection runs the kernels from this many positions (B * H * W) up.  Below it a training call -- two weight packings, six small
#: launches -- does not beat MIOpen's three GEMMs: with every projection on the kernels (profiles/heads_train_bench_unrouted.json, and an
#: earlier run of the same; profiles/EXPERIMENTS.md section K) 4096 positions and fewer lose in every round (0.61-0.77x: chal_4 at batch 4,
#: chal_3 and chal_4 at batch 1), 16384 positions are level or lose (chal_3 at batch 4: 1.02x in one run, 0.95x and slower in every round in
#: the other; chal_2 at batch 1: 0.91-0.92x, slower in every round of both), 65536 positions and more win (1.07-2.3x).
PROJ_MIN_POSITIONS = 32768


def _enabled(x):
    return (E.HEADS_TRAIN_HIP and E.TRAIN_HIP and E._heads_hip_on() and E.CONV_ENGINE == "f16x3" and isinstance(x, torch.Tensor)
            and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous())


def tail_workspace(B, C, H, W, device):
    n = _lib.query_bytes("ss_seghead_tail_workspace_bytes", B, 32, C, H, W)
    return torch.empty(max(1, n // 4), dtype=torch.float32, device=device)


# ---- the head's tail: Conv2d(32 -> C, 1x1, bias) + bilinear x2 ----------------------------------------------------------------

class _SegheadTail(torch.autograd.Function):
    """out = up2(w2 . a + bias): one launch forward, one backward (+ its fixed-order final sum); a gradient autograd does not need is
    not computed (a NULL pointer)."""

    @staticmethod
    def forward(ctx, a, w2, bias, up2):
        a = T._c(a)
        B, K, H, W = a.shape
        C = w2.shape[0]
        s = 2 if up2 else 1
        out = torch.empty((B, C, s * H, s * W), dtype=a.dtype, device=a.device)
        w2c, bc = T._c(w2.detach()), T._c(bias.detach())
        with torch.cuda.device(a.device):
            E.call("ss_seghead_tail_fwd", ptr(a), ptr(w2c), ptr(bc), ptr(out), B, K, C, H, W, int(bool(up2)))
        ctx.save_for_backward(a, w2)
        ctx.up2 = int(bool(up2))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        a, w2 = ctx.saved_tensors
        need_a, need_w, need_b = ctx.needs_input_grad[:3]
        if not (need_a or need_w or need_b):
            return None, None, None, None
        g = T._c(g)
        B, K, H, W = a.shape
        C = w2.shape[0]
        ga = torch.empty_like(a) if need_a else None
        gw = torch.empty((C, K), dtype=torch.float32, device=a.device) if need_w else None
        gb = torch.empty(C, dtype=torch.float32, device=a.device) if need_b else None
        work = tail_workspace(B, C, H, W, a.device) if (need_w or need_b) else None
        with torch.cuda.device(a.device):
            E.call("ss_seghead_tail_bwd", ptr(g), ptr(a), ptr(T._c(w2.detach())), ptr(ga), ptr(gw), ptr(gb), ptr(work), B, K, C, H, W,
                   ctx.up2)
        return ga, None if gw is None else gw.reshape(w2.shape), gb, None


def seghead_train_applies(head, x):
    # (the tail addresses one element's 32-channel map and its up-sampled logits through 32-bit offsets: its own size condition)
    return (_enabled(x) and E.seghead_applies(head, x) and bn_ok(head.conv1.bn)
            and 32 * x.shape[2] * x.shape[3] * 4 < 0x7fffffff
            and head.conv2.out_channels * (4 if head.scale_factor is not None else 1) * x.shape[2] * x.shape[3] * 4 < 0x7fffffff)


def seghead_train(head, x):
    """segmenthead.forward under autograd / in train(): 3x3 conv, BatchNorm (batch statistics in train(), frozen ones in eval()) +
    ReLU, then the tail."""
    count("hip_train")
    a = T.conv2d_k3(head.conv1.conv, x)
    a = T.batchnorm_train(head.conv1.bn, a, relu=True)
    return _SegheadTail.apply(a, head.conv2.weight, head.conv2.bias, head.scale_factor is not None)


# ---- a projection's Conv2d(1x1, bias) -------------------------------------------------------------------------------------------

class _Proj2dK1(torch.autograd.Function):
    """y = w . x + bias on the K-looped two-term fp16 1x1 kernel (scale NULL, shift = the bias); the weights change every step, so they
    are packed on the fly.  Data gradient: the same kernel on the transposed weight; weight / bias gradients: the exact-fp32 seams."""

    @staticmethod
    def forward(ctx, x, w, bias):
        x = T._c(x)
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        shift = None if bias is None else T._c(bias.detach().float())
        return E.conv2d_k1_f16s_hip(x, E.pack_conv2d_k1_weight(w), w.shape[0], None, shift, False)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = T._c(g)
        B, Cin, H, W = x.shape
        Cout = w.shape[0]
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            wt = w.detach().reshape(Cout, Cin).t().contiguous()
            gx = E.conv2d_k1_f16s_hip(g, E.pack_conv2d_k1_weight(wt), Cin, None, None, False)
        if ctx.needs_input_grad[1]:
            gw = torch.empty((Cout, Cin), dtype=torch.float32, device=g.device)
            with torch.cuda.device(g.device):
                E.call("ss_conv_k1_wgrad_fwd", ptr(g), ptr(x), ptr(gw), B, Cin, Cout, H * W)
            gw = gw.reshape(w.shape)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            sums = torch.empty(Cout, dtype=torch.float64, device=g.device)
            with torch.cuda.device(g.device):
                E.call("ss_channel_sum_fwd", ptr(g), ptr(sums), B, Cout, H * W)
            gb = sums.float()
        return gx, gw, gb


def proj_train_applies(proj, x):
    conv, bn = proj[0], proj[1]
    return (_enabled(x) and E._is_conv_k1(conv) and conv.in_channels % 8 == 0 and conv.out_channels % 8 == 0
            and x.shape[1] == conv.in_channels and x.numel() > 0
            and x.shape[0] * x.shape[2] * x.shape[3] >= PROJ_MIN_POSITIONS
            and max(conv.in_channels, conv.out_channels) * x.shape[2] * x.shape[3] * 4 < 0x7fffffff and bn_ok(bn))


def proj_train(proj, x):
    """nn.Sequential(Conv2d(1x1, bias), BatchNorm2d) under autograd / in train()."""
    count("hip_train")
    return T.batchnorm_train(proj[1], _Proj2dK1.apply(x, proj[0].weight, proj[0].bias), relu=False)
