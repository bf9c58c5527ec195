"""Training side of the 2-D decoder (models/SemStereo.py:59-86, 207-211; models/submodule.py:119-161): every Conv2x of FeatUp and of
the spx chain, and `spx2`, under autograd / in train(), forward and backward on this repo's kernels.

  conv2x_train   Conv2x.forward, the transposed concatenating form with a skip map of exactly twice the input's size:
                 `_Deconv2dK4S2` -> train.batchnorm_train(+ ReLU) -> `_Conv2dK3Cat` (the concat + 3x3 conv, the concatenation never
                 materialised) -> train.batchnorm_train(+ ReLU)
  spx2_train     the biased ConvTranspose2d(C, 6, 4, 2, 1) alone: `_Deconv2dK4S2` with the bias as the forward's shift

`_Deconv2dK4S2`: forward ss_deconv2d_bf16s_fwd (weights packed on the fly: they change every step); data gradient
ss_conv2d_k4s2_f16s_fwd (a 4x4 stride-2 convolution of the output's gradient with the same weight tensor), weight gradient
ss_deconv2d_k4s2_wgrad_fwd (csrc/deconv2d_train.hip), bias gradient ss_channel_sum_fwd.  Each of the two gradients has its own seam
(`DGRAD_HIP` / `WGRAD_HIP`) with aten.convolution_backward behind it.  `_Conv2dK3Cat`: forward ss_conv2d_bf16s_cat_fwd; data gradient
by train._Conv2dK3's recipe -- the plain 3x3 kernel on the flipped, channel-swapped weight, once per half so that each source's
gradient is written contiguously --; weight gradient from conv3d_wgrad_hip on depth-1 volumes, once per source, or, with
`engine.CONV2D_WGRAD_HIP` (SS_CONV2D_WGRAD_HIP=1, off by default), from one call of train.conv2d_k3_wgrad_hip on both sources.

Opt-in: `engine.DECODER_TRAIN_HIP` (SS_DECODER_TRAIN_HIP=1), with `engine.TRAIN_HIP`, the decoder's own switch and the f16x3 engine.
What the kernels are not built for -- a skip map of another size (the F.interpolate branch), CPU, float64, non-contiguous inputs, a
transposed conv whose channel count is not a multiple of 8 (the concat-free 3x3 needs whole chunks) -- keeps the stock layers
(`*_applies` below is False; the twins count PATH_COUNTS["torch"]).  No layer is routed back by size: none was slower than the stock
layers in every round at both measured batch sizes (profiles/EXPERIMENTS.md section L).

In train() the reference calls each Conv2x of FeatUp on the left view and then on the right view, each with its own batch statistics,
the running statistics moving twice in that order (models/SemStereo.py:74-84): the twins call conv2x_train per view, never per pair.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _lib
from . import engine as E
from . import train as T
from ._host import bn_ok, count
from ._lib import ptr

#: the two gradient seams of `_Deconv2dK4S2`: False sends that gradient to aten.convolution_backward (the other keeps its kernel)
DGRAD_HIP = True
WGRAD_HIP = True


def _enabled(*xs):
    return (E.DECODER_TRAIN_HIP and E.TRAIN_HIP and E._decoder_hip_on() and E.CONV_ENGINE == "f16x3"
            and all(isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()
                    and x.numel() > 0 for x in xs))


def _count():
    count("hip_train")
    count("decoder_train")


def pack_conv2d_k4s2_weight(w):
    """[Cout,Cin,4,4] fp32 (a ConvTranspose2d's own [its Cin, its Cout, 4, 4]) -> the fragments of ss_conv2d_k4s2_f16s_fwd."""
    Cout, Cin = w.shape[0], w.shape[1]
    assert tuple(w.shape[2:]) == (4, 4)
    return E._pack("ss_pack_conv2d_k4s2_weights_f16s", w, Cout, Cin)


def conv2d_k4s2_hip(g, wsplit, Cout):
    """Conv2d(k4, s2, p1, no bias) of g [B,Cin,H,W] (H, W even) -> [B,Cout,H/2,W/2] on the two-term fp16 engine."""
    g = T._c(g)
    dev = _lib.require_device(g)
    B, Cin, H, W = g.shape
    out = torch.empty((B, Cout, H // 2, W // 2), dtype=g.dtype, device=g.device)
    with torch.cuda.device(dev):
        E.call("ss_conv2d_k4s2_f16s_fwd", ptr(g), ptr(wsplit), ptr(out), B, Cin, H, W, Cout)
    return out


def wgrad_workspace_bytes(B, Cin, H, W, Cout):
    return _lib.query_bytes("ss_deconv2d_k4s2_wgrad_workspace_bytes", B, Cin, H, W, Cout)


def deconv2d_k4s2_wgrad_hip(x, g, Cout):
    """grad_w [Cin,Cout,4,4] of ConvTranspose2d(k4, s2, p1): x [B,Cin,H,W], g [B,Cout,2H,2W]."""
    x, g = T._c(x), T._c(g)
    dev = _lib.require_device(x, g)
    B, Cin, H, W = x.shape
    assert tuple(g.shape) == (B, Cout, 2 * H, 2 * W)
    gw = torch.empty((Cin, Cout, 4, 4), dtype=torch.float32, device=x.device)
    work = torch.empty(wgrad_workspace_bytes(B, Cin, H, W, Cout) // 4, dtype=torch.float32, device=x.device)
    with torch.cuda.device(dev):
        E.call("ss_deconv2d_k4s2_wgrad_fwd", ptr(x), ptr(g), ptr(gw), ptr(work), B, Cin, H, W, Cout)
    return gw


# ---- ConvTranspose2d(k = 4, s = 2, p = 1) [+ bias] ------------------------------------------------------------------------------

class _Deconv2dK4S2(torch.autograd.Function):
    """y = conv_transpose2d(x, w, bias, stride=2, padding=1), w [Cin,Cout,4,4]; a gradient autograd does not need is not computed."""

    @staticmethod
    def forward(ctx, x, w, bias):
        x = T._c(x)
        ctx.save_for_backward(x, w)
        ctx.has_bias = bias is not None
        shift = None if bias is None else T._c(bias.detach().float())
        return E.deconv2d_bf16s_hip(x, E.pack_deconv2d_weight(w), w.shape[1], None, shift, False)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = T._c(g)
        Cin, Cout = w.shape[0], w.shape[1]
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gx = gw = gb = None
        if need_x and DGRAD_HIP:
            gx = conv2d_k4s2_hip(g, pack_conv2d_k4s2_weight(w), Cin)
        if need_w and WGRAD_HIP:
            gw = deconv2d_k4s2_wgrad_hip(x, g, Cout)
        stock = (need_x and gx is None, need_w and gw is None, False)
        if stock[0] or stock[1]:
            sx, sw, _ = torch.ops.aten.convolution_backward(g, x, w.detach(), None, [2, 2], [1, 1], [1, 1], True, [0, 0], 1, list(stock))
            gx, gw = (sx if stock[0] else gx), (sw if stock[1] else gw)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            sums = torch.empty(Cout, dtype=torch.float64, device=g.device)
            with torch.cuda.device(g.device):
                E.call("ss_channel_sum_fwd", ptr(g), ptr(sums), g.shape[0], Cout, g.shape[2] * g.shape[3])
            gb = sums.float()
        return gx, gw, gb


# ---- cat((y, rem), 1) -> Conv2d(3x3, s1, p1, no bias), the concatenation never materialised ---------------------------------------

class _Conv2dK3Cat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, rem, w):
        y, rem = T._c(y), T._c(rem)
        ctx.save_for_backward(y, rem, w)
        B, Cs, H, W = y.shape
        Cout, Cin = w.shape[0], w.shape[1]
        nt = E._tiled_nterms()
        ws = E.pack_conv2d_weight_bf16s(w.detach(), nt)
        out = torch.empty((B, Cout, H, W), dtype=y.dtype, device=y.device)
        with torch.cuda.device(y.device):
            E.call("ss_conv2d_bf16s_cat_fwd", ptr(y), ptr(rem), None, None, ptr(ws), None, None, ptr(out), B, Cs, Cin, H, W, Cout, 0, int(nt))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        y, rem, w = ctx.saved_tensors
        M = T._M()
        g = T._c(g)
        Cs, Cout = y.shape[1], w.shape[0]
        nt = E._tiled_nterms()
        gy = grem = gw = None
        # the data gradient of a 3x3 conv: the same conv on the flipped, channel-swapped weight -- split by OUTPUT half, so that each
        # source's gradient is one contiguous tensor
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            wt = w.detach().transpose(0, 1).flip(2, 3)
            if ctx.needs_input_grad[0]:
                gy = E.conv2d_bf16s_hip(g, E.pack_conv2d_weight_bf16s(wt[:Cs].contiguous(), nt), Cs, None, None, False, nt)
            if ctx.needs_input_grad[1]:
                grem = E.conv2d_bf16s_hip(g, E.pack_conv2d_weight_bf16s(wt[Cs:].contiguous(), nt), w.shape[1] - Cs, None, None, False, nt)
        if ctx.needs_input_grad[2] and T.conv2d_k3_wgrad_applies(g, y, rem):
            gw = T.conv2d_k3_wgrad_hip(g, y, rem)           # (engine.CONV2D_WGRAD_HIP: one call, both sources, no cat and no slice copy)
        elif ctx.needs_input_grad[2]:
            # depth-1 volumes through the 3x3x3 weight-gradient kernel (its kd = 1 plane is the 3x3 gradient), once per source
            g5 = g.unsqueeze(2)
            gw = torch.cat((M.conv3d_wgrad_hip(g5, y.unsqueeze(2), Cout, Cs, 1)[:, :, 1],
                            M.conv3d_wgrad_hip(g5, rem.unsqueeze(2), Cout, rem.shape[1], 1)[:, :, 1]), 1)
        return gy, grem, gw


# ---- the layers ----------------------------------------------------------------------------------------------------------------

def _deconv_fits(conv, x):
    """The geometry conditions of the inference twin (engine.run_deconv2d), and the kernels' 32-bit offsets per element."""
    return (E._is_deconv_k4s2(conv) and x.shape[1] == conv.in_channels
            and max(conv.in_channels, 4 * conv.out_channels) * x.shape[2] * x.shape[3] * 4 < 0x7fffffff)


def conv2x_train_applies(m, x, rem):
    a, b = m.conv1, m.conv2
    return (_enabled(x, rem) and m.concat and not m.is_3d and _deconv_fits(a.conv, x) and a.conv.bias is None and a.use_bn and a.relu
            and E._is_plain_3x3(b.conv) and b.use_bn and bn_ok(a.bn) and bn_ok(b.bn)
            and a.conv.out_channels % 8 == 0 and b.conv.in_channels == a.conv.out_channels + rem.shape[1]
            and tuple(rem.shape) == (x.shape[0], rem.shape[1], 2 * x.shape[2], 2 * x.shape[3])      # (else: the F.interpolate branch)
            and b.conv.in_channels * rem.shape[2] * rem.shape[3] * 4 < 0x7fffffff)


def conv2x_train(m, x, rem):
    """Conv2x.forward (models/submodule.py:149-161) under autograd / in train(); BatchNorm on batch statistics in train(), on the
    frozen ones in eval()."""
    _count()
    a, b = m.conv1, m.conv2
    y = T.batchnorm_train(a.bn, _Deconv2dK4S2.apply(x, a.conv.weight, None), relu=True)
    z = _Conv2dK3Cat.apply(y, rem, b.conv.weight)
    return T.batchnorm_train(b.bn, z, relu=bool(b.relu))


def spx2_train_applies(m, x):
    return _enabled(x) and len(m) == 1 and _deconv_fits(m[0], x)


def spx2_train(m, x):
    """`spx2` (models/SemStereo.py:207) under autograd / in train()."""
    _count()
    return _Deconv2dK4S2.apply(x, m[0].weight, m[0].bias)
