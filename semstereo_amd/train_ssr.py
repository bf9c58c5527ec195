"""Training side of the semantic-guided refinement head SSR_upsample (models/submodule.py:412-431, called twice per training forward at
models/SemStereo.py:311 and :324): one autograd Function whose forward and backward are csrc/ssr_upsample_train.hip.

BatchNorm runs on batch statistics in train() (the running statistics and num_batches_tracked move inside the kernels, as F.batch_norm
moves them) and on the running statistics in eval() under autograd.  Nothing of full resolution is saved for the backward: the inputs,
the packed parameters and 256 floats of statistics.  Each call computes its own gate statistics, so the reference's two calls move the
gate's running statistics twice, as the reference does.
"""
import torch
import torch.nn as nn

from . import _lib
from ._host import _c
from ._lib import call, ptr

NCLS = 6
SAVED_FLOATS = 256        # csrc/ssr_upsample_train.hip: SAVED_FLOATS
_KS, _GMAX = 128, 1024    # ... KS (slab row, doubles) and GMAX (workgroups of a reduction pass)


def _bns(m):
    return (m.conv[0], m.conv[2], m.conv1[1], m.conv2[1])


def workspace_bytes(B, h, w, backward=False, grad_low=False):
    """The scratch ss_ssr_upsample_train_fwd / _bwd ask for (include/semstereo_hip.h)."""
    n = B * 16 * h * w
    g = min(-(-n // 256), _GMAX)
    return 8 * _KS * g + ((256 + (28 * n if grad_low else 0)) if backward else 0)


def _workspace(nbytes, device):
    return torch.empty(-(-nbytes // 8), dtype=torch.float64, device=device)


def supported(m, depth_low, weights, pred_label):
    """The shapes, dtypes and module settings the kernels are built for (anything else keeps the PyTorch composition)."""
    ts = (depth_low, weights, pred_label)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 for t in ts):
        return False
    dev = depth_low.device
    if weights.device != dev or pred_label.device != dev or m.num_classes != NCLS or depth_low.dim() != 4:
        return False
    b, c, h, w = depth_low.shape
    if c != 1 or tuple(weights.shape) != (b, NCLS, 4 * h, 4 * w) or tuple(pred_label.shape) != tuple(weights.shape):
        return False
    if b * 16 * h * w * NCLS >= 2 ** 31 - _GMAX * 256 or b * h * w == 0:
        return False
    bns = _bns(m)
    for bn in bns:
        if not (isinstance(bn, nn.BatchNorm2d) and bn.affine and bn.track_running_stats and isinstance(bn.momentum, float)
                and bn.training == bns[0].training and bn.running_mean is not None and bn.running_var is not None):
            return False
        for t in (bn.running_mean, bn.running_var):
            if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
                return False
        nbt = bn.num_batches_tracked
        if nbt is not None and (nbt.dtype != torch.int64 or nbt.device != dev):
            return False
    convs = (m.conv[1], m.conv1[0], m.conv2[0], m.conv3)
    if not all(isinstance(cv, nn.Conv2d) and cv.bias is not None for cv in convs):
        return False
    if (m.conv[1].kernel_size, m.conv[1].padding, m.conv[1].stride) != ((3, 3), (1, 1), (1, 1)) or m.conv[1].in_channels != 1:
        return False
    if any(cv.kernel_size != (1, 1) or cv.padding != (0, 0) or cv.stride != (1, 1) for cv in convs[1:]):
        return False
    if any(cv.groups != 1 or cv.dilation != (1, 1) for cv in convs):
        return False
    params = list(m.parameters())
    return len(params) == 16 and all(p.dtype == torch.float32 and p.device == dev for p in params)


class _SSRUpsampleTrain(torch.autograd.Function):
    """out = SSR_upsample(depth_low, weights, pred_label) [B,4h,4w].  Differentiable inputs: depth_low, weights, pred_label and the
    head's 16 parameters (nn.Module.parameters() order); `running` = ((running_mean, running_var, num_batches_tracked, eps, momentum)
    for conv.0, conv.2, conv1.1, conv2.1) -- a tuple, so that autograd does not see the buffers; `batch` = batch statistics."""

    @staticmethod
    def forward(ctx, depth_low, weights, pred_label, running, batch, *params):
        depth_low, weights, pred_label = _c(depth_low), _c(weights), _c(pred_label)
        B, _, h, w = depth_low.shape
        dev = depth_low.device
        prm = torch.cat([p.detach().reshape(-1) for p in params])
        saved = torch.empty(SAVED_FLOATS, dtype=torch.float32, device=dev)
        out = torch.empty((B, 4 * h, 4 * w), dtype=torch.float32, device=dev)
        nbytes = workspace_bytes(B, h, w)
        ws = _workspace(nbytes, dev)
        run_args = []
        for rm, rv, nbt, _eps, _mom in running:
            run_args += [ptr(rm), ptr(rv), ptr(nbt)]
        with torch.cuda.device(dev):
            call("ss_ssr_upsample_train_fwd", ptr(depth_low), ptr(weights), ptr(pred_label), ptr(prm), ptr(out), ptr(saved), *run_args,
                 *[float(r[3]) for r in running], *[float(r[4]) for r in running], int(bool(batch)), B, h, w, NCLS, ptr(ws), nbytes)
        if batch:
            for rm, rv, nbt, _eps, _mom in running:       # (written through raw pointers: the eval path's _params() cache keys on versions)
                for t in (rm, rv, nbt):
                    if t is not None:
                        torch.autograd.graph.increment_version(t)
        ctx.save_for_backward(depth_low, weights, pred_label, prm, saved)
        ctx.batch = bool(batch)
        ctx.shapes = [p.shape for p in params]
        return out

    @staticmethod
    def backward(ctx, g):
        depth_low, weights, pred_label, prm, saved = ctx.saved_tensors
        B, _, h, w = depth_low.shape
        dev = depth_low.device
        g = _c(g)
        need = ctx.needs_input_grad
        glow = torch.empty_like(depth_low) if need[0] else None
        gwt = torch.empty_like(weights) if need[1] else None
        glg = torch.empty_like(pred_label) if need[2] else None
        gprm = torch.empty_like(prm)
        nbytes = workspace_bytes(B, h, w, backward=True, grad_low=glow is not None)
        ws = _workspace(nbytes, dev)
        with torch.cuda.device(dev):
            call("ss_ssr_upsample_train_bwd", ptr(depth_low), ptr(weights), ptr(pred_label), ptr(prm), ptr(saved), ptr(g), ptr(glow),
                 ptr(gwt), ptr(glg), ptr(gprm), int(ctx.batch), B, h, w, NCLS, ptr(ws), nbytes)
        grads, o = [], 0
        for shape, want in zip(ctx.shapes, need[5:]):
            n = 1
            for s in shape:
                n *= s
            grads.append(gprm[o:o + n].view(shape) if want else None)
            o += n
        return (glow, gwt, glg, None, None, *grads)


def ssr_train(m, depth_low, weights, pred_label):
    """The head `m` (modules.SSR_upsample) on the HIP training kernels; `supported(m, ...)` must hold."""
    _lib.require_device(depth_low, weights, pred_label)
    bns = _bns(m)
    batch = bns[0].training
    running = tuple((bn.running_mean, bn.running_var, bn.num_batches_tracked, float(bn.eps), float(bn.momentum)) for bn in bns)
    return _SSRUpsampleTrain.apply(depth_low, weights, pred_label, running, batch, *m.parameters())
