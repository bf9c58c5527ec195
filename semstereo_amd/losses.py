"""The training objective of the reference (main_us3d.py:199-208; models/loss.py) under its own names and signatures.

  model_loss_train / model_loss_test   models/loss.py:19-31    weighted smooth-L1 / L1 over the masked pixels of up to four outputs
  model_label_loss                     models/loss.py:106-119  2.4 (1.6) x (cross-entropy ignoring class 5 + multi-class Dice loss)
  LRSC_loss                            models/loss.py:121-135  cross-entropy of the right view's logits against the warped left labels
  train_objective                      main_us3d.py:199-208    the three together; the masks are ranges on the ground truth, never tensors

CUDA fp32 inputs run csrc/loss.hip: one autograd Function per loss, a reduction launch and a one-workgroup finish forward, one launch
backward, the result and the record of sums staying on the device -- no `nonzero`, no host wait, nothing of full resolution saved
beyond the caller's own tensors.  Everything else (CPU tensors, float64, other class counts, SS_LOSS_HIP=0) takes the PyTorch
composition below, which is written without boolean indexing (masked sums through torch.where) and therefore does not wait on the host
either.  modules.PATH_COUNTS["loss_hip"] / ["loss_torch"] count the calls of each path.
"""
import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib
from . import engine as E
from ._host import LABEL_CODES, _c, count
from ._lib import call, ptr

NCLS = 6
TRAIN_WEIGHTS = (1.0, 0.6, 0.5, 0.3)      # models/loss.py:20
TEST_WEIGHTS = (1.0,)                     # :27
DICE_EPS = 1e-6                           # :33
NAMES = ("model_loss_train", "model_loss_test", "model_label_loss", "LRSC_loss")


def workspace_bytes(kind):
    """Scratch of the forward entry points: kind 0 = ss_disparity_loss_fwd, 1 = ss_label_loss_fwd / ss_lrsc_loss_fwd."""
    return _lib.query_bytes("ss_loss_workspace_bytes", kind)


def _workspace(kind, device):
    return torch.empty(workspace_bytes(kind) // 8, dtype=torch.float64, device=device)


# ------------------------------------------------------------------------------------------------ PyTorch composition (the fallback)
def _keep(gt, mask, rng):
    if mask is not None:
        if mask.shape != gt.shape:
            raise ValueError(f"mask {tuple(mask.shape)} and disparity {tuple(gt.shape)} differ in shape")
        return mask if mask.dtype == torch.bool else mask.bool()
    return (gt >= rng[0]) & (gt < rng[1])


def _disparity_loss_torch(ests, gts, masks, rng, weights, l1):
    total = 0
    for est, gt, w, mask in zip(ests, gts, weights, masks):
        keep = _keep(gt, mask, rng)
        d = est - gt
        ad = d.abs()
        v = ad if l1 else torch.where(ad < 1, 0.5 * d * d, ad - 0.5)
        total = total + w * (torch.where(keep, v, torch.zeros_like(v)).sum() / keep.sum())     # 0 / 0 = NaN: an empty selection's mean
    return total


def _label_loss_torch(logits, labels, ce_ignore, dice, drop_last, scale):
    C = logits.shape[1]
    y = labels.long()
    inside = (y >= 0) & (y < C)
    counted = inside if ce_ignore is None else inside & (y != ce_ignore)
    ys = torch.where(inside, y, torch.zeros_like(y)).unsqueeze(1)
    logp = F.log_softmax(logits, dim=1)
    zero = logp.new_zeros(())
    loss = torch.where(counted, -logp.gather(1, ys).squeeze(1), zero).sum() / counted.sum()
    if dice:
        p = logp.exp()
        fg = inside & (y < C - 1) if drop_last else inside
        inter = 2 * torch.where(fg, p.gather(1, ys).squeeze(1), zero).sum()
        sets = (p[:, :-1] if drop_last else p).sum() + fg.sum()
        empty = sets == 0                                                     # models/loss.py:42
        loss = loss + 1 - torch.where(empty, torch.ones_like(sets), (inter + DICE_EPS) / (sets + DICE_EPS))
    return loss * scale if scale != 1 else loss


def warp_labels(disp, y):
    """The left labels as the right view sees them (models/loss.py:123-133): y[b, h, (long) clamp(x - disp[b, h, x], 0, W - 1)], the
    difference evaluated in the disparity's dtype as the reference's int64 - float tensor expression is."""
    b, h, w = y.shape
    x = torch.arange(w, device=y.device).view(1, 1, w).expand(b, h, w)
    xs = torch.clamp(x - disp.detach(), min=0, max=w - 1).long()
    return torch.gather(y, 2, xs).to(torch.int64)


# ------------------------------------------------------------------------------------------------ what the kernels are built for
def _same_cuda_f32(ts):
    return all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.device == ts[0].device for t in ts)


def supported_disparity(ests, gts, masks):
    """CUDA fp32 estimates and ground truths of equal shape on one device, bool masks of that shape (or None: a range), at most four
    terms, fewer than 2^31 elements each, no gradient asked of the ground truth."""
    n = min(len(ests), len(gts), len(masks))
    if not 1 <= n <= 4 or not _same_cuda_f32(list(ests[:n]) + list(gts[:n])):
        return False
    for est, gt, mask in zip(ests[:n], gts[:n], masks[:n]):
        if est.shape != gt.shape or not 0 < est.numel() < 2 ** 31 or (gt.requires_grad and torch.is_grad_enabled()):
            return False
        if mask is not None and not (isinstance(mask, torch.Tensor) and mask.dtype == torch.bool and mask.shape == est.shape
                                     and mask.device == est.device):
            return False
    return True


def supported_labels(logits, labels, disp=None):
    """CUDA fp32 logits [B,6,H,W] with fewer than 2^31 elements, integer (or floating) labels [B,H,W] on the same device and, for the
    LRSC form, an fp32 disparity [B,H,W]."""
    if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 4):
        return False
    B, C, H, W = logits.shape
    if C != NCLS or not 0 < logits.numel() < 2 ** 31:
        return False
    if not (isinstance(labels, torch.Tensor) and labels.device == logits.device and tuple(labels.shape) == (B, H, W)
            and not labels.is_complex() and not labels.requires_grad):
        return False
    if disp is not None and not (isinstance(disp, torch.Tensor) and disp.device == logits.device and disp.dtype == torch.float32
                                 and tuple(disp.shape) == (B, H, W)):
        return False
    return True


# ------------------------------------------------------------------------------------------------ autograd Functions over csrc/loss.hip
class _DisparityLoss(torch.autograd.Function):
    """loss = sum_i w_i * mean_{kept}(smooth-L1 or L1 of est_i - gt_i).  tensors = n estimates, n ground truths, n masks (bool or None);
    `rng` = (lo, hi) keeps lo <= gt < hi where the mask is None.  Differentiable inputs: the estimates."""

    @staticmethod
    def forward(ctx, weights, l1, rng, n, *tensors):
        ests, gts = [_c(t) for t in tensors[:n]], [_c(t) for t in tensors[n:2 * n]]
        masks = [None if m is None else _c(m) for m in tensors[2 * n:3 * n]]
        dev = ests[0].device
        rec = torch.empty(8, dtype=torch.float64, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        ws = _workspace(0, dev)
        terms = []
        for i in range(4):
            terms += [ptr(ests[i]), ptr(gts[i]), ptr(masks[i]), ests[i].numel()] if i < n else [None, None, None, 0]
        w = [float(weights[i]) if i < n else 0.0 for i in range(4)]
        with torch.cuda.device(dev):
            call("ss_disparity_loss_fwd", *terms, *w, float(rng[0]), float(rng[1]), n, int(bool(l1)), ptr(rec), ptr(loss), ptr(ws),
                 ws.numel() * 8)
        ctx.save_for_backward(rec, *ests, *gts, *[m for m in masks if m is not None])
        ctx.cfg = (w, bool(l1), (float(rng[0]), float(rng[1])), n, [m is not None for m in masks])
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        w, l1, rng, n, has_mask = ctx.cfg
        rec, *rest = ctx.saved_tensors
        ests, gts, given = rest[:n], rest[n:2 * n], list(rest[2 * n:])
        masks = [given.pop(0) if h else None for h in has_mask]
        need = ctx.needs_input_grad[4:4 + n]
        grads = [torch.empty_like(e) if want else None for e, want in zip(ests, need)]
        if any(need):
            g = _c(g.to(torch.float32))
            terms = []
            for i in range(4):
                terms += [ptr(ests[i]), ptr(gts[i]), ptr(masks[i]), ptr(grads[i]), ests[i].numel()] if i < n else [None, None, None, None, 0]
            with torch.cuda.device(g.device):
                call("ss_disparity_loss_bwd", *terms, *w, rng[0], rng[1], n, int(l1), ptr(rec), ptr(g))
        return (None, None, None, None, *grads, *([None] * (2 * n)))


class _LabelLoss(torch.autograd.Function):
    """scale * (cross-entropy ignoring `ignore` + Dice loss) of logits [B,6,H,W] against labels [B,H,W]; with `disp` the LRSC form: a plain
    cross-entropy against the labels gathered along the row (`warped`, optional int64 [B,H,W], receives them).  Differentiable: logits."""

    @staticmethod
    def forward(ctx, logits, labels, disp, ignore, scale, warped):
        logits, labels = _c(logits), _c(labels)
        if labels.dtype not in LABEL_CODES:
            labels = labels.to(torch.int64)
        B, C, H, W = logits.shape
        dev = logits.device
        rec = torch.empty(8, dtype=torch.float64, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        ws = _workspace(1, dev)
        code = LABEL_CODES[labels.dtype]
        with torch.cuda.device(dev):
            if disp is None:
                call("ss_label_loss_fwd", ptr(logits), ptr(labels), code, B, C, H, W, int(ignore), float(scale), ptr(rec), ptr(loss), ptr(ws),
                     ws.numel() * 8)
                ctx.save_for_backward(rec, logits, labels)
            else:
                disp = _c(disp.detach())
                call("ss_lrsc_loss_fwd", ptr(logits), ptr(disp), ptr(labels), code, B, C, H, W, ptr(rec), ptr(loss), ptr(warped), ptr(ws),
                     ws.numel() * 8)
                ctx.save_for_backward(rec, logits, labels, disp)
        ctx.cfg = (code, int(ignore), float(scale))
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        code, ignore, scale = ctx.cfg
        rec, logits, labels, *disp = ctx.saved_tensors
        B, C, H, W = logits.shape
        g = _c(g.to(torch.float32))
        grad = torch.empty_like(logits)
        with torch.cuda.device(logits.device):
            if disp:
                call("ss_lrsc_loss_bwd", ptr(logits), ptr(disp[0]), ptr(labels), code, B, C, H, W, ptr(rec), ptr(g), ptr(grad))
            else:
                call("ss_label_loss_bwd", ptr(logits), ptr(labels), code, B, C, H, W, ignore, scale, ptr(rec), ptr(g), ptr(grad))
        return (grad, None, None, None, None, None)


# ------------------------------------------------------------------------------------------------ the reference's four names
def _disparity_loss(disp_ests, disp_gts, img_masks, rng, weights, l1):
    n = min(len(disp_ests), len(disp_gts), len(img_masks), len(weights))
    ests, gts, masks = list(disp_ests[:n]), list(disp_gts[:n]), list(img_masks[:n])
    if E.LOSS_HIP and supported_disparity(ests, gts, masks):
        count("loss_hip")
        return _DisparityLoss.apply(weights, l1, rng, n, *ests, *gts, *masks)
    count("loss_torch")
    return _disparity_loss_torch(ests, gts, masks, rng, weights, l1)


def model_loss_train(disp_ests, disp_gts, img_masks):
    """models/loss.py:19-24: sum of 1.0 / 0.6 / 0.5 / 0.3 x smooth-L1 over disp_est[mask] (the lists are zipped: shorter ones cut it)."""
    return _disparity_loss(disp_ests, disp_gts, img_masks, (0.0, 0.0), TRAIN_WEIGHTS, False)


def model_loss_test(disp_ests, disp_gts, img_masks):
    """models/loss.py:26-31: the L1 of the first output over its mask."""
    return _disparity_loss(disp_ests, disp_gts, img_masks, (0.0, 0.0), TEST_WEIGHTS, True)


def model_label_loss(masks_preds, true_masks, num_classes, attention_weights_only, ignore=5):
    """models/loss.py:106-119.  As there, a false `ignore` (None, 0) means no ignored class and a Dice term over all classes."""
    if masks_preds.dim() != 4 or masks_preds.shape[1] != num_classes:
        raise ValueError(f"logits {tuple(masks_preds.shape)} do not carry num_classes = {num_classes} channels")
    scale = 1.6 if attention_weights_only else 2.4
    if E.LOSS_HIP and ignore and supported_labels(masks_preds, true_masks):
        count("loss_hip")
        return _LabelLoss.apply(masks_preds, true_masks, None, int(ignore), scale, None)
    count("loss_torch")
    return _label_loss_torch(masks_preds, true_masks, int(ignore) if ignore else None, True, bool(ignore), scale)


def LRSC_loss(label_est_r, disp_ests, y, warped=None):
    """models/loss.py:121-135: the right view's logits against the left labels y [B,H,W] warped by disp_ests[0] [B,H,W]; the disparity
    gets no gradient.  `warped` (not in the reference): an int64 [B,H,W] tensor that receives the warped label map."""
    disp = disp_ests[0]
    if E.LOSS_HIP and supported_labels(label_est_r, y, disp) and (warped is None or (
            warped.dtype == torch.int64 and warped.shape == y.shape and warped.device == y.device and warped.is_contiguous())):
        count("loss_hip")
        return _LabelLoss.apply(label_est_r, y, disp, -1, 1.0, warped)
    count("loss_torch")
    yw = warp_labels(disp, y)
    if warped is not None:
        warped.copy_(yw)
    return _label_loss_torch(label_est_r, yw, -1, False, False, 1)


def train_objective(disp_ests, label_est, label_est_r, disp_gt, disp_gt_4, label_true, maxdisp, attention_weights_only, num_classes=6):
    """main_us3d.py:199-208: (loss, disp_loss, label_loss, lrsc_loss) with loss their sum.  The masks `-maxdisp <= gt < maxdisp` of
    :199-200 are evaluated inside the disparity kernel: no mask tensor is built."""
    gts = [disp_gt, disp_gt_4, disp_gt, disp_gt_4]                 # :202
    lrsc_loss = LRSC_loss(label_est_r, disp_ests, label_true)      # :204
    disp_loss = _disparity_loss(disp_ests, gts, [None] * 4, (-float(maxdisp), float(maxdisp)), TRAIN_WEIGHTS, False)
    label_loss = model_label_loss(label_est, label_true, num_classes, attention_weights_only)
    return disp_loss + label_loss + lrsc_loss, disp_loss, label_loss, lrsc_loss
