"""Host-side helpers every module around the binding shares (nothing here touches the library)."""
import torch
import torch.nn as nn

#: calls per path ("hip", "torch", "hip_train", "loss_hip", ...): what ran the kernels and what ran the PyTorch composition
PATH_COUNTS = {"hip": 0, "torch": 0}
#: include/semstereo_hip.h: label_dtype / src_dtype
LABEL_CODES = {torch.int64: 0, torch.uint8: 1, torch.float32: 2}
_CONST = {}


def count(key, n=1):
    PATH_COUNTS[key] = PATH_COUNTS.get(key, 0) + n


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _nograd(fn):
    def wrapper(*args, **kwargs):
        with torch.no_grad():
            return fn(*args, **kwargs)
    wrapper.__name__, wrapper.__doc__ = fn.__name__, fn.__doc__
    return wrapper


def _const(key, device, make):
    """A small constant tensor on `device`, uploaded once (without waiting)."""
    k = (key, str(device))
    if k not in _CONST:
        _CONST[k] = make().to(device, non_blocking=True)
    return _CONST[k]


def _label_classes(y, C):
    """int64 of y's shape: the class of a label in [0, C), or C for "outside" -- csrc/metrics_decode.h's label_class.  Float labels
    truncate toward zero, NaN is outside."""
    if y.is_floating_point():
        inside = (y > -1) & (y < C)
        y = torch.where(inside, y, torch.zeros_like(y)).long()
    else:
        y = y.long()
        inside = (y >= 0) & (y < C)
    return torch.where(inside, y, torch.full_like(y, C))


def argmax_first(logits):
    """np.argmax over the channel axis as elementwise selects: the lowest index among equal maxima, a NaN counts as the maximum
    (csrc/metrics_decode.h's argmax_take)."""
    best = logits[:, 0]
    idx = torch.zeros(best.shape, dtype=torch.int64, device=logits.device)
    for k in range(1, logits.shape[1]):
        z = logits[:, k]
        take = ~torch.isnan(best) & ((z > best) | torch.isnan(z))
        best = torch.where(take, z, best)
        idx = torch.where(take, torch.full_like(idx, k), idx)
    return idx


def bn_ok(bn):
    return isinstance(bn, nn.BatchNorm2d) and (bn.training or bn.running_mean is not None)
