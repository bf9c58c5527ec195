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


def bn_ok(bn):
    return isinstance(bn, nn.BatchNorm2d) and (bn.training or bn.running_mean is not None)
