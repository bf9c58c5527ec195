"""Drop-in installation into the reference's own model code.

The reference has no plugin registry: `models/SemStereo.py` star-imports the op library and looks
the functions up BY BARE NAME in its module globals at call time (models/SemStereo.py:7-8, 273,
283, 285, 291, 316, 323), and holds the 3-D stack as nn.Module attributes created in __init__
(:219-236).  So a drop-in is two steps, both leaving `forward()` untouched:

    import models.SemStereo as ms                  # the reference's module
    import semstereo_amd
    semstereo_amd.install(ms)                      # rebind the op-library names in ITS globals
    net = ms.SemStereo(...); net.load_state_dict(ckpt); net.cuda().eval()
    semstereo_amd.accelerate(net)                  # swap hourglass/classifier/... for HIP-backed twins

That alone runs every hot op and module of the reference's forward() on the HIP kernels (measured on the
bench shape: 190 pairs/s for the hot segment).  The fusions that cross the lines of forward() -- patch+gate,
softmax+regression+variance, the two attention-tail kernels, warp+concat+gate, stem+gate, the two-stream
overlap (260 pairs/s) -- need the inference call path itself:

    semstereo_amd.accelerate(net, fuse_forward=True)   # eval()/no_grad calls take the fused path; training,
                                                       # autograd and seg-only calls still run the reference forward()

A training script adds `fuse_training=True`: train() / autograd calls then run `fused_training_forward` -- the reference's sub-module
calls around the segment's training kernels (train.attention_tail, train.concat_volume_sampled) -- instead of its forward():

    semstereo_amd.accelerate(net, fuse_forward=True, fuse_training=True)
"""
import torch
import torch.nn as nn

from . import modules as M
from . import ops
from . import segment


def _rebind(module, names, source):
    previous = {}
    for name in names:
        previous[name] = getattr(module, name, None)
        setattr(module, name, getattr(source, name))
    return previous


def install(model_module, names=ops.REFERENCE_NAMES, unsigned=False):
    """setattr(model_module, name, hip_op) for every hot-path callable.  Rebinding
    `models.submodule.X` alone would not be enough: the star-import copied the binding.
    `unsigned`: the unsigned-range op set (`ops_unsigned`, models/submodule_.py's definitions) -- what
    models/SemStereo_WHU.py needs in its globals to run at all (see ops_unsigned's docstring).
    Returns {name: previous object} so `uninstall` can restore it."""
    from . import ops_unsigned
    return _rebind(model_module, names, ops_unsigned if unsigned else ops)


def install_losses(script_module):
    """The objective's counterpart of `install`: the reference's training script imports model_loss_train, model_loss_test,
    model_label_loss and LRSC_loss into its own globals (main_us3d.py:18) and calls them by bare name (:204-206), so the drop-in is the
    same rebinding, in the SCRIPT's module.  Returns {name: previous object} for `uninstall`."""
    from . import losses
    return _rebind(script_module, losses.NAMES, losses)


def install_metrics(script_module):
    """The evaluation step's counterpart of `install_losses`: the scripts get EPE_metric, D1_metric, Thres_metric, their *_mask variants
    and SegmentationMetric by `from utils import *` (main_us3d.py:16) and call them by bare name in test_sample (:228, :254-257), so
    the drop-in is the same rebinding in the SCRIPT's module.  Returns {name: previous object} for `uninstall`."""
    from . import metrics
    return _rebind(script_module, metrics.NAMES, metrics)


def install_visualization(script_module):
    """The image outputs' counterpart of `install_metrics`: the scripts get disp_error_image_func and feature_vis by
    `from utils import *` (main_us3d.py:16; utils/__init__.py:2, :6) and call them by bare name in test_sample (main_us3d.py:266-268),
    so the drop-in is the same rebinding in the SCRIPT's module.  Returns {name: previous object} for `uninstall`."""
    from . import visualization
    return _rebind(script_module, visualization.NAMES, visualization)


def uninstall(model_module, previous):
    for name, obj in previous.items():
        if obj is None:
            if hasattr(model_module, name):
                delattr(model_module, name)
        else:
            setattr(model_module, name, obj)


# attribute of the reference SemStereo instance -> adopting class
_SWAPS = {
    "hourglass_att": M.hourglass,
    "hourglass": M.hourglass2,
    "classif_att_": M.Classifier,
    "classif": M.Classifier,
    "concat_stem": M.BasicConv,
    "concat_feature": M.ConcatFeature,
    "patch": M.DepthwisePatch,
    "corr_feature_att_8": M.channelAtt,
    "concat_feature_att_4": M.channelAtt,
    "ssr_upsample": M.SSR_upsample,
    "propagation": M.Propagation,              # parameter-free: one-hot convolutions -> shifted views
    "propagation_prob": M.Propagation_prob,
}


# ... and of the 2-D decoder (FeatUp, the spx chain, spx2: models/SemStereo.py:194, 207-211), swapped by accelerate(decoder=True)
_DECODER_SWAPS = {
    "feature_up": M.FeatUp,
    "spx32_16": M.Conv2x,
    "spx16_8": M.Conv2x,
    "spx8_4": M.Conv2x,
    "spx4_2": M.Conv2x,
    "spx2": M.Spx2,
}


# ... and of the segmentation heads and the chal_* projections (models/SemStereo.py:200-201, 213-217), swapped by accelerate(heads=True)
_HEAD_SWAPS = {
    "head_l": M.segmenthead,
    "head_r": M.segmenthead,
    "chal_0": M.ChalProjection,
    "chal_1": M.ChalProjection,
    "chal_2": M.ChalProjection,
    "chal_3": M.ChalProjection,
    "chal_4": M.ChalProjection,
}


def accelerate(model, fuse_forward=False, decoder=False, heads=False, fuse_training=False):
    """Replace the hot-path sub-modules of a reference `SemStereo` instance (or of the .module of
    its nn.DataParallel wrapper) by HIP-backed twins that SHARE its parameters; state_dict keys and
    values are unchanged.  With `fuse_forward` the instance's forward is additionally routed through
    `fused_inference_forward` for inference calls.  With `fuse_training` (which includes `fuse_forward`) train() and autograd calls
    are routed through `fused_training_forward` instead of being handed back to the model's own forward(); SS_FUSE_TRAINING=0 in the
    environment turns that off again.  With `decoder` the 2-D decoder (`feature_up`, `spx32_16` .. `spx4_2`, `spx2`)
    is swapped too: its 4x4 stride-2 transposed convs and concat + 3x3 convs then run on HIP kernels in inference (SS_DECODER_HIP).
    With `heads` the segmentation heads (`head_l`, `head_r`) and the projections `chal_0` .. `chal_4` are swapped as well (SS_HEADS_HIP); a
    module without the expected layout -- the WHU variant's pre-activation head -- stays in place.
    Returns the list of swapped attribute names."""
    target = model.module if isinstance(model, nn.DataParallel) else model
    done = []
    swaps = list(_SWAPS.items()) + (list(_DECODER_SWAPS.items()) if decoder else []) + (list(_HEAD_SWAPS.items()) if heads else [])
    for name, cls in swaps:
        sub = getattr(target, name, None)
        if sub is None or isinstance(sub, cls):
            continue
        before = list(sub.state_dict().keys())
        new = cls.adopt(sub)
        if new is None:                      # (the twin declines this layout: the module stays)
            continue
        assert list(new.state_dict().keys()) == before, f"state_dict keys of {name} changed"
        setattr(target, name, new)
        done.append(name)
    if fuse_training and not getattr(type(target), "_ss_fused_training", False):
        target.__class__ = _fused_class(getattr(type(target), "_ss_reference_class", type(target)), training=True)
    elif fuse_forward and not getattr(type(target), "_ss_fused_forward", False):
        target.__class__ = _fused_class(type(target))
    if not target.__dict__.get("_ss_output_hook"):
        # deferred handles (deferred.py) never leave the model: whatever forward() returns is realised on the way out -- since r05
        # also the SSR head's result (`pred_up * 4`, models/SemStereo.py:346); a handle that is NOT part of the output, like the
        # `pred_att_up` of an eval forward (:311), is simply never computed
        target.register_forward_hook(_realise_outputs)
        target.__dict__["_ss_output_hook"] = True
    return done


def _realise_outputs(module, inputs, output):
    from . import deferred as dfr
    M.drop_parked_gates(module)       #  a class gate parked by an odd number of SSR_upsample calls does not outlive the forward
    return dfr.real(output)


_FUSED_CLASSES = {}


def _fused_class(base, training=False):
    """A subclass of the model's own class whose forward() is `fused_inference_forward`; the reference's forward()
    stays reachable as the base class's.  The routing lives on the CLASS, not in the instance __dict__:
    nn.DataParallel builds its per-GPU replicas with `replica = cls.__new__(cls); replica.__dict__ =
    module.__dict__.copy()` (torch/nn/modules/module.py: _replicate_for_data_parallel), so a bound method stored in
    the instance would keep pointing every replica at the cuda:0 original (main_us3d.py:100, test_us3d.py:58).
    `training`: the class of `accelerate(..., fuse_training=True)`, whose forward() is `fused_training_forward` -- that one passes
    eval() / no-autograd calls on to `fused_inference_forward`."""
    key = (base, True) if training else base
    cls = _FUSED_CLASSES.get(key)
    if cls is None:
        route = fused_training_forward if training else fused_inference_forward
        def forward(self, left, right):
            return route(self, left, right, reference_forward=super(cls, self).forward)
        def reduce_ex(self, protocol):
            # whole-model pickling (torch.save(model), multiprocessing spawn): as an instance of the reference's own class --
            # this subclass exists only in the running process (accelerate(..., fuse_forward=True) again after loading)
            return (_rebuild_as, (base, self.__dict__.copy()))
        cls = type(base.__name__, (base,), {"forward": forward, "_ss_fused_forward": True, "_ss_reference_class": base,
                                            "_ss_fused_training": bool(training), "__reduce_ex__": reduce_ex,
                                            "__module__": base.__module__, "__qualname__": base.__qualname__})
        _FUSED_CLASSES[key] = cls
    return cls


def _rebuild_as(base, state):
    obj = base.__new__(base)
    obj.__dict__.update(state)
    return obj


def restore_forward(model):
    """Undo `accelerate(..., fuse_forward=True)`'s forward routing (the swapped sub-modules stay)."""
    target = model.module if isinstance(model, nn.DataParallel) else model
    if getattr(type(target), "_ss_fused_forward", False):
        target.__class__ = type(target)._ss_reference_class


def _reference_forward(self):
    ref_cls = getattr(type(self), "_ss_reference_class", None)
    assert ref_cls is not None or type(self).forward not in (fused_inference_forward, fused_training_forward), \
        "no reference forward() to hand the call to"
    return (ref_cls or type(self)).forward.__get__(self)


def fused_training_forward(self, left, right, reference_forward=None):
    """The training counterpart of `fused_inference_forward`: models/SemStereo.py:246-346 for train() calls and for eval() calls
    under autograd (frozen statistics) -- the same sub-module calls in the same order as the reference's forward() around
    `segment.run_segment`, which under autograd runs :279-310 as `train.attention_tail` and :316-318 as `train.concat_volume_sampled`
    (where either declines the statements run, counted in PATH_COUNTS["train_tail_statements"] / ["train_concat_statements"]: by
    default the concat volume declines a quarter-resolution width that is no multiple of 64; with SS_TRAIN_CONCAT_ANY_WIDTH=1,
    `train.CONCAT_VOLUME_ANY_WIDTH`, it takes every width).  Every sub-module is called once per view as the reference
    calls it -- no pair launch merges the two views' batch statistics, and `ssr_upsample` runs on `pred_att` (:311) and then on `pred`
    (:324) -- so every BatchNorm sees the reference's calls in the reference's order.  Returns what the reference returns:
    `[pred_up*4, pred.squeeze(1)*4, pred_att_up*4, pred_att*4], pred_label, pred_label_r` in train() (`[pred_att_up*4, pred_att*4], ...`
    with att_weights_only), the eval structure in eval().  Without `seg_if` the lists alone; the label logits that `ssr_upsample`
    needs are then computed from `head_l` all the same, as the inference route does (the reference itself fails there, :311), and
    `head_r` is not called.  `SemStereo_WHU` takes the same route, told apart as in inference: by `self.unsigned` (segment.run_segment).
    eval() calls without autograd go to `fused_inference_forward`; CPU, non-fp32 and segmentation-only calls, and every call while
    SS_FUSE_TRAINING=0, to the reference's own forward()."""
    if reference_forward is None:
        reference_forward = _reference_forward(self)
    if not (self.stereo_if and left.is_cuda and right.is_cuda and left.dtype == right.dtype == torch.float32):
        return reference_forward(left, right)
    if M._inference(self, left, right):
        return fused_inference_forward(self, left, right, reference_forward=reference_forward)
    if not M.E._fuse_training_on():
        return reference_forward(left, right)
    M.PATH_COUNTS["train_route"] = M.PATH_COUNTS.get("train_route", 0) + 1
    fl, fr = self.feature(left), self.feature(right)                                         # :248-249
    fl, fr = self.feature_up(fl, fr)                                                         # :251
    fl, fr = list(fl), list(fr)
    pred_label = self.head_l(fl[0])                                                          # :254
    pred_label_r = self.head_r(fr[0]) if self.seg_if else None                               # :255
    for i, name in enumerate(("chal_0", "chal_1", "chal_2", "chal_3", "chal_4")):            # :258-262
        fl[i] = getattr(self, name)(fl[i])
    fr[1] = self.chal_1(fr[1])                                                               # :264-265
    fr[2] = self.chal_2(fr[2])
    xspx = self.spx32_16(fl[4], fl[3])                                                       # :267-271
    xspx = self.spx16_8(xspx, fl[2])
    xspx = self.spx8_4(xspx, fl[1])
    xspx = self.spx4_2(xspx, fl[0])
    spx_pred = self.spx2(xspx)
    try:
        r = segment.run_segment(self, fl[1], fr[1], fl[2], fr[2], matching=not self.att_weights_only)   # :273-310, :314-323
        pred_att = r["pred_att"]
        pred_att_up = self.ssr_upsample(pred_att.unsqueeze(1), spx_pred, pred_label)         # :311
        if not self.att_weights_only:
            pred = r["pred"]
            pred_up = self.ssr_upsample(pred, spx_pred, pred_label)                          # :324
    finally:
        M.drop_parked_gates(self)       # (a class gate parked by an odd number of ssr_upsample calls does not outlive the call)
    from . import deferred as dfr
    if self.training:                                                                        # :329-337
        outs = [pred_att_up * 4, pred_att * 4] if self.att_weights_only else [pred_up * 4, pred.squeeze(1) * 4, pred_att_up * 4, pred_att * 4]
        return dfr.real((outs, pred_label, pred_label_r) if self.seg_if else outs)
    outs = [pred_att_up * 4] if self.att_weights_only else [pred_up * 4]                     # :338-346
    return dfr.real((outs, pred_label) if self.seg_if else outs)


def fused_inference_forward(self, left, right, reference_forward=None):
    """The caller side of the hot path, models/SemStereo.py:246-346, for eval-mode / no-autograd calls: the
    same sub-module calls in the same order as the reference's forward() around `segment.run_segment`
    (:273-323 fused).  Returns exactly what the reference returns in eval mode: `[disp_full_res]` or
    `([disp_full_res], label_logits)`, disp = 4 * SSR_upsample(pred).  Everything else (training, autograd,
    segmentation-only models) is handed to the reference's own forward()."""
    if reference_forward is None:
        reference_forward = _reference_forward(self)
    if (self.training or not self.stereo_if or not left.is_cuda
            or (torch.is_grad_enabled() and (left.requires_grad or right.requires_grad
                                             or any(p.requires_grad for p in self.parameters())))):
        return reference_forward(left, right)
    fl, fr = self.feature(left), self.feature(right)                                         # :248-249
    fl, fr = self.feature_up(fl, fr)                                                         # :251
    fl, fr = list(fl), list(fr)
    # :253-255; without seg_if the reference itself fails at ssr_upsample (pred_label undefined), so the
    # label logits are computed whenever the stereo branch runs
    pred_label = self.head_l(fl[0])
    for i, name in enumerate(("chal_0", "chal_1", "chal_2", "chal_3", "chal_4")):            # :258-262
        chal = getattr(self, name)
        if i in (1, 2) and hasattr(chal, "forward_pair"):                                    # (the twin: both views in one launch)
            fl[i], fr[i] = chal.forward_pair(fl[i], fr[i])
        else:
            fl[i] = chal(fl[i])
    for i, name in ((1, "chal_1"), (2, "chal_2")):                                           # :264-265
        if not hasattr(getattr(self, name), "forward_pair"):
            fr[i] = getattr(self, name)(fr[i])
    xspx = self.spx32_16(fl[4], fl[3])                                                       # :267-271
    xspx = self.spx16_8(xspx, fl[2])
    xspx = self.spx8_4(xspx, fl[1])
    xspx = self.spx4_2(xspx, fl[0])
    spx_pred = self.spx2(xspx)
    r = segment.run_segment(self, fl[1], fr[1], fl[2], fr[2], matching=not self.att_weights_only)   # :273-323
    if self.att_weights_only:
        disp = self.ssr_upsample(r["pred_att"].unsqueeze(1), spx_pred, pred_label)           # :311
    else:
        disp = self.ssr_upsample(r["pred"], spx_pred, pred_label)                            # :324
    from . import deferred as dfr
    return dfr.real(([disp * 4], pred_label) if self.seg_if else [disp * 4])                 # :340-346
