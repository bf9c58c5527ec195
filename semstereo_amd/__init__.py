"""semstereo_amd -- MI355X-native (gfx950) cost-volume + 3-D aggregation hot path of SemStereo.

  ops       drop-in callables with the reference's names (models/submodule.py)
  modules   nn.Module twins of the 3-D stack with the reference's state_dict keys
  segment   HotSegment: features -> disparities (models/SemStereo.py:273-323)
  install   install(model_module) / accelerate(model): drop-in into the reference's own model
  losses    the training objective under the reference's names (models/loss.py), install_losses(script_module)
  metrics   the evaluation step's metrics under the reference's names (utils/metrics.py), install_metrics(script_module)
  joint_metrics  disparity error per semantic class and mIoU-3 from one pass: joint_metrics, JointMetric, eval_metrics_joint
  visualization  the evaluation step's image outputs under the reference's names (utils/visualization.py, utils/mask_vis.py),
            install_visualization(script_module)
  data      the datasets' sample preparation on the device (datasets/us3d_.py, datasets/whu_dataset.py): normalised views, ground-truth
            pyramids, gx / gy; right_view (right-view ground truth, the left view's visibility) and lr_consistency;
            RawStereoDataset and DeviceLoader
  augment   training augmentation on the device: Augmentation (the reference's KITTI recipe, plus a vertical flip and a horizontal flip
            with the views swapped), AugmentParams, augment_sample; DeviceLoader(..., augment=...)
  refine    what follows the model call: fill_disparity (holes filled from the nearest kept pixel of the same predicted class in the row,
            then of any class; axes="both": in the row and the column), refine_disparity (the left-right check and that fill), median_disparity (a 2-D
            median in which a pixel is smoothed only with pixels of its own class) and filter_speckles (small connected blobs
            of one class removed before the fill)
  scene     inference on whole scenes of any size: TilePlan (windows, feather weights, bands), tile_views and blend_tiles (the two
            kernels around the model call), SceneStereo (tiles on a PairPipeline's lanes, a feathered mosaic with a seam diagnostic)
  dist      one-process-per-GPU batch sharding (RCCL / gloo)

The compute lives in csrc/libsemstereo_hip.so behind the C ABI of include/semstereo_hip.h.
Nothing here falls back to the CPU or to the test oracle.
"""
from . import _lib, augment, data, dist, engine, joint_metrics, losses, metrics, modules, ops, ops_unsigned, refine, scene, segment, train_layers, visualization  # noqa: F401
from .install import accelerate, install, install_losses, install_metrics, install_visualization, restore_forward, uninstall  # noqa: F401
from .losses import LRSC_loss, model_label_loss, model_loss_test, model_loss_train, train_objective  # noqa: F401
from .metrics import EvalAverager, SegmentationMetric, disparity_metrics, eval_metrics  # noqa: F401
from .joint_metrics import JointMetric, eval_metrics_joint  # noqa: F401  (the record itself: joint_metrics.joint_metrics)
from .visualization import disp_error_image_func, eval_images, feature_vis, label_vis, normalize_image  # noqa: F401
from .data import DeviceLoader, RawStereoDataset, image_gradients, nearest_pyramid, normalize_views, prepare_sample  # noqa: F401
from .data import RIGHT_VIEW_KEYS, lr_consistency, right_view  # noqa: F401
from .augment import AugmentParams, Augmentation, augment_sample  # noqa: F401
from .refine import MEDIAN_KEYS, REFINE_KEYS, REFINE_KEYS_2D, SPECKLE_KEYS, fill_disparity, filter_speckles, median_disparity, refine_disparity  # noqa: F401
from .scene import SceneStereo, TilePlan, blend_tiles, tile_views  # noqa: F401
from .segment import GraphedSegment, HotSegment, PairPipeline  # noqa: F401

__version__ = "0.1.0"
