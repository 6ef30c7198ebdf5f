"""unet_hip - MI355X-native (gfx950) UNet training / inference path for the DDTI
thyroid-nodule workload (drop-in for models/model.py:UNet of
WuJiaqiii/Thyroid-nodule-image-segmentation-UNet-DDTI).

    from unet_hip import UNet, seg_losses, HipAdamW

Everything on the hot path runs in libunet_hip.so (hand-written HIP kernels, C ABI in
include/unet_hip.h); this package is the PyTorch-facing host side.  There is no CPU
fallback: without the built library every entry point raises ``HipUnavailable``.
"""
from ._lib import HipError, HipUnavailable, LIB_PATH, load  # noqa: F401
from .data import GpuResizeToTensor  # noqa: F401
from .functional import (LovaszHingeFunction, boundary_loss, connected_components, connected_components_host,  # noqa: F401
                         curve_edges, curve_hist, curve_hist_host, curve_stats, curve_stats_host,
                         curve_summary, distance_maps, echo_descriptors, echo_table, echo_table_host,
                         lesion_echo, lesion_echo_host, lesion_metrics, lesion_metrics_host,
                         lesion_morphometry, lesion_morphometry_host, lovasz_hinge,
                         lovasz_hinge_host, lovasz_hinge_parts, overlay,
                         morphometry_table, morphometry_table_host, overlay_host, postprocess_mask, postprocess_mask_host, resize_back, resize_back_host,
                         seg_losses, shape_descriptors, surface_metrics, surface_metrics_host,
                         tta_merge, tta_merge_host, tta_predict, tta_views, tta_views_host)
from .module import ModUNet, ResUNet, UNet  # noqa: F401
from .optim import HipAdamW  # noqa: F401
from .predict import Predictor  # noqa: F401
from .runtime import UNetRuntime  # noqa: F401
