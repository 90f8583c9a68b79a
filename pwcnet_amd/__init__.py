"""pwcnet_amd -- MI355X-native (gfx950) PWC-Net inference path.

Drop-in for the forward pass of daigo0927/pwcnet (model.py / modules.py op-level API):
Python host classes over hand-written HIP kernels in csrc/ (C ABI: include/pwc_hip.h).
"""
from .model import PWCDCNet  # noqa: F401
from .pipeline import ForwardPipeline  # noqa: F401
from .autograd import PWCDCNetModule  # noqa: F401
from .unsup import (census_grad, census_loss, census_sums, fb_consistency_grad, fb_consistency_loss,  # noqa: F401
                    fb_consistency_sums, fb_valid, flow_distill_grad, flow_distill_loss, flow_distill_sums, photometric_loss,
                    photometric_sums, smoothness_loss, smoothness_sums, ssim_grad, ssim_loss, ssim_sums)
from .splat import forward_splat, range_map, range_valid, splat_grad  # noqa: F401
from .compose import chain_flows, compose_flows, compose_grad  # noqa: F401
from . import track  # noqa: F401
from .track import grid_points, track_points  # noqa: F401
from . import interp  # noqa: F401
from .interp import interpolate_frames  # noqa: F401
from . import motion  # noqa: F401
from .motion import fit_motion, motion_residual, smooth_path, warp_frames  # noqa: F401
from . import homography  # noqa: F401
from .homography import fit_homography  # noqa: F401
from . import regions  # noqa: F401
from .regions import label_regions, moving_regions  # noqa: F401
from . import fundamental  # noqa: F401
from .fundamental import epipolar_regions, epipolar_residual, fit_fundamental  # noqa: F401
from . import pose  # noqa: F401
from .pose import camera_pose, flow_depth, triangulate_depth  # noqa: F401
from . import trajectory  # noqa: F401
from .trajectory import camera_trajectory, flow_trajectory  # noqa: F401
from . import pose_refine  # noqa: F401
from .pose_refine import refine_pose  # noqa: F401
from . import region_tracks  # noqa: F401
from .region_tracks import link_regions, region_identities, relabel_regions, track_regions  # noqa: F401
from . import flow_filter  # noqa: F401
from .flow_filter import fill_flow, filter_flow, filter_tables  # noqa: F401
from . import temporal  # noqa: F401
from .temporal import plan_windows, temporal_filter  # noqa: F401
from . import plate  # noqa: F401
from .plate import background_plate, canvas_matrices, plate_canvas, plate_difference, plate_path  # noqa: F401
from . import vis  # noqa: F401
from .vis import flow_error_color, flow_max_radius, flow_to_color, pyramid_montage  # noqa: F401
from .fit import FitInfo, fit_frames, fit_info, flow_any_size, refit_flow  # noqa: F401
from .augment import augment_pairs, crop_params, draw_params  # noqa: F401
from .pyramid import frame_pyramid, level_flow_scale, mask_pyramid  # noqa: F401
from .objective import UnsupObjective  # noqa: F401
from .modules import (ContextNetwork, CostVolumeLayer, FeatureNormLayer, FeaturePyramidExtractor_custom,  # noqa: F401
                      OpticalFlowEstimator_custom, WarpingLayer, resize_bilinear)

__all__ = ["PWCDCNet", "ForwardPipeline", "PWCDCNetModule", "FeaturePyramidExtractor_custom", "WarpingLayer", "CostVolumeLayer",
           "OpticalFlowEstimator_custom", "ContextNetwork", "resize_bilinear", "photometric_sums", "photometric_loss",
           "smoothness_sums", "smoothness_loss", "census_sums", "census_loss", "census_grad", "ssim_sums", "ssim_loss", "ssim_grad", "fb_valid",
           "fb_consistency_sums", "fb_consistency_loss", "fb_consistency_grad", "forward_splat", "splat_grad", "range_map", "range_valid", "FitInfo", "fit_frames", "fit_info",
           "refit_flow", "flow_any_size", "draw_params", "crop_params", "augment_pairs", "frame_pyramid", "mask_pyramid", "level_flow_scale",
           "UnsupObjective", "FeatureNormLayer", "flow_distill_sums", "flow_distill_loss", "flow_distill_grad",
           "compose_flows", "compose_grad", "chain_flows", "vis", "flow_max_radius", "flow_to_color", "flow_error_color", "pyramid_montage",
           "track", "track_points", "grid_points",
           "interp", "interpolate_frames",
           "motion", "fit_motion", "motion_residual", "warp_frames", "smooth_path", "homography", "fit_homography",
           "regions", "label_regions", "moving_regions",
           "fundamental", "fit_fundamental", "epipolar_residual", "epipolar_regions",
           "pose", "camera_pose", "triangulate_depth", "flow_depth",
           "trajectory", "camera_trajectory", "flow_trajectory",
           "pose_refine", "refine_pose",
           "region_tracks", "link_regions", "region_identities", "relabel_regions", "track_regions",
           "flow_filter", "filter_tables", "filter_flow", "fill_flow",
           "temporal", "temporal_filter", "plan_windows",
           "plate", "plate_path", "plate_canvas", "canvas_matrices", "background_plate", "plate_difference"]
