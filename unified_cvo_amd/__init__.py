"""unified_cvo_amd -- MI355X (gfx950) backend for unified_cvo's pairwise SE(3) kernel-correlation path.

Only what the path needs: csrc/ (HIP kernels + the C-ABI of include/cvo_hip.h) and the host-side
mirror of the reference interface (CvoGPU / CvoPointCloud / CvoParams).
"""
from .params import CvoParams, read_cvo_params_yaml, parse_cvo_yaml_text  # noqa: F401
from .api import (CvoGPU, CvoPointCloud, DeviceCloud, DeviceCloudAoS, CvoError, AlignResult, CvoFrameGPU,  # noqa: F401
                  BinaryStateGPU, CVO_POINT_DTYPE, cvo_points_from_pointcloud, RGBDFrame, rgbd_points_host, StereoFrame, fast_select_host,
                  stereo_points_host, LidarScan, LidarConfig, LidarRand, lidar_select_host, debug_lidar_atan2,
                  debug_order_route_rule, debug_wide_plan, debug_wide_plan_at,
                  nlm_weights, nlm_denoise_host, nlm_denoise_lab_host,
                  SGMConfig, stereo_disparity_host, DFilterConfig, disparity_filter_host,
                  MapConfig, SemanticMap, MapQuery, MapRays, MapView, map_open_host, map_insert_host, map_cloud_host, map_close_host,
                  DepthFilter, depth_filter_accumulate_host, depth_filter_finish_host,
                  DeviceRGBDFrame, rgbd_frame_rows_host)
