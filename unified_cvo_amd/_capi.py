"""ctypes binding of the C-ABI in include/cvo_hip.h.

The library is the product: there is no Python / CPU fallback.  Importing this module when
libcvo_hip.so is missing raises, loudly.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libcvo_hip.so")

CVO_OK = 0
CVO_RET_FLOW_VANISHED = -1
CVO_E_INVALID = -2
CVO_E_HIP = -3
CVO_E_NOMEM = -4
CVO_E_UNSUPPORTED = -5
CVO_E_VERIFY = -6


class cvo_params_t(C.Structure):
    """Layout-identical to cvo::CvoParams (CvoParams.hpp:12-73) / cvo_params_t (cvo_hip.h)."""

    _fields_ = [
        ("ell_init_first_frame", C.c_float),
        ("ell_init", C.c_float),
        ("ell_min", C.c_float),
        ("min_ell_iter_limit", C.c_int),
        ("ell_max", C.c_float),
        ("dl", C.c_double),
        ("dl_step", C.c_double),
        ("sigma", C.c_float),
        ("sp_thres", C.c_float),
        ("c", C.c_float),
        ("d", C.c_float),
        ("c_ell", C.c_float),
        ("c_sigma", C.c_float),
        ("s_ell", C.c_float),
        ("s_sigma", C.c_float),
        ("MAX_ITER", C.c_int),
        ("eps", C.c_float),
        ("eps_2", C.c_float),
        ("min_step", C.c_float),
        ("max_step", C.c_float),
        ("step", C.c_float),
        ("nearest_neighbors_max", C.c_int),
        ("ell_decay_rate", C.c_float),
        ("ell_decay_rate_first_frame", C.c_float),
        ("ell_decay_start", C.c_int),
        ("ell_decay_start_first_frame", C.c_int),
        ("indicator_window_size", C.c_int),
        ("indicator_stable_threshold", C.c_float),
        ("is_pcl_visualization_on", C.c_int),
        ("is_using_least_square", C.c_int),
        ("is_ell_adaptive", C.c_int),
        ("is_full_ip_matrix", C.c_int),
        ("is_using_geometry", C.c_int),
        ("is_using_intensity", C.c_int),
        ("is_using_semantics", C.c_int),
        ("is_using_range_ell", C.c_int),
        ("is_using_kdtree", C.c_int),
        ("is_exporting_association", C.c_int),
        ("is_using_geometric_type", C.c_int),
        ("multiframe_using_cpu", C.c_int),
        ("multiframe_max_iters", C.c_int),
        ("multiframe_ell_init", C.c_float),
        ("multiframe_ell_min", C.c_float),
        ("multiframe_iter_per_ell", C.c_int),
        ("multiframe_ell_decay_rate", C.c_float),
        ("multiframe_iterations_per_ell", C.c_int),
        ("multiframe_iterations_per_solve", C.c_int),
        ("multiframe_expected_points", C.c_int),
        ("multiframe_downsample_voxel_size", C.c_float),
        ("multiframe_num_neighbors", C.c_int),
        ("multiframe_least_squares_num_threads", C.c_int),
        ("multiframe_min_nonzeros", C.c_int),
    ]


class cvo_trace_t(C.Structure):
    _fields_ = [
        ("k", C.c_int),
        ("K", C.c_int),
        ("ell", C.c_float),
        ("step", C.c_float),
        ("nnz", C.c_uint),
        ("max_nnz", C.c_uint),
        ("omega", C.c_float * 3),
        ("v", C.c_float * 3),
        ("B", C.c_double),
        ("C", C.c_double),
        ("D", C.c_double),
        ("E", C.c_double),
        ("dist", C.c_double),
        ("R", C.c_float * 9),
        ("T", C.c_float * 3),
    ]


class cvo_align_info_t(C.Structure):
    _fields_ = [
        ("iterations", C.c_int),
        ("ret", C.c_int),
        ("final_ell", C.c_float),
        ("final_num_neighbors", C.c_int),
        ("seconds", C.c_double),
    ]


class cvo_align_opts_t(C.Structure):
    _fields_ = [
        ("max_iterations", C.c_int),
        ("override_state", C.c_int),
        ("ell0", C.c_float),
        ("K0", C.c_int),
        ("trace", C.POINTER(cvo_trace_t)),
        ("trace_capacity", C.c_int),
        ("trace_dense", C.c_int),
        ("trace_every", C.c_int),
        ("n_trace", C.POINTER(C.c_int)),
        ("iters_per_launch", C.c_int),
        ("use_graph", C.c_int),
        ("kernel_clock", C.c_int),
    ]


class cvo_multiframe_info_t(C.Structure):
    _fields_ = [
        ("outer_iterations", C.c_int),
        ("solves", C.c_int),
        ("steps", C.c_int),
        ("accepted_steps", C.c_int),
        ("final_ell", C.c_float),
        ("last_total_nonzeros", C.c_uint),
        ("seconds", C.c_double),
    ]


class cvo_multiframe_trace_t(C.Structure):
    _fields_ = [
        ("iter", C.c_int),
        ("n_active_edges", C.c_int),
        ("solved", C.c_int),
        ("steps", C.c_int),
        ("accepted", C.c_int),
        ("termination", C.c_int),
        ("ell", C.c_float),
        ("total_nonzeros", C.c_uint),
        ("cost_initial", C.c_double),
        ("cost_final", C.c_double),
    ]


class cvo_batch_result_t(C.Structure):
    _fields_ = [
        ("ticket", C.c_longlong),
        ("transform", C.c_float * 16),
        ("info", cvo_align_info_t),
    ]


class cvo_rgbd_frame_t(C.Structure):
    _fields_ = [
        ("rows", C.c_int),
        ("cols", C.c_int),
        ("channels", C.c_int),
        ("image", C.c_void_p),
        ("gray", C.c_void_p),
        ("depth", C.c_void_p),
        ("depth_type", C.c_int),
        ("fx", C.c_float),
        ("fy", C.c_float),
        ("cx", C.c_float),
        ("cy", C.c_float),
        ("scaling_factor", C.c_float),
        ("num_classes", C.c_int),
        ("semantic", C.c_void_p),
    ]


class cvo_rgbd_device_frame_t(C.Structure):
    """An RGB-D frame whose planes are in device memory (cvo_cloud_from_rgbd_device) - or, for cvo_rgbd_frame_rows_host, in host
    memory: dense image / gray / depth, class scores with byte strides."""

    _fields_ = [
        ("rows", C.c_int),
        ("cols", C.c_int),
        ("channels", C.c_int),
        ("image", C.c_void_p),
        ("gray", C.c_void_p),
        ("depth", C.c_void_p),
        ("depth_type", C.c_int),
        ("fx", C.c_float),
        ("fy", C.c_float),
        ("cx", C.c_float),
        ("cy", C.c_float),
        ("scaling_factor", C.c_float),
        ("num_classes", C.c_int),
        ("semantic", C.c_void_p),
        ("semantic_row_stride", C.c_size_t),
        ("semantic_pixel_stride", C.c_size_t),
        ("semantic_class_stride", C.c_size_t),
    ]


class cvo_fast_schedule_t(C.Structure):
    _fields_ = [("thresh", C.c_int), ("num_want", C.c_int), ("num_min", C.c_int), ("break_thresh", C.c_int)]


class cvo_stereo_frame_t(C.Structure):
    _fields_ = [
        ("rows", C.c_int),
        ("cols", C.c_int),
        ("channels", C.c_int),
        ("image", C.c_void_p),
        ("gray", C.c_void_p),
        ("disparity", C.c_void_p),
        ("fx", C.c_float),
        ("fy", C.c_float),
        ("cx", C.c_float),
        ("cy", C.c_float),
        ("baseline", C.c_float),
        ("num_classes", C.c_int),
        ("semantic", C.c_void_p),
    ]


class cvo_lidar_scan_t(C.Structure):
    _fields_ = [("n", C.c_int), ("xyzi", C.c_void_p), ("semantic", C.c_void_p), ("num_classes", C.c_int)]


class cvo_lidar_config_t(C.Structure):
    _fields_ = [
        ("n_scan", C.c_int),
        ("horizon_scan", C.c_int),
        ("ang_res_x", C.c_float),
        ("ground_scan_ind", C.c_int),
        ("sensor_min_range", C.c_float),
        ("sensor_mount_angle", C.c_float),
        ("segment_theta", C.c_float),
        ("segment_alpha_x", C.c_float),
        ("segment_alpha_y", C.c_float),
        ("segment_valid_point_num", C.c_int),
        ("segment_valid_line_num", C.c_int),
        ("edge_threshold", C.c_float),
        ("surf_threshold", C.c_float),
        ("intensity_bound", C.c_double),
        ("depth_bound", C.c_double),
        ("distance_bound", C.c_double),
        ("beam_num", C.c_int),
        ("tan_theta", C.c_double),
        ("sin_alpha_x", C.c_double),
        ("cos_alpha_x", C.c_double),
        ("sin_alpha_y", C.c_double),
        ("cos_alpha_y", C.c_double),
        ("tan_ground_lo", C.c_double),
        ("tan_ground_hi", C.c_double),
        ("tan_self_lo", C.c_double),
        ("tan_self_hi", C.c_double),
    ]


class cvo_lidar_rand_t(C.Structure):
    _fields_ = [("r", C.c_uint * 31), ("front", C.c_int), ("rear", C.c_int)]


class cvo_nlm_config_t(C.Structure):
    _fields_ = [("h", C.c_float), ("template_window", C.c_int), ("search_window", C.c_int)]


class cvo_sgm_config_t(C.Structure):
    _fields_ = [("max_disparity", C.c_int), ("p1", C.c_int), ("p2", C.c_int), ("uniqueness", C.c_int), ("lr_max_diff", C.c_int), ("paths", C.c_int)]


class cvo_dfilter_config_t(C.Structure):
    _fields_ = [("speckle_sim_threshold", C.c_float), ("speckle_size", C.c_int), ("ipol_gap_width", C.c_int), ("adaptive_mean", C.c_int)]


class cvo_map_config_t(C.Structure):
    _fields_ = [("resolution", C.c_float), ("block_depth", C.c_int), ("num_classes", C.c_int), ("sf2", C.c_float), ("ell", C.c_float),
                ("prior", C.c_float), ("var_thresh", C.c_float), ("free_thresh", C.c_float), ("occupied_thresh", C.c_float),
                ("ds_resolution", C.c_float), ("free_resolution", C.c_float), ("max_range", C.c_float)]


class cvo_map_query_out_t(C.Structure):
    """Output pointers of cvo_map_query / _query_cloud / _query_host; each may be NULL."""

    _fields_ = [("found", C.c_void_p), ("state", C.c_void_p), ("semantics", C.c_void_p), ("probs", C.c_void_p), ("vars", C.c_void_p),
                ("feat", C.c_void_p), ("centre", C.c_void_p)]


class cvo_map_ray_out_t(C.Structure):
    """Output pointers of cvo_map_raycast(_host); each may be NULL."""

    _fields_ = [("status", C.c_void_p), ("key", C.c_void_p), ("centre", C.c_void_p), ("t", C.c_void_p), ("steps", C.c_void_p),
                ("state", C.c_void_p), ("semantics", C.c_void_p)]


class cvo_map_render_out_t(C.Structure):
    """Output planes of cvo_map_render(_host); each may be NULL."""

    _fields_ = [("depth", C.c_void_p), ("semantics", C.c_void_p), ("feat", C.c_void_p), ("label", C.c_void_p)]


CVO_MAP_STOP_FREE, CVO_MAP_STOP_OCCUPIED, CVO_MAP_STOP_UNKNOWN, CVO_MAP_STOP_ABSENT = 1, 2, 4, 8


class cvo_device_rows_t(C.Structure):
    """Rows of one cloud in device memory (cvo_cloud_from_device): byte strides, optional row indices."""

    _fields_ = [
        ("n", C.c_int),
        ("n_records", C.c_int),
        ("xyz", C.c_void_p),
        ("xyz_stride", C.c_size_t),
        ("feat", C.c_void_p),
        ("feat_stride", C.c_size_t),
        ("label", C.c_void_p),
        ("label_stride", C.c_size_t),
        ("geotype", C.c_void_p),
        ("geotype_stride", C.c_size_t),
        ("rows", C.c_void_p),
    ]


CVO_DEPTH_U16, CVO_DEPTH_F32 = 0, 1
CVO_SELECT_CV_FAST, CVO_SELECT_DSO_EDGES, CVO_SELECT_FULL = 0, 2, 8
CVO_FAST_RGBD, CVO_FAST_STEREO, CVO_FAST_STEREO_SEMANTIC = (9, 15000, 12000, 13), (4, 24000, 15000, 50), (4, 28000, 15000, 50)

# every symbol include/cvo_hip.h declares (tests/test_capi_symbols.py checks the two lists agree)
EXPORTED = [
    "cvo_params_default", "cvo_ctx_create", "cvo_ctx_destroy", "cvo_last_error", "cvo_ctx_stream",
    "cvo_ctx_synchronize", "cvo_cloud_upload", "cvo_cloud_upload_aos192", "cvo_cloud_size", "cvo_cloud_free",
    "cvo_align", "cvo_align_ex", "cvo_align_batch", "cvo_batch_poses_to_device", "cvo_inner_product",
    "cvo_function_angle", "cvo_association", "cvo_association_non_isotropic", "cvo_cloud_transformed", "cvo_edge_kernel_matrix", "cvo_debug_last_ell", "cvo_debug_time_scan", "cvo_debug_time_kernels",
    "cvo_debug_kernel_clock",
    "cvo_debug_last_candidates", "cvo_debug_list_builds", "cvo_debug_row_classes", "cvo_debug_speculation", "cvo_debug_scan_stats", "cvo_debug_last_geometry", "cvo_version",
    "cvo_align_association", "cvo_debug_scalar_math", "cvo_debug_prim", "cvo_debug_verified_rows", "cvo_debug_device_memory", "cvo_cloud_upload_many",
    "cvo_ctx_set_option", "cvo_ctx_advice", "cvo_debug_cloud_order",
    "cvo_debug_cloud_order_route", "cvo_debug_order_route_rule", "cvo_debug_wide_plan",
    "cvo_debug_wide_plan_at", "cvo_debug_cloud_wide_pivots",
    "cvo_process_hint_hw_queues", "cvo_shutdown",
    "cvo_batch_open", "cvo_batch_submit", "cvo_batch_poll", "cvo_batch_pending", "cvo_batch_stats", "cvo_batch_close",
    "cvo_inner_product_batch", "cvo_function_angle_batch", "cvo_debug_last_score_batch", "cvo_debug_cloud_tiles",
    "cvo_multiframe_align", "cvo_debug_irls_normal", "cvo_debug_irls_eval", "cvo_debug_irls_gather",
    "cvo_voxel_select", "cvo_voxel_select_host", "cvo_cloud_upload_voxel", "cvo_debug_voxel_stats",
    "cvo_rgbd_points", "cvo_rgbd_points_host", "cvo_cloud_upload_rgbd", "cvo_debug_rgbd_stats",
    "cvo_debug_rgbd_readback",
    "cvo_fast_select", "cvo_fast_select_host", "cvo_stereo_points", "cvo_stereo_points_host", "cvo_cloud_upload_stereo",
    "cvo_cloud_upload_stereo_recipe", "cvo_debug_stereo_stats",
    "cvo_lidar_config_default", "cvo_lidar_config_derive", "cvo_lidar_rand_seed", "cvo_lidar_rand_next", "cvo_lidar_select", "cvo_lidar_select_host",
    "cvo_cloud_upload_lidar", "cvo_debug_lidar_stats", "cvo_debug_lidar_atan2",
    "cvo_nlm_config_default", "cvo_nlm_weights", "cvo_nlm_denoise_host", "cvo_nlm_denoise", "cvo_nlm_denoise_lab_host",
    "cvo_nlm_denoise_lab", "cvo_debug_nlm_stats",
    "cvo_sgm_config_default", "cvo_stereo_disparity_host", "cvo_stereo_disparity", "cvo_cloud_upload_stereo_pair", "cvo_debug_sgm_stats",
    "cvo_debug_sgm_readback",
    "cvo_dfilter_config_default", "cvo_disparity_filter_host", "cvo_disparity_filter", "cvo_stereo_disparity_filtered",
    "cvo_cloud_upload_stereo_pair_filtered", "cvo_debug_dfilter_stats",
    "cvo_map_config_default", "cvo_map_open", "cvo_map_close", "cvo_map_insert", "cvo_map_insert_posed", "cvo_map_size", "cvo_map_cloud",
    "cvo_map_open_host", "cvo_map_close_host", "cvo_map_insert_host", "cvo_map_cloud_host", "cvo_debug_map_stats",
    "cvo_cloud_from_device", "cvo_cloud_from_device_many", "cvo_cloud_from_device_aos192",
    "cvo_debug_device_buffer", "cvo_debug_device_release",
    "cvo_cloud_merge", "cvo_cloud_download",
    "cvo_map_insert_cloud", "cvo_map_cloud_resident", "cvo_map_set_kernel",
    "cvo_map_query", "cvo_map_query_cloud", "cvo_map_query_host", "cvo_map_raycast", "cvo_map_raycast_host",
    "cvo_map_render", "cvo_map_render_host",
    "cvo_depth_filter_open", "cvo_depth_filter_add", "cvo_depth_filter_size", "cvo_depth_filter_state", "cvo_depth_filter_finish",
    "cvo_depth_filter_close", "cvo_depth_filter", "cvo_depth_filter_accumulate_host", "cvo_depth_filter_finish_host",
    "cvo_debug_depth_filter_rows",
    "cvo_cloud_from_rgbd_device", "cvo_cloud_from_rgbd_device_recipe", "cvo_rgbd_frame_rows_host",
]

_libs = {}


def lib(path=None):
    """Loads libcvo_hip.so (once; `path`: another build of the same C-ABI, e.g. an experiment build of build.build_variant).  Raises if the
    HIP extension has not been built."""
    path = os.path.abspath(path) if path else LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: build it with `python -m unified_cvo_amd.build` "
            "(there is no CPU fallback for the hot path)")
    L = C.CDLL(path)
    vp, ip, fp = C.c_void_p, C.c_int, C.POINTER(C.c_float)
    L.cvo_version.restype = C.c_char_p
    L.cvo_params_default.argtypes = [C.POINTER(cvo_params_t)]
    L.cvo_params_default.restype = None
    L.cvo_ctx_create.argtypes = [ip, C.POINTER(vp)]
    L.cvo_ctx_destroy.argtypes = [vp]
    L.cvo_ctx_destroy.restype = None
    L.cvo_ctx_set_option.argtypes = [vp, C.c_char_p, C.c_char_p]
    L.cvo_last_error.argtypes = [vp]
    L.cvo_last_error.restype = C.c_char_p
    L.cvo_ctx_advice.argtypes = [vp]
    L.cvo_ctx_advice.restype = C.c_char_p
    L.cvo_ctx_stream.argtypes = [vp]
    L.cvo_ctx_stream.restype = vp
    L.cvo_ctx_synchronize.argtypes = [vp]
    L.cvo_cloud_upload.argtypes = [vp, ip, fp, fp, fp, fp, C.POINTER(vp)]
    L.cvo_cloud_upload_aos192.argtypes = [vp, ip, vp, C.POINTER(vp)]
    L.cvo_cloud_upload_many.argtypes = [vp, ip, C.POINTER(C.c_int), C.POINTER(fp), C.POINTER(fp), C.POINTER(fp),
                                        C.POINTER(fp), ip, C.POINTER(vp)]
    L.cvo_cloud_size.argtypes = [vp]
    L.cvo_cloud_free.argtypes = [vp]
    L.cvo_cloud_free.restype = None
    L.cvo_align.argtypes = [vp, C.POINTER(cvo_params_t), vp, vp, fp, fp, C.POINTER(cvo_align_info_t)]
    L.cvo_align_ex.argtypes = [vp, C.POINTER(cvo_params_t), vp, vp, fp, fp, C.POINTER(cvo_align_info_t),
                               C.POINTER(cvo_align_opts_t)]
    L.cvo_align_batch.argtypes = [vp, C.POINTER(cvo_params_t), ip, C.POINTER(vp), C.POINTER(vp), fp, fp,
                                  C.POINTER(cvo_align_info_t), C.POINTER(cvo_align_opts_t)]
    L.cvo_batch_poses_to_device.argtypes = [vp, vp, ip]
    L.cvo_batch_open.argtypes = [vp, C.POINTER(cvo_params_t), ip, ip, ip, ip, C.POINTER(cvo_align_opts_t), C.POINTER(vp)]
    L.cvo_batch_submit.argtypes = [vp, vp, vp, fp, ip, C.POINTER(C.c_longlong)]
    L.cvo_batch_poll.argtypes = [vp, ip, ip, C.POINTER(cvo_batch_result_t), C.POINTER(C.c_int)]
    L.cvo_batch_pending.argtypes = [vp]
    L.cvo_batch_stats.argtypes = [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    L.cvo_batch_close.argtypes = [vp]
    L.cvo_batch_close.restype = None
    L.cvo_inner_product.argtypes = [vp, C.POINTER(cvo_params_t), vp, vp, fp, C.c_float, fp]
    L.cvo_function_angle.argtypes = [vp, C.POINTER(cvo_params_t), vp, vp, fp, C.c_float, ip, fp]
    L.cvo_inner_product_batch.argtypes = [vp, C.POINTER(cvo_params_t), ip, C.POINTER(vp), C.POINTER(vp), fp, fp, fp]
    L.cvo_function_angle_batch.argtypes = [vp, C.POINTER(cvo_params_t), ip, C.POINTER(vp), C.POINTER(vp), fp, fp, ip, fp]
    L.cvo_debug_last_score_batch.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.cvo_association.argtypes = [vp, C.POINTER(cvo_params_t), vp, vp, fp, C.c_float, C.POINTER(C.c_int),
                                  C.POINTER(C.c_int), fp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.cvo_association_non_isotropic.argtypes = [vp, C.POINTER(cvo_params_t), vp, vp, fp, fp, C.POINTER(C.c_int),
                                                 C.POINTER(C.c_int), fp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.cvo_cloud_transformed.argtypes = [vp, vp, fp, C.POINTER(vp)]
    L.cvo_edge_kernel_matrix.argtypes = [vp, C.POINTER(cvo_params_t), vp, vp, C.c_float, ip, fp, C.POINTER(C.c_int), C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    L.cvo_debug_last_ell.argtypes = [vp, ip, fp, C.POINTER(C.c_int), C.POINTER(C.c_uint)]
    L.cvo_debug_time_scan.argtypes = [vp, ip, fp]
    L.cvo_debug_time_kernels.argtypes = [vp, ip, fp, fp]
    L.cvo_debug_kernel_clock.argtypes = [vp, fp, fp, C.POINTER(C.c_ulonglong)]
    L.cvo_debug_last_candidates.argtypes = [vp, C.POINTER(C.c_ulonglong)]
    L.cvo_debug_list_builds.argtypes = [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    L.cvo_debug_row_classes.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.cvo_debug_speculation.argtypes = [vp, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.cvo_debug_last_geometry.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.cvo_debug_scan_stats.argtypes = [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.cvo_align_association.argtypes = [vp, ip, C.POINTER(C.c_int), C.POINTER(C.c_int), fp, C.c_size_t,
                                        C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.cvo_debug_scalar_math.argtypes = [vp, ip, ip, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.cvo_debug_prim.argtypes = [vp, ip, ip, ip, C.POINTER(C.c_ulonglong), C.c_size_t, C.POINTER(C.c_uint), C.c_size_t, C.POINTER(C.c_uint), C.c_size_t]
    L.cvo_debug_verified_rows.argtypes = [vp, C.POINTER(C.c_ulonglong)]
    L.cvo_debug_device_memory.argtypes = [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.cvo_debug_cloud_order.argtypes = [vp, C.POINTER(C.c_int)]
    L.cvo_debug_cloud_order_route.argtypes = [vp]
    L.cvo_debug_cloud_tiles.argtypes = [vp, vp, fp, C.POINTER(C.c_int)]
    L.cvo_debug_order_route_rule.argtypes = [ip, ip, C.c_char_p, ip]
    L.cvo_debug_wide_plan.argtypes = [ip, C.POINTER(C.c_int), C.POINTER(C.c_int), ip, C.POINTER(C.c_int)]
    L.cvo_debug_wide_plan_at.argtypes = [ip, ip, C.POINTER(C.c_int), ip, C.POINTER(C.c_int)]
    L.cvo_debug_cloud_wide_pivots.argtypes = [vp, ip, C.POINTER(C.c_uint), C.POINTER(C.c_uint), C.POINTER(C.c_int)]
    dp = C.POINTER(C.c_double)
    L.cvo_multiframe_align.argtypes = [vp, C.POINTER(cvo_params_t), ip, C.POINTER(vp), dp, C.POINTER(C.c_int), ip,
                                       C.POINTER(C.c_int), C.POINTER(cvo_multiframe_info_t),
                                       C.POINTER(cvo_multiframe_trace_t), ip, C.POINTER(C.c_int)]
    L.cvo_debug_irls_normal.argtypes = [vp, vp, vp, dp, dp, dp]
    ipp = C.POINTER(C.c_int)
    L.cvo_debug_irls_eval.argtypes = [vp, ip, C.POINTER(vp), dp, ip, ipp, ipp, ipp, ipp, fp, ip, dp]
    L.cvo_debug_irls_gather.argtypes = [vp, ip, ipp, ipp, fp]
    L.cvo_voxel_select.argtypes = [vp, ip, fp, C.c_float, ipp, ipp]
    L.cvo_voxel_select_host.argtypes = [ip, fp, C.c_float, ipp, ipp]
    L.cvo_cloud_upload_voxel.argtypes = [vp, ip, fp, fp, fp, fp, C.c_float, C.POINTER(vp), ipp, ipp]
    L.cvo_debug_voxel_stats.argtypes = [vp] + [C.POINTER(C.c_ulonglong)] * 5
    fr = C.POINTER(cvo_rgbd_frame_t)
    L.cvo_rgbd_points.argtypes = [vp, fr, ip, ipp, ipp, fp, fp, fp, fp]
    L.cvo_rgbd_points_host.argtypes = [fr, ip, ipp, ipp, fp, fp, fp, fp]
    L.cvo_cloud_upload_rgbd.argtypes = [vp, fr, C.c_float, C.c_float, C.POINTER(vp), ipp, C.POINTER(C.c_ubyte), ipp]
    dfr = C.POINTER(cvo_rgbd_device_frame_t)
    L.cvo_cloud_from_rgbd_device.argtypes = [vp, dfr, C.c_int, C.POINTER(vp), ipp, ipp]
    L.cvo_cloud_from_rgbd_device_recipe.argtypes = [vp, dfr, C.c_float, C.c_float, C.POINTER(vp), ipp, ipp, ipp]
    L.cvo_rgbd_frame_rows_host.argtypes = [dfr, C.c_int, C.c_int, C.c_int, ipp, C.POINTER(C.c_ubyte), fp, fp, fp, fp, C.POINTER(C.c_ubyte)]
    L.cvo_debug_rgbd_stats.argtypes = [vp, ipp, ipp, ipp] + [C.POINTER(C.c_ulonglong)] * 4 + [ipp]
    L.cvo_debug_rgbd_readback.argtypes = [vp, ipp, ipp, ipp, fp, fp, fp, ipp]
    sched, sf, up = C.POINTER(cvo_fast_schedule_t), C.POINTER(cvo_stereo_frame_t), C.POINTER(C.c_ubyte)
    L.cvo_fast_select.argtypes = [vp, ip, ip, up, sched, ipp, ipp, ipp]
    L.cvo_fast_select_host.argtypes = [ip, ip, up, sched, ipp, ipp, ipp]
    L.cvo_stereo_points.argtypes = [vp, sf, ip, ipp, ipp, fp, fp, fp, fp]
    L.cvo_stereo_points_host.argtypes = [sf, ip, ipp, ipp, fp, fp, fp, fp]
    L.cvo_cloud_upload_stereo.argtypes = [vp, sf, ip, C.POINTER(vp), ipp, ipp]
    L.cvo_cloud_upload_stereo_recipe.argtypes = [vp, sf, C.c_float, C.c_float, C.POINTER(vp), ipp, up, ipp]
    L.cvo_debug_stereo_stats.argtypes = [vp, ip, ipp, ipp, ipp, ipp, C.POINTER(C.c_uint)] + [C.POINTER(C.c_ulonglong)] * 2 + [ipp]
    ls, lc, lr = C.POINTER(cvo_lidar_scan_t), C.POINTER(cvo_lidar_config_t), C.POINTER(cvo_lidar_rand_t)
    L.cvo_lidar_config_default.argtypes = [lc, ip]
    L.cvo_lidar_config_default.restype = None
    L.cvo_lidar_config_derive.argtypes = [lc]
    L.cvo_lidar_config_derive.restype = None
    L.cvo_lidar_rand_seed.argtypes = [lr, C.c_uint]
    L.cvo_lidar_rand_seed.restype = None
    L.cvo_lidar_rand_next.argtypes = [lr]
    L.cvo_lidar_rand_next.restype = C.c_uint
    L.cvo_debug_lidar_atan2.argtypes = [ip, dp, dp, dp]
    L.cvo_lidar_select_host.argtypes = [ls, lc, lr, ipp, up, ipp]
    L.cvo_lidar_select.argtypes = [vp, ls, lc, lr, ipp, up, ipp]
    L.cvo_cloud_upload_lidar.argtypes = [vp, ls, lc, lr, C.POINTER(vp), ipp, ipp]
    L.cvo_debug_lidar_stats.argtypes = [vp, C.POINTER(C.c_ulonglong), ipp]
    nc, bp = C.POINTER(cvo_nlm_config_t), C.POINTER(C.c_ubyte)
    L.cvo_nlm_config_default.argtypes = [nc]
    L.cvo_nlm_config_default.restype = None
    L.cvo_nlm_weights.argtypes = [nc, ip, ipp, ip, ipp, ipp, ipp, ipp]
    L.cvo_nlm_denoise_host.argtypes = [ip, ip, ip, bp, nc, bp]
    L.cvo_nlm_denoise.argtypes = [vp, ip, ip, ip, bp, nc, bp]
    L.cvo_nlm_denoise_lab_host.argtypes = [ip, ip, bp, nc, C.c_float, bp]
    L.cvo_nlm_denoise_lab.argtypes = [vp, ip, ip, bp, nc, C.c_float, bp]
    L.cvo_debug_nlm_stats.argtypes = [vp] + [ipp] * 7
    sc, fp = C.POINTER(cvo_sgm_config_t), C.POINTER(C.c_float)
    L.cvo_sgm_config_default.argtypes = [sc]
    L.cvo_sgm_config_default.restype = None
    L.cvo_stereo_disparity_host.argtypes = [ip, ip, bp, bp, sc, fp]
    L.cvo_stereo_disparity.argtypes = [vp, ip, ip, bp, bp, sc, fp]
    L.cvo_cloud_upload_stereo_pair.argtypes = [vp, C.POINTER(cvo_stereo_frame_t), bp, sc, ip, C.POINTER(vp), ipp, ipp]
    L.cvo_debug_sgm_stats.argtypes = [vp] + [ipp] * 8
    L.cvo_debug_sgm_readback.argtypes = [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.POINTER(C.c_ushort)]
    dc = C.POINTER(cvo_dfilter_config_t)
    L.cvo_dfilter_config_default.argtypes = [dc]
    L.cvo_dfilter_config_default.restype = None
    L.cvo_disparity_filter_host.argtypes = [ip, ip, fp, dc, fp]
    L.cvo_disparity_filter.argtypes = [vp, ip, ip, fp, dc, fp]
    L.cvo_stereo_disparity_filtered.argtypes = [vp, ip, ip, bp, bp, sc, dc, fp]
    L.cvo_cloud_upload_stereo_pair_filtered.argtypes = [vp, C.POINTER(cvo_stereo_frame_t), bp, sc, dc, ip, C.POINTER(vp), ipp, ipp]
    L.cvo_debug_dfilter_stats.argtypes = [vp] + [ipp] * 5 + [C.POINTER(C.c_ulonglong), fp, fp, fp]
    mc, ll, llp = C.POINTER(cvo_map_config_t), C.c_longlong, C.POINTER(C.c_longlong)
    L.cvo_map_config_default.argtypes = [mc]
    L.cvo_map_config_default.restype = None
    L.cvo_map_open.argtypes = [vp, mc, ll, C.POINTER(vp)]
    L.cvo_map_open_host.argtypes = [mc, C.POINTER(vp)]
    L.cvo_map_close.argtypes = [vp]
    L.cvo_map_close.restype = None
    L.cvo_map_close_host.argtypes = [vp]
    L.cvo_map_close_host.restype = None
    L.cvo_map_insert.argtypes = [vp, ip, fp, fp, fp, fp]
    L.cvo_map_insert_host.argtypes = [vp, ip, fp, fp, fp, fp]
    L.cvo_map_insert_posed.argtypes = [vp, ip, fp, fp, fp, fp]
    L.cvo_map_size.argtypes = [vp, llp, llp]
    L.cvo_map_cloud.argtypes = [vp, ll, fp, fp, fp, llp, C.POINTER(vp)]
    L.cvo_map_cloud_host.argtypes = [vp, ll, fp, fp, fp, llp]
    L.cvo_debug_map_stats.argtypes = [vp, ipp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), fp, fp]
    dr = C.POINTER(cvo_device_rows_t)
    L.cvo_cloud_from_device.argtypes = [vp, dr, C.POINTER(vp)]
    L.cvo_cloud_from_device_many.argtypes = [vp, ip, dr, C.POINTER(vp)]
    L.cvo_cloud_from_device_aos192.argtypes = [vp, ip, vp, C.POINTER(vp)]
    L.cvo_debug_device_buffer.argtypes = [vp, C.c_size_t, vp, C.POINTER(vp)]
    L.cvo_debug_device_release.argtypes = [vp, vp]
    L.cvo_cloud_merge.argtypes = [vp, ip, C.POINTER(vp), dp, C.c_float, C.POINTER(vp), ipp, ipp]
    L.cvo_cloud_download.argtypes = [vp, vp, fp, fp, fp, fp, ipp]
    L.cvo_map_insert_cloud.argtypes = [vp, vp, fp, fp]
    L.cvo_map_set_kernel.argtypes = [vp, C.c_int]
    L.cvo_map_cloud_resident.argtypes = [vp, C.POINTER(vp), llp]
    qo, ro, vo = C.POINTER(cvo_map_query_out_t), C.POINTER(cvo_map_ray_out_t), C.POINTER(cvo_map_render_out_t)
    L.cvo_map_query.argtypes = [vp, ip, fp, qo]
    L.cvo_map_query_host.argtypes = [vp, ip, fp, qo]
    L.cvo_map_query_cloud.argtypes = [vp, vp, fp, qo]
    L.cvo_map_raycast.argtypes = [vp, ip, fp, fp, C.c_uint, ip, ro]
    L.cvo_map_raycast_host.argtypes = [vp, ip, fp, fp, C.c_uint, ip, ro]
    L.cvo_map_render.argtypes = [vp, fp] + [C.c_float] * 4 + [ip, ip, C.c_float, C.c_uint, vo]
    L.cvo_map_render_host.argtypes = [vp, fp] + [C.c_float] * 4 + [ip, ip, C.c_float, C.c_uint, vo]
    pp = C.POINTER(cvo_params_t)
    L.cvo_depth_filter_open.argtypes = [vp, vp, C.POINTER(vp)]
    L.cvo_depth_filter_add.argtypes = [vp, pp, vp, fp, fp, fp]
    L.cvo_depth_filter_size.argtypes = [vp]
    L.cvo_depth_filter_state.argtypes = [vp, fp, fp, ipp]
    L.cvo_depth_filter_finish.argtypes = [vp, ip, C.POINTER(vp), ipp, fp, ipp, ipp]
    L.cvo_depth_filter_close.argtypes = [vp]
    L.cvo_depth_filter_close.restype = None
    L.cvo_depth_filter.argtypes = [vp, pp, vp, ip, C.POINTER(vp), fp, fp, fp, ip, C.POINTER(vp), ipp, fp, ipp, ipp]
    L.cvo_depth_filter_accumulate_host.argtypes = [ip, ipp, ipp, fp, ip, fp, fp, fp, fp, ipp]
    L.cvo_depth_filter_finish_host.argtypes = [ip, fp, fp, fp, ipp, ip, fp, ipp, fp, ipp, ipp]
    L.cvo_debug_depth_filter_rows.argtypes = [vp] + [ipp] * 8
    for name in EXPORTED:
        getattr(L, name)  # AttributeError here = the library does not export what the header declares
    _libs[path] = L
    return L
