"""extractorb_amd — MI355X-native ORB feature extraction (host-side mirror of the reference interface).

The compute lives in ``liborbx.so`` (hand-written HIP kernels behind the C ABI of ``include/orbx.h``);
this package only binds it with ctypes and mirrors ``ORB_SLAM3::ORBextractor``
(reference inc/ORBextractor.h:44-111) so Python callers and the tests read like the reference's callers.

There is no CPU fallback: importing works anywhere (so the C ABI can be inspected), but constructing an
extractor without the built library or without a HIP device raises.
"""
from .orbextractor import (KEYPOINT_DTYPE, ORBextractor, OrbxError, build_library, library_path, load_library,
                           compute_tables, describe_tables, describe_levels, DESCRIBE_LEVEL_FIELDS, compute_level_sizes, compute_cell_grid, header_symbols, camera, camera_kb8,
                           compute_image_bounds, pinned_empty, pinned_free, source_hash, Vocabulary, debug_set_option,
                           debug_reset_options, predict_scale, predict_scale_breakpoints, sim3_hamming_bound, PROJ_QUERY_DTYPE,
                           TRACK_RECORD_DTYPE, FRUSTUM_LOCAL_MAP, FRUSTUM_RELOCALIZATION, FRUSTUM_FLAG, FRUSTUM_NEG_DEPTH,
                           FRUSTUM_NOT_IN_IMAGE, FRUSTUM_DISTANCE, FRUSTUM_VIEW_COS, FRUSTUM_FAR, FRUSTUM_REQUEST, TWO_VIEW_RESULT_DTYPE,
                           TWO_VIEW_STATUS, SIM3_PROBLEM_DTYPE, SIM3_RESULT_DTYPE, SIM3_STATUS, POSE_PROBLEM_DTYPE, POSE_RESULT_DTYPE,
                           POSE_OPTIMIZATION_STATUS, PLACE_RESULT_DTYPE, PLACE_N_BEST, PLACE_RELOCALIZATION, PLACE_STATUS,
                           COVIS_RESULT_DTYPE, REDUNDANCY_RESULT_DTYPE, COVIS_UPDATE_CONNECTIONS, COVIS_LOCAL_KEYFRAMES, COVIS_STATUS,
                           REDUNDANCY_STATUS)

__all__ = ["KEYPOINT_DTYPE", "ORBextractor", "OrbxError", "build_library", "library_path", "load_library",
           "compute_tables", "describe_tables", "describe_levels", "DESCRIBE_LEVEL_FIELDS", "compute_level_sizes", "compute_cell_grid", "header_symbols", "camera", "camera_kb8", "compute_image_bounds", "pinned_empty", "pinned_free", "source_hash", "Vocabulary",
           "debug_set_option", "debug_reset_options", "predict_scale", "predict_scale_breakpoints", "sim3_hamming_bound",
           "PROJ_QUERY_DTYPE", "TRACK_RECORD_DTYPE", "FRUSTUM_LOCAL_MAP", "FRUSTUM_RELOCALIZATION", "FRUSTUM_FLAG", "FRUSTUM_NEG_DEPTH",
           "FRUSTUM_NOT_IN_IMAGE", "FRUSTUM_DISTANCE", "FRUSTUM_VIEW_COS", "FRUSTUM_FAR", "FRUSTUM_REQUEST", "TWO_VIEW_RESULT_DTYPE", "TWO_VIEW_STATUS",
           "SIM3_PROBLEM_DTYPE", "SIM3_RESULT_DTYPE", "SIM3_STATUS", "POSE_PROBLEM_DTYPE", "POSE_RESULT_DTYPE",
           "POSE_OPTIMIZATION_STATUS", "PLACE_RESULT_DTYPE", "PLACE_N_BEST", "PLACE_RELOCALIZATION", "PLACE_STATUS",
           "COVIS_RESULT_DTYPE", "REDUNDANCY_RESULT_DTYPE", "COVIS_UPDATE_CONNECTIONS", "COVIS_LOCAL_KEYFRAMES", "COVIS_STATUS", "REDUNDANCY_STATUS"]
__version__ = "0.1.0"
