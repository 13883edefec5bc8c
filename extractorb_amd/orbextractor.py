"""ctypes binding of liborbx.so and the Python mirror of ORB_SLAM3::ORBextractor.

Reference interface mirrored here: inc/ORBextractor.h:44-111 (constructor, operator(), scale getters,
mvImagePyramid), called from Frame::ExtractORB (src/Frame.cc:419-427).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
_LIB = os.environ.get("ORBX_LIBRARY") or os.path.join(_PKG, "liborbx.so")   # ORBX_LIBRARY: another build of the same library (tuning experiments)
_HEADER = os.path.join(_ROOT, "include", "orbx.h")

# numpy mirror of cv::KeyPoint / orbx_keypoint (28 bytes)
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KEYPOINT_DTYPE.itemsize == 28
# orbx_proj_query: one search request of orbx_search_by_projection_device (32 bytes)
PROJ_QUERY_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("radius", "<f4"), ("min_level", "<i4"), ("max_level", "<i4"),
                             ("flags", "<i4"), ("angle", "<f4")])
# orbx_track_record: what Frame::isInFrustum leaves in a MapPoint (28 bytes); mbTrackInView is exit >= FRUSTUM_FAR
TRACK_RECORD_DTYPE = np.dtype([("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("depth", "<f4"), ("view_cos", "<f4"),
                               ("level", "<i4"), ("exit", "<i4")])
assert PROJ_QUERY_DTYPE.itemsize == 32 and TRACK_RECORD_DTYPE.itemsize == 28
# == orbx_two_view_result / enum orbx_two_view_status
TWO_VIEW_RESULT_DTYPE = np.dtype([("status", "<i4"), ("model", "<i4"), ("n_matches", "<i4"), ("best_it_h", "<i4"), ("best_it_f", "<i4"),
                                  ("n_inliers", "<i4"), ("chosen", "<i4"), ("SH", "<f4"), ("SF", "<f4"), ("RH", "<f4"), ("H21", "<f4", 9),
                                  ("F21", "<f4", 9), ("R21", "<f4", 9), ("t21", "<f4", 3), ("n_good", "<i4", 8), ("parallax", "<f4", 8)])
assert TWO_VIEW_RESULT_DTYPE.itemsize == 224
TWO_VIEW_STATUS = ("ACCEPTED_H", "ACCEPTED_F", "TOO_FEW_MATCHES", "BAD_INDEX", "ZERO_SCORES", "H_DEGENERATE", "H_AMBIGUOUS", "H_LOW_PARALLAX",
                   "H_FEW_POINTS", "H_BELOW_INLIER_SHARE", "F_FEW_POINTS", "F_AMBIGUOUS", "F_LOW_PARALLAX")
# == orbx_sim3_problem / orbx_sim3_result / enum orbx_sim3_solve_status
SIM3_PROBLEM_DTYPE = np.dtype([("n1", "<i4"), ("fix_scale", "<i4"), ("model1", "<i4"), ("model2", "<i4"), ("cam1", "<f4", 8), ("cam2", "<f4", 8),
                               ("Tcw1", "<f4", 12), ("Tcw2", "<f4", 12), ("level_sigma2", "<f4", 16)])
SIM3_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n", "<i4"), ("max_its", "<i4"), ("iterations", "<i4"), ("best_it", "<i4"), ("n_inliers", "<i4"),
                              ("best_inliers", "<i4"), ("scale", "<f4"), ("R", "<f4", 9), ("t", "<f4", 3), ("T12", "<f4", 16)])
assert SIM3_PROBLEM_DTYPE.itemsize == 240 and SIM3_RESULT_DTYPE.itemsize == 144
SIM3_STATUS = ("CONVERGED", "NO_MORE", "TOO_FEW", "BAD_ARGUMENT")
# == orbx_pose_problem / orbx_pose_result / enum orbx_pose_optimization_status
POSE_PROBLEM_DTYPE = np.dtype([("model", "<i4"), ("model2", "<i4"), ("cam", "<f4", 8), ("cam2", "<f4", 8), ("mbf", "<f4"), ("Trl", "<f4", 12),
                               ("inv_level_sigma2", "<f4", 16)])
POSE_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_initial", "<i4"), ("n_bad", "<i4"), ("n_inliers", "<i4"), ("rounds", "<i4"),
                              ("empty_rounds", "<i4"), ("its", "<i4", 4), ("trials", "<i4", 4), ("lambda", "<f8", 4), ("chi2", "<f8", 4)])
assert POSE_PROBLEM_DTYPE.itemsize == 188 and POSE_RESULT_DTYPE.itemsize == 120
POSE_OPTIMIZATION_STATUS = ("ALL_ROUNDS", "FEW_EDGES", "TOO_FEW", "BAD_ARGUMENT")
# == orbx_place_result / enum orbx_place_mode / enum orbx_place_status
PLACE_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_sharing", "<i4"), ("max_common_words", "<i4"), ("min_common_words", "<i4"),
                               ("n_scored", "<i4"), ("best_acc_score", "<f4"), ("n_loop", "<i4"), ("n_merge", "<i4")])
assert PLACE_RESULT_DTYPE.itemsize == 32
PLACE_N_BEST, PLACE_RELOCALIZATION = 0, 1
PLACE_STATUS = ("OK", "NO_SHARING", "NONE_SCORED", "EMPTY_DATABASE", "EMPTY_QUERY", "BAD_KEYFRAME", "TRUNCATED")
# == orbx_covis_result / orbx_redundancy_result / enum orbx_covis_mode / orbx_covis_status / orbx_redundancy_status
COVIS_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_counter", "<i4"), ("n_ordered", "<i4"), ("nmax", "<i4"), ("kf_max", "<i4")])
REDUNDANCY_RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_mps", "<i4"), ("n_redundant", "<i4"), ("redundant", "<i4")])
assert COVIS_RESULT_DTYPE.itemsize == 20 and REDUNDANCY_RESULT_DTYPE.itemsize == 16
COVIS_UPDATE_CONNECTIONS, COVIS_LOCAL_KEYFRAMES = 0, 1
COVIS_STATUS = ("OK", "EMPTY", "TRUNCATED", "BAD_INDEX", "DUPLICATE_KEY")
REDUNDANCY_STATUS = ("OK", "SKIPPED", "BAD_INDEX")
FRUSTUM_LOCAL_MAP, FRUSTUM_RELOCALIZATION = 0, 1      # orbx_frustum_mode
(FRUSTUM_FLAG, FRUSTUM_NEG_DEPTH, FRUSTUM_NOT_IN_IMAGE, FRUSTUM_DISTANCE, FRUSTUM_VIEW_COS, FRUSTUM_FAR,
 FRUSTUM_REQUEST) = range(7)                           # orbx_frustum_exit

ORBX_OK = 0
ORBX_ERR_EMPTY_IMAGE = -1
ORBX_NUM_KERNELS = 10


class OrbxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("orbx error %d: %s" % (code, msg))
        self.code = code


def library_path():
    return _LIB


def build_library(force=False):
    """Compiles liborbx.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    csrc = os.path.join(_PKG, "csrc")
    args = ["make", "-C", csrc]
    if force:
        args.append("-B")
    subprocess.check_call(args)
    return _LIB


def source_hash():
    """Short hash of every source file liborbx.so is built from.  Counter files under profiles/ carry the hash of the
    sources they were measured on; bench.py refuses (null) counters whose hash differs from the tree it runs in."""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(_PKG, "csrc", "*.hip")) + glob.glob(os.path.join(_PKG, "csrc", "*.hpp")) +
                   glob.glob(os.path.join(_PKG, "csrc", "*.inc")) + glob.glob(os.path.join(_PKG, "csrc", "*.cpp")) +
                   glob.glob(os.path.join(_PKG, "csrc", "Makefile")) + glob.glob(os.path.join(_ROOT, "include", "*")))
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


class Vocabulary:
    """DBoW2 ORB vocabulary on the device (reference inc/ORBVocabulary.h; System.cc:81-82 loads ORBvoc.txt once per process)."""

    def __init__(self, path=None, arrays=None, device=-1):
        self._L = load_library()
        self._v = C.c_void_p()
        if path is not None:
            rc = self._L.orbx_vocabulary_load_text(C.byref(self._v), str(path).encode(), device)
        else:
            a = arrays
            par = np.ascontiguousarray(a["parent"], np.int32); leaf = np.ascontiguousarray(a["is_leaf"], np.uint8)
            d = np.ascontiguousarray(a["desc"], np.uint8); w = np.ascontiguousarray(a["weight"], np.float64)
            rc = self._L.orbx_vocabulary_create(C.byref(self._v), a["k"], a["L"], a["scoring"], a["weighting"], len(par), _ptr(par), _ptr(leaf),
                                                _ptr(d), _ptr(w), device)
        if rc != ORBX_OK:
            raise OrbxError(rc, (self._L.orbx_last_error(None) or b"").decode())

    def info(self):
        k, L, n, w = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._L.orbx_vocabulary_info(self._v, C.byref(k), C.byref(L), C.byref(n), C.byref(w))
        return dict(k=k.value, L=L.value, n_nodes=n.value, n_words=w.value)

    def __del__(self):
        try:
            if getattr(self, "_v", None):
                self._L.orbx_vocabulary_destroy(self._v)
                self._v = None
        except Exception:
            pass


def header_symbols():
    """Names of every function include/orbx.h declares."""
    text = open(_HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(orbx_[a-z0-9_]+)\s*\(", text)))


_lib = None


def load_library():
    """Loads liborbx.so; raises if it has not been built (there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB):
        raise OrbxError(-100, "%s not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "or `make -C extractorb_amd/csrc` (the HIP library is the only compute path)" % _LIB)
    L = C.CDLL(_LIB)
    vp, ip, fp = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)
    L.orbx_abi_version.restype = C.c_int
    L.orbx_create.restype = C.c_int
    L.orbx_create.argtypes = [C.POINTER(vp), C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.orbx_destroy.argtypes = [vp]
    L.orbx_last_error.restype = C.c_char_p
    L.orbx_last_error.argtypes = [vp]
    L.orbx_get_levels.argtypes = [vp]
    L.orbx_get_scale_factor.restype = C.c_float
    L.orbx_get_scale_factor.argtypes = [vp]
    L.orbx_get_tables.argtypes = [vp] + [vp] * 6
    L.orbx_max_keypoints.argtypes = [vp]
    L.orbx_compute_tables.argtypes = [C.c_int, C.c_float, C.c_int] + [vp] * 6
    L.orbx_compute_level_sizes.argtypes = [C.c_float, C.c_int, C.c_int, C.c_int, vp, vp]
    L.orbx_compute_cell_grid.argtypes = [C.c_float, C.c_int, C.c_int, C.c_int, C.c_int] + [ip] * 7
    L.orbx_extract.argtypes = [vp, vp, C.c_int, C.c_int, C.c_ssize_t, C.c_int, C.c_int, vp, vp, C.c_int, ip, ip, vp, vp]
    L.orbx_extract_view.argtypes = [vp, vp, C.c_int, C.c_int, C.c_ssize_t, C.c_int, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp), ip, ip,
                                    C.POINTER(vp), C.POINTER(vp)]
    L.orbx_compute_pyramid.argtypes = [vp, vp, C.c_int, C.c_int, C.c_ssize_t]
    L.orbx_compute_keypoints_octree.argtypes = [vp, vp, C.c_int, vp]
    L.orbx_fetch_pyramid.argtypes = [vp, C.c_int, C.POINTER(vp), vp, vp, vp, vp]
    L.orbx_debug_last_forms.argtypes = [vp, ip, ip, ip]
    L.orbx_debug_last_split_level.argtypes = [vp]
    if hasattr(L, "orbx_debug_lds_pollutions"):      # (an earlier build loaded through ORBX_LIBRARY for an A/B has no such export)
        L.orbx_debug_lds_pollutions.argtypes = [vp]
    L.orbx_debug_set_option.argtypes = [C.c_char_p, C.c_int]
    if hasattr(L, "orbx_debug_describe_tables"):      # (an earlier build loaded through ORBX_LIBRARY for an A/B has no such export)
        L.orbx_debug_describe_tables.argtypes = [vp, vp]
    if hasattr(L, "orbx_debug_describe_levels"):
        L.orbx_debug_describe_levels.argtypes = [C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, ip, vp, vp]
    L.orbx_debug_clock_probe.argtypes = [vp, C.c_int]
    L.orbx_debug_clock_read.argtypes = [vp, C.c_int, vp]
    L.orbx_debug_policy.restype = C.c_char_p
    L.orbx_debug_policy.argtypes = [vp]
    L.orbx_extract_batch.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_ssize_t, C.c_ssize_t, vp, vp, vp, C.c_int,
                                     vp, vp, vp, vp]
    L.orbx_extract_batch_begin.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_ssize_t, C.c_ssize_t, vp, C.c_int]
    L.orbx_extract_batch_end.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp]
    L.orbx_extract_batch_end_view.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), ip, C.POINTER(vp), C.POINTER(vp)]
    L.orbx_host_alloc.restype = vp
    L.orbx_host_alloc.argtypes = [C.c_size_t]
    L.orbx_host_free.argtypes = [vp]
    L.orbx_extract_batch_device.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_ssize_t, C.c_ssize_t, vp, vp, vp,
                                            C.c_int, vp, vp, vp, vp]
    L.orbx_get_level.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, C.c_ssize_t, ip, ip]
    L.orbx_stereo_match_device.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, C.c_float, C.c_float, vp, vp, vp]
    L.orbx_project_last_frame_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp,
                                                 C.c_float, C.c_float, C.c_float, C.c_int, vp]
    L.orbx_search_by_projection_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int,
                                                   vp, vp, vp, vp, vp, C.c_int, C.c_float, C.c_int, C.c_int, vp, vp]
    L.orbx_search_by_projection_two_eyes_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp,
                                                            C.c_int, vp, vp, vp, vp, vp, vp, C.c_float, C.c_int, vp, vp]
    L.orbx_debug_two_eyes_search_stats.argtypes = [ip]
    L.orbx_kb8_project_device.argtypes = [vp, C.c_int, vp, vp, vp]
    L.orbx_project_last_frame_two_eyes_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp,
                                                          C.c_float, C.c_float, C.c_int, vp]
    L.orbx_search_last_frame_two_eyes_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int,
                                                         C.c_int, vp, vp]
    L.orbx_debug_last_frame_two_eyes_stats.argtypes = [ip]
    L.orbx_vocabulary_load_text.argtypes = [C.POINTER(vp), C.c_char_p, C.c_int]
    L.orbx_vocabulary_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int]
    L.orbx_vocabulary_destroy.argtypes = [vp]
    L.orbx_vocabulary_destroy.restype = None
    L.orbx_vocabulary_info.argtypes = [vp, ip, ip, ip, ip]
    L.orbx_compute_bow_device.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    L.orbx_search_by_bow_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_float,
                                            C.c_int, C.c_int, vp, vp]
    L.orbx_search_by_bow_keyframes_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int,
                                                      C.c_float, C.c_int, C.c_int, vp, vp]
    L.orbx_search_by_bow_two_eyes_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_int,
                                                     C.c_float, C.c_int, C.c_int, vp, vp]
    L.orbx_search_for_triangulation_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                       C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    L.orbx_fuse_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int,
                                   vp, vp, vp, vp, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, vp, vp, vp, vp]
    L.orbx_fuse_two_eyes_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp,
                                            vp, C.c_int, vp, vp, vp, C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    L.orbx_search_for_triangulation_two_eyes_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                                vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    L.orbx_kb8_unproject_device.argtypes = [vp, C.c_int, vp, vp, vp]
    L.orbx_kb8_triangulate_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, C.c_float, C.c_float, vp, vp]
    L.orbx_debug_search_triangulation_two_eyes_stats.argtypes = [ip]
    L.orbx_debug_search_triangulation_two_eyes_enable.argtypes = [C.c_int]
    L.orbx_stereo_fisheye_match_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.orbx_debug_stereo_fisheye_stats.argtypes = [ip]
    L.orbx_debug_stereo_fisheye_enable.argtypes = [C.c_int]
    L.orbx_create_new_map_points_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int,
                                                    C.c_int, C.c_float, C.c_float, C.c_int, C.c_float, vp, vp, vp, vp, vp]
    L.orbx_create_new_map_points_two_eyes_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp,
                                                             C.c_int, C.c_int, C.c_int, C.c_float, vp, vp, vp, vp, vp]
    L.orbx_debug_new_map_points_stats.argtypes = [ip]
    L.orbx_reconstruct_two_views_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, C.c_float,
                                                    C.c_int, C.c_float, C.c_int, C.c_float, vp, C.c_int, vp, vp, vp]
    L.orbx_update_map_points_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp,
                                                vp, vp, vp, vp]
    L.orbx_update_map_points_two_eyes_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int,
                                                         C.c_int, vp, vp, vp, vp, vp, vp]
    L.orbx_debug_new_map_points_enable.argtypes = [C.c_int]
    L.orbx_debug_two_view_shape.argtypes = [C.c_int]
    L.orbx_sim3_solve_device.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp, vp, vp, C.c_double, C.c_int, C.c_int, vp, vp, vp]
    L.orbx_debug_sim3_solve_steps.argtypes = [C.c_int]
    L.orbx_optimize_pose_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, vp]
    L.orbx_debug_pose_optimization_launches.argtypes = []
    if hasattr(L, "orbx_detect_candidates_device"):      # (an earlier build loaded through ORBX_LIBRARY for an A/B has no such export)
        L.orbx_detect_candidates_device.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp,
                                                    C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp]
        L.orbx_debug_place_recognition_launches.argtypes = [C.c_int]
    if hasattr(L, "orbx_covisibility_device"):           # (likewise)
        L.orbx_covisibility_device.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int,
                                               C.c_int, vp, vp, vp, vp, vp]
        L.orbx_keyframe_redundancy_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp, vp, C.c_int, vp, C.c_int,
                                                      C.c_int, C.c_float, vp, vp]
        L.orbx_debug_covisibility_launches.argtypes = [C.c_int]
    L.orbx_search_by_projection_sim3_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp,
                                                        vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float, vp,
                                                        vp, vp, vp, vp, vp]
    L.orbx_frustum_requests_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp,
                                               C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_float, vp, vp, vp, vp, vp, vp]
    L.orbx_frustum_requests_two_eyes_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp,
                                                        vp, vp, vp, vp, C.c_int, C.c_float, C.c_float, C.c_int, C.c_float, C.c_int, vp, vp, vp,
                                                        vp, vp, vp, vp]
    L.orbx_sim3_hamming_bound.argtypes = [C.c_int, C.c_float]
    L.orbx_debug_sim3_search_stats.argtypes = [ip]
    L.orbx_debug_sim3_search_list_length.argtypes = []
    L.orbx_predict_scale.argtypes = [C.c_float, C.c_float, C.c_float, C.c_int]
    L.orbx_predict_scale_breakpoints.argtypes = [C.c_float, C.c_int, vp]
    L.orbx_stereo_match_last.argtypes = [vp, C.c_int, C.c_float, C.c_float, vp, vp, C.c_int, vp]
    L.orbx_compute_image_bounds.argtypes = [vp, C.c_int, C.c_int, vp]
    L.orbx_frame_finish_device.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.orbx_frame_finish_two_eyes_device.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.orbx_search_for_initialization_device.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, vp,
                                                        vp, vp, C.c_int, C.c_float, C.c_int, vp, vp]
    L.orbx_stereo_from_rgbd_device.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_ssize_t, C.c_ssize_t,
                                               C.c_float, C.c_float, vp, vp]
    L.orbx_gray_from_color_device.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_ssize_t, C.c_ssize_t, vp,
                                              C.c_ssize_t, C.c_ssize_t]
    L.orbx_set_stream.argtypes = [vp, vp]
    L.orbx_get_stream.restype = vp
    L.orbx_get_stream.argtypes = [vp]
    L.orbx_synchronize.argtypes = [vp]
    L.orbx_debug_num_candidates.argtypes = [vp, C.c_int, C.c_int, ip]
    L.orbx_debug_get_candidates.argtypes = [vp, C.c_int, C.c_int, vp, C.c_int]
    L.orbx_debug_get_blurred.argtypes = [vp, C.c_int, C.c_int, vp, C.c_ssize_t]
    L.orbx_profile_enable.argtypes = [vp, C.c_int]
    L.orbx_profile_reset.argtypes = [vp]
    L.orbx_profile_read.argtypes = [vp, vp, vp]
    L.orbx_profile_kernel_name.restype = C.c_char_p
    L.orbx_profile_kernel_name.argtypes = [C.c_int]
    L.orbx_profile_kernel_name_of.restype = C.c_char_p
    L.orbx_profile_kernel_name_of.argtypes = [vp, C.c_int]
    L.orbx_algorithmic_bytes.restype = C.c_long
    L.orbx_algorithmic_bytes.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    _lib = L
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dev(x):
    """a device pointer argument: None (NULL: optional, or refused by the C entry with ORBX_ERR_BAD_ARGUMENT), an int, or an object with .data_ptr()"""
    return C.c_void_p(0 if x is None else (x.data_ptr() if hasattr(x, "data_ptr") else int(x)))


def _host_f32(a):
    """a small host array the C entry reads during the call (camera, bounds, a 3x4 transform): None stays NULL"""
    return None if a is None else _ptr(np.ascontiguousarray(a, np.float32))


def _split_levels(lvl, counts):
    """the per-level keypoint arrays out of the level-major array and its counts"""
    per_level, o = [], 0
    for c in counts.tolist():
        per_level.append(lvl[o:o + c].copy()); o += c
    return per_level


def _lapping(lapping, n):
    """vLappingArea per frame as int32 [n, 2] (one pair is given to every frame), or None"""
    if lapping is None:
        return None
    return np.ascontiguousarray(np.broadcast_to(np.asarray(lapping, np.int32).reshape(-1, 2), (n, 2)))


# ---- test aids (include/orbx.h: orbx_debug_set_option).  Not reachable from the environment; handles created AFTERWARDS carry the setting ----
TEST_AIDS = ("poison", "lds_pollute", "fail_after_fast")


def debug_set_option(name, value):
    rc = load_library().orbx_debug_set_option(name.encode(), int(value))
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbx_debug_set_option(%r)" % name)


def debug_reset_options():
    debug_set_option("poison", -1)
    debug_set_option("lds_pollute", -1)
    debug_set_option("fail_after_fast", 0)
    debug_set_option("pyr_cols_shape", -1)
    debug_set_option("shared_upload_bytes", -1)
    debug_set_option("two_eyes_walk", 0)
    debug_set_option("two_eyes_bow_stage", -1)
    load_library().orbx_debug_set_option(b"describe_sums", -1)      # (an earlier build loaded through ORBX_LIBRARY for an A/B has no such aid)


# ---- handle-free host helpers (no GPU needed) -------------------------------------------------------------
def describe_tables():
    """IC_Angle's static weight words (include/orbx.h: orbx_debug_describe_tables): uint32 [2, 16, 12] (patch-blur form) and [2, 16, 8]"""
    pb = np.zeros((2, 16, 12), np.uint32); plain = np.zeros((2, 16, 8), np.uint32)
    rc = load_library().orbx_debug_describe_tables(_ptr(pb), _ptr(plain))
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbx_debug_describe_tables")
    return pb, plain


DESCRIBE_LEVEL_FIELDS = ("selOff", "w", "h", "pyrStride", "blurStride", "pyrOff", "pyrFrameBytes", "blurOff", "blurFrameBytes", "scale_bits", "patchSize")


def describe_levels(rows, cols, nfeatures=1000, scale_factor=1.2, nlevels=8, max_batch=1):
    """(nlevels, desc, geom): the level table the description kernels take by value and the per-level geometry it is filled from, both int64
    [11, 16] with the rows of DESCRIBE_LEVEL_FIELDS (include/orbx.h: orbx_debug_describe_levels)"""
    desc = np.zeros((11, 16), np.int64); geom = np.zeros((11, 16), np.int64)
    n = C.c_int()
    rc = load_library().orbx_debug_describe_levels(nfeatures, scale_factor, nlevels, rows, cols, max_batch, C.byref(n), _ptr(desc), _ptr(geom))
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbx_debug_describe_levels")
    return n.value, desc, geom


def compute_tables(nfeatures=1000, scale_factor=1.2, nlevels=8):
    L = load_library()
    sf = np.zeros(nlevels, np.float32); isf = sf.copy(); s2 = sf.copy(); is2 = sf.copy()
    q = np.zeros(nlevels, np.int32); um = np.zeros(16, np.int32)
    rc = L.orbx_compute_tables(nfeatures, scale_factor, nlevels, _ptr(sf), _ptr(isf), _ptr(s2), _ptr(is2), _ptr(q), _ptr(um))
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbx_compute_tables")
    return dict(scale_factors=sf, inv_scale_factors=isf, level_sigma2=s2, inv_level_sigma2=is2,
                features_per_level=q, umax=um)


def compute_level_sizes(rows, cols, scale_factor=1.2, nlevels=8):
    L = load_library()
    w = np.zeros(nlevels, np.int32); h = np.zeros(nlevels, np.int32)
    rc = L.orbx_compute_level_sizes(scale_factor, nlevels, rows, cols, _ptr(w), _ptr(h))
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbx_compute_level_sizes")
    return list(zip(w.tolist(), h.tolist()))


def compute_cell_grid(rows, cols, level, scale_factor=1.2, nlevels=8):
    L = load_library()
    v = [C.c_int() for _ in range(7)]
    rc = L.orbx_compute_cell_grid(scale_factor, nlevels, rows, cols, level, *[C.byref(x) for x in v])
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbx_compute_cell_grid")
    keys = ["n_cols", "n_rows", "w_cell", "h_cell", "n_cells", "n_ini", "cand_cap"]
    return dict(zip(keys, [x.value for x in v]))


def pinned_empty(shape, dtype=np.uint8):
    """numpy array backed by pinned host memory (orbx_host_alloc): H2D copies from it overlap with kernels."""
    L = load_library()
    dtype = np.dtype(dtype)
    nbytes = int(np.prod(shape)) * dtype.itemsize
    p = L.orbx_host_alloc(nbytes)
    if not p:
        raise OrbxError(-6, "orbx_host_alloc failed")
    buf = (C.c_uint8 * nbytes).from_address(p)
    return np.frombuffer(buf, dtype=dtype).reshape(shape)   # free with pinned_free(arr); it must not be used afterwards


def pinned_free(arr):
    load_library().orbx_host_free(C.c_void_p(arr.ctypes.data))


def predict_scale(max_distance, dist, scale_factor=1.2, nlevels=8):
    """MapPoint::PredictScale (reference src/MapPoint.cc:514-529) through the host libm.  Host only."""
    rc = load_library().orbx_predict_scale(max_distance, dist, scale_factor, nlevels)
    if rc < 0:
        raise OrbxError(rc, "orbx_predict_scale")
    return rc


def predict_scale_breakpoints(scale_factor=1.2, nlevels=8):
    """The nlevels - 1 ratios at which MapPoint::PredictScale steps: the level of a ratio is the number of breakpoints <= ratio.  Host only."""
    b = np.zeros(max(nlevels - 1, 0), np.float32)
    rc = load_library().orbx_predict_scale_breakpoints(scale_factor, nlevels, _ptr(b))
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbx_predict_scale_breakpoints")
    return b


def sim3_hamming_bound(th_low=50, ratio_hamming=1.0):
    """The largest descriptor distance the Sim3 projection search accepts: the largest d in [0, 255] with (float)d <= (float)th_low *
    ratio_hamming, -1 if that product is negative or NaN.  Host only."""
    return load_library().orbx_sim3_hamming_bound(int(th_low), C.c_float(ratio_hamming))


def camera(fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0):
    """orbx_camera: Frame::mK and Frame::mDistCoef as nine floats."""
    return np.array([fx, fy, cx, cy, k1, k2, p1, p2, k3], np.float32)


def camera_kb8(fx, fy, cx, cy, k1=0.0, k2=0.0, k3=0.0, k4=0.0):
    """orbx_camera_kb8: KannalaBrandt8::mvParameters as eight floats."""
    return np.array([fx, fy, cx, cy, k1, k2, k3, k4], np.float32)


def compute_image_bounds(cam, cols, rows):
    """Frame::ComputeImageBounds (reference src/Frame.cc:784-811): (mnMinX, mnMaxX, mnMinY, mnMaxY).  Host only."""
    L = load_library()
    b = np.zeros(4, np.float32)
    rc = L.orbx_compute_image_bounds(_host_f32(cam), cols, rows, _ptr(b))
    if rc != ORBX_OK:
        raise OrbxError(rc, "orbx_compute_image_bounds")
    return b


class ORBextractor:
    """Mirror of ``ORB_SLAM3::ORBextractor`` (reference inc/ORBextractor.h:44-111) on one MI355X.

    ``ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)`` as in the reference; the
    extra keyword arguments size the device arenas once (the reference reallocates per call).
    ``extractor(image, mask=None, lapping=(0, 1000))`` mirrors ``operator()``: it returns
    ``(mono_index, keypoints, descriptors, all_levels_keypoints)`` where the reference fills its output
    arguments; ``mono_index`` is the reference's return value (-1 for an empty image).
    """

    def __init__(self, nfeatures=1000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7, *,
                 max_width=640, max_height=480, max_batch=1, device=-1):
        self._L = load_library()
        self._h = C.c_void_p()
        rc = self._L.orbx_create(C.byref(self._h), nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST,
                                 max_width, max_height, max_batch, device)
        if rc != ORBX_OK:
            self._h = None
            raise OrbxError(rc, (self._L.orbx_last_error(None) or b"").decode())
        self.nfeatures, self.nlevels = nfeatures, nlevels
        self.scaleFactor, self.iniThFAST, self.minThFAST = scaleFactor, iniThFAST, minThFAST
        self.max_width, self.max_height, self.max_batch = max_width, max_height, max_batch
        self.capacity = self._L.orbx_max_keypoints(self._h)
        t = compute_tables(nfeatures, scaleFactor, nlevels)
        self.mvScaleFactor, self.mvInvScaleFactor = t["scale_factors"], t["inv_scale_factors"]
        self.mvLevelSigma2, self.mvInvLevelSigma2 = t["level_sigma2"], t["inv_level_sigma2"]
        self.mnFeaturesPerLevel, self.umax = t["features_per_level"], t["umax"]

    # ---- reference getters (inc/ORBextractor.h:63-83) ----
    def GetLevels(self): return self.nlevels
    def GetScaleFactor(self): return self._L.orbx_get_scale_factor(self._h)
    def GetScaleFactors(self): return self.mvScaleFactor.copy()
    def GetInverseScaleFactors(self): return self.mvInvScaleFactor.copy()
    def GetScaleSigmaSquares(self): return self.mvLevelSigma2.copy()
    def GetInverseScaleSigmaSquares(self): return self.mvInvLevelSigma2.copy()

    def close(self):
        if getattr(self, "_h", None):
            self._L.orbx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != ORBX_OK:
            raise OrbxError(rc, (self._L.orbx_last_error(self._h) or b"").decode())

    # ---- operator() ----
    def __call__(self, image, mask=None, lapping=(0, 1000)):
        image = np.asarray(image)
        if image.size == 0:
            return -1, np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8), [np.zeros(0, KEYPOINT_DTYPE)] * self.nlevels
        if image.dtype != np.uint8 or image.ndim != 2 or image.strides[1] != 1:
            raise ValueError("image must be a 2-D uint8 array with contiguous rows (CV_8UC1)")   # assert at ORBextractor.cc:1087
        cap = self.capacity
        kps = np.zeros(cap, KEYPOINT_DTYPE); desc = np.zeros((cap, 32), np.uint8)
        lvl = np.zeros(cap, KEYPOINT_DTYPE); counts = np.zeros(self.nlevels, np.int32)
        n, mono = C.c_int(), C.c_int()
        self._check(self._L.orbx_extract(self._h, _ptr(image), image.shape[0], image.shape[1], image.strides[0],
                                         int(lapping[0]), int(lapping[1]), _ptr(kps), _ptr(desc), cap,
                                         C.byref(n), C.byref(mono), _ptr(lvl), _ptr(counts)))
        return mono.value, kps[:n.value].copy(), desc[:n.value].copy(), _split_levels(lvl, counts)

    def extract_batch(self, images, lapping=None):
        """images: uint8 [B, rows, cols].  Returns a list of (mono_index, keypoints, descriptors, per_level)."""
        images = np.ascontiguousarray(images, np.uint8)
        B, rows, cols = images.shape
        cap = self.capacity
        kps = np.zeros((B, cap), KEYPOINT_DTYPE); desc = np.zeros((B, cap, 32), np.uint8)
        lvl = np.zeros((B, cap), KEYPOINT_DTYPE); counts = np.zeros((B, self.nlevels), np.int32)
        n = np.zeros(B, np.int32); mono = np.zeros(B, np.int32)
        lap = _lapping(lapping, B)
        self._check(self._L.orbx_extract_batch(self._h, B, _ptr(images), rows, cols, cols, rows * cols, _ptr(lap),
                                               _ptr(kps), _ptr(desc), cap, _ptr(n), _ptr(mono), _ptr(lvl), _ptr(counts)))
        return [(int(mono[f]), kps[f, :n[f]].copy(), desc[f, :n[f]].copy(), _split_levels(lvl[f], counts[f])) for f in range(B)]

    def extract_batch_begin(self, images, lapping=None, want_levels=False):
        """Asynchronous host-buffer form: enqueue H2D + path + D2H and return (one batch in flight per handle)."""
        # rows may be padded (a view into a wider buffer, as a cv::Mat ROI): stride / frame_stride are passed as they are
        assert images.dtype == np.uint8 and images.ndim == 3 and images.strides[2] == 1 and images.strides[1] >= images.shape[2] and images.strides[0] > 0
        B, rows, cols = images.shape
        lap = _lapping(lapping, B)
        self._check(self._L.orbx_extract_batch_begin(self._h, B, _ptr(images), rows, cols, images.strides[1], images.strides[0], _ptr(lap), int(want_levels)))
        self._pending = (B, images, lap)     # keep the buffers alive until the batch ends

    def extract_batch_end(self):
        if getattr(self, "_pending", None) is None:
            raise OrbxError(-2, "no batch in flight: call extract_batch_begin first")
        B = self._pending[0]
        cap = self.capacity
        kps = np.zeros((B, cap), KEYPOINT_DTYPE); desc = np.zeros((B, cap, 32), np.uint8)
        n = np.zeros(B, np.int32); mono = np.zeros(B, np.int32)
        self._check(self._L.orbx_extract_batch_end(self._h, _ptr(kps), _ptr(desc), cap, _ptr(n), _ptr(mono), None, None))
        self._pending = None
        return [(int(mono[f]), kps[f, :n[f]].copy(), desc[f, :n[f]].copy()) for f in range(B)]

    def extract_batch_end_view(self):
        """Zero-copy form of extract_batch_end: waits, then returns numpy views (keypoints[B, cap], descriptors[B, cap, 32], n[B],
        mono[B]) into the handle's pinned staging, valid until the next extract_batch_begin on this extractor."""
        if getattr(self, "_pending", None) is None:
            raise OrbxError(-2, "no batch in flight: call extract_batch_begin first")
        B = self._pending[0]
        vk, vd, vn, vm, vc = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int()
        self._check(self._L.orbx_extract_batch_end_view(self._h, C.byref(vk), C.byref(vd), C.byref(vc), C.byref(vn), C.byref(vm)))
        self._pending = None
        cap = vc.value
        as_np = lambda ptr, nbytes: np.frombuffer((C.c_uint8 * nbytes).from_address(ptr.value), np.uint8)
        kps = as_np(vk, B * cap * 28).view(KEYPOINT_DTYPE).reshape(B, cap)
        desc = as_np(vd, B * cap * 32).reshape(B, cap, 32)
        return kps, desc, as_np(vn, 4 * B).view(np.int32), as_np(vm, 4 * B).view(np.int32)

    def extract_batch_device(self, d_images, n_frames, rows, cols, d_kps, d_desc, d_n, d_mono, capacity,
                             stride=None, frame_stride=None, lapping=None, d_level_kps=0, d_level_counts=0):
        """Device-pointer form (ints or objects with .data_ptr()); asynchronous on the handle's stream."""
        stride = cols if stride is None else stride
        frame_stride = rows * stride if frame_stride is None else frame_stride
        lap = _lapping(lapping, n_frames)
        self._check(self._L.orbx_extract_batch_device(self._h, n_frames, _dev(d_images), rows, cols, stride, frame_stride,
                                                      _ptr(lap), _dev(d_kps), _dev(d_desc), capacity, _dev(d_n), _dev(d_mono),
                                                      _dev(d_level_kps), _dev(d_level_counts)))

    # ---- Frame::ComputeStereoMatches (reference src/Frame.cc:813-991) on the last batch ----
    def stereo_match_last(self, n_pairs, bf, b):
        """Frames 2p / 2p+1 of the last extract_batch call are the left / right eye of pair p.
        Returns a list of (uRight[nL], depth[nL], n_matched) per pair."""
        cap = self.capacity
        u = np.zeros((n_pairs, cap), np.float32); d = np.zeros((n_pairs, cap), np.float32)
        nm = np.zeros(n_pairs, np.int32)
        self._check(self._L.orbx_stereo_match_last(self._h, n_pairs, bf, b, _ptr(u), _ptr(d), cap, _ptr(nm)))
        return u, d, nm

    def stereo_match_device(self, n_pairs, d_kps, d_desc, d_n, capacity, bf, b, d_u_right, d_depth, d_n_matched):
        self._check(self._L.orbx_stereo_match_device(self._h, n_pairs, _dev(d_kps), _dev(d_desc), _dev(d_n), capacity, bf, b,
                                                     _dev(d_u_right), _dev(d_depth), _dev(d_n_matched)))

    def frame_finish_device(self, n_frames, d_kps, d_n, capacity, cam, bounds, d_kps_un, d_grid_off, d_grid_idx, d_n_inside):
        """UndistortKeyPoints + AssignFeaturesToGrid (reference src/Frame.cc:748-782, 383-417) on device buffers."""
        self._check(self._L.orbx_frame_finish_device(self._h, n_frames, _dev(d_kps), _dev(d_n), capacity, _host_f32(cam), _host_f32(bounds),
                                                     _dev(d_kps_un), _dev(d_grid_off), _dev(d_grid_idx), _dev(d_n_inside)))

    def frame_finish_two_eyes_device(self, n_pairs, d_kps, d_n, capacity, cam, bounds, d_kps_un, d_grid_off, d_grid_idx, d_n_inside):
        """AssignFeaturesToGrid's Nleft != -1 branch (reference src/Frame.cc:404-414: mGrid / mGridRight from the RAW keys of frames 2p / 2p + 1)
        + UndistortKeyPoints, on device buffers of 2 * n_pairs frames."""
        self._check(self._L.orbx_frame_finish_two_eyes_device(self._h, n_pairs, _dev(d_kps), _dev(d_n), capacity, _host_f32(cam), _host_f32(bounds),
                                                              _dev(d_kps_un), _dev(d_grid_off), _dev(d_grid_idx), _dev(d_n_inside)))

    def search_for_initialization_device(self, n_pairs, frames1, frames2, d_kps_un, d_desc, d_n, capacity, d_grid_off, d_grid_idx,
                                         bounds, d_prev_matched, d_matches12, d_n_matches, window=100, nnratio=0.9,
                                         check_orientation=True):
        """ORBmatcher::SearchForInitialization (reference src/ORBmatcher.cc:706-821) for n_pairs pairs of device-resident
        frames; frames1 / frames2 = (first, step) of the F1 / F2 frame index of pair p."""
        self._check(self._L.orbx_search_for_initialization_device(
            self._h, n_pairs, frames1[0], frames1[1], frames2[0], frames2[1], _dev(d_kps_un), _dev(d_desc), _dev(d_n), capacity,
            _dev(d_grid_off), _dev(d_grid_idx), _host_f32(bounds), _dev(d_prev_matched), window, nnratio, int(check_orientation),
            _dev(d_matches12), _dev(d_n_matches)))

    def reconstruct_two_views_device(self, n_pairs, frames1, frames2, d_kps_un, d_n, capacity, d_matches12, d_n_matches, cam, d_rand,
                                     d_result, d_p3d, d_triangulated, sigma=1.0, iterations=200, min_parallax=1.0, min_triangulated=50,
                                     rh_threshold=0.5, prune=False):
        """TwoViewReconstruction::Reconstruct (reference src/TwoViewReconstruction.cc:39-125) on the tables search_for_initialization_device
        wrote; frames1 / frames2 = (first, step).  d_rand [(p*iterations + it)*8 + j] holds the caller's raw rand() values (int32); d_result
        one TWO_VIEW_RESULT_DTYPE row per pair; d_p3d [(p*capacity + i)*3] and d_triangulated [p*capacity + i] are vP3D and vbTriangulated.
        prune: the tracker's next statement (src/Tracking.cc:2083-2090) on d_matches12 / d_n_matches of an accepted pair."""
        self._check(self._L.orbx_reconstruct_two_views_device(
            self._h, n_pairs, frames1[0], frames1[1], frames2[0], frames2[1], _dev(d_kps_un), _dev(d_n), capacity, _dev(d_matches12),
            _dev(d_n_matches), _host_f32(cam), sigma, iterations, min_parallax, min_triangulated, rh_threshold, _dev(d_rand), int(prune),
            _dev(d_result), _dev(d_p3d), _dev(d_triangulated)))

    def sim3_solve_device(self, n_problems, d_problems, capacity, d_x1w, d_x2w, d_octave1, d_octave2, d_rand, d_result, d_inliers,
                          probability=0.99, min_inliers=15, max_iterations=300):
        """Sim3Solver's constructor, SetRansacParameters and the iterate(20, ..) loop (reference src/Sim3Solver.cc, call site
        src/LoopClosing.cc:673-684) for n_problems problems.  d_problems: SIM3_PROBLEM_DTYPE rows; d_x1w / d_x2w [(p*capacity + i)*3] the world
        positions of pMP1 / pMP2 of slot i1 = i, d_octave1 / d_octave2 [p*capacity + i] the octaves of kp1 / kp2 (-1: the slot is absent);
        d_rand [(p*max_iterations + it)*3 + j] the caller's raw rand() values (int32); d_result one SIM3_RESULT_DTYPE row per problem;
        d_inliers [p*capacity + i] = vbInliers, all zero unless CONVERGED."""
        self._check(self._L.orbx_sim3_solve_device(self._h, n_problems, _dev(d_problems), capacity, _dev(d_x1w), _dev(d_x2w), _dev(d_octave1),
                                                   _dev(d_octave2), probability, min_inliers, max_iterations, _dev(d_rand), _dev(d_result),
                                                   _dev(d_inliers)))

    def optimize_pose_device(self, n_problems, frames, d_problems, d_kps, d_n, d_u_right, capacity, d_matches, d_mp_world, n_map_points, d_poses,
                             d_outlier, d_result, eyes=1):
        """Optimizer::PoseOptimization (reference src/Optimizer.cc:854-1168) for n_problems frames; frames = (first, step).  d_problems:
        POSE_PROBLEM_DTYPE rows; d_kps / d_n / d_u_right (None: no stereo edge) of all frames; d_matches [row*capacity + i] indices into
        d_mp_world [m*3], -1 = no MapPoint; d_poses [f*12] in/out; d_outlier [row*capacity + i] in/out (mvbOutlier); d_result one
        POSE_RESULT_DTYPE row per problem.  eyes=2: frames are rigs (device frames 2f, 2f + 1; rows 2p, 2p + 1; one pose per rig)."""
        self._check(self._L.orbx_optimize_pose_device(self._h, n_problems, frames[0], frames[1], eyes, _dev(d_problems), _dev(d_kps), _dev(d_n),
                                                      _dev(d_u_right), capacity, _dev(d_matches), _dev(d_mp_world), n_map_points, _dev(d_poses),
                                                      _dev(d_outlier), _dev(d_result)))

    def debug_pose_optimization_launches(self):
        """launches of the pose optimiser's kernel so far in this process (it has one launch form)"""
        return self._L.orbx_debug_pose_optimization_launches()

    def detect_candidates_device(self, vocab, mode, n_db, d_db_word_ids, d_db_word_weights, d_db_n_words, capacity, d_db_map_id, d_db_flags,
                                 d_db_covis, n_queries, queries, d_q_word_ids, d_q_word_weights, d_q_n_words, q_capacity, d_q_map_id, d_score,
                                 d_result, d_connected=None, n_candidates=3, d_loop=None, d_merge=None, d_cand=None, cand_capacity=0,
                                 d_common_words=None):
        """KeyFrameDatabase::DetectNBestCandidates (mode PLACE_N_BEST) / DetectRelocalizationCandidates (PLACE_RELOCALIZATION) (reference
        src/KeyFrameDatabase.cc:612-780, :783-895) for n_queries queries against n_db database rows in KeyFrameDatabase::add order; queries
        = (first, step) into the query arrays.  The three BoW arrays are compute_bow_device's layout.  d_db_flags: bit 0 isBad(), bit 1
        GetMap()->IsBad(); d_db_covis [k*10 + j] database rows or -1; d_connected [q*n_db + k] (N_BEST, None = none); d_score [q*n_db + k]
        in/out (mPlaceRecognitionScore / mRelocScore: state); d_result one PLACE_RESULT_DTYPE row per query; d_loop / d_merge
        [q*n_candidates + i] (N_BEST), d_cand [q*cand_capacity + i] (RELOCALIZATION); d_common_words [q*n_db + k] optional."""
        self._check(self._L.orbx_detect_candidates_device(
            self._h, vocab._v, int(mode), n_db, _dev(d_db_word_ids), _dev(d_db_word_weights), _dev(d_db_n_words), capacity, _dev(d_db_map_id),
            _dev(d_db_flags), _dev(d_db_covis), n_queries, queries[0], queries[1], _dev(d_q_word_ids), _dev(d_q_word_weights), _dev(d_q_n_words),
            q_capacity, _dev(d_q_map_id), _dev(d_connected), n_candidates, _dev(d_score), _dev(d_result), _dev(d_loop), _dev(d_merge), _dev(d_cand),
            cand_capacity, _dev(d_common_words)))

    def debug_place_recognition_launches(self, which):
        """launches so far in this process of k_place_pairs (which = 0) / k_place_query (which = 1): the entry has one launch form"""
        return self._L.orbx_debug_place_recognition_launches(which)

    def covisibility_device(self, mode, n_points, d_obs_off, d_obs, d_mp_flags, n_frames, d_kf_flags, d_kf_key, n_subjects, d_subject_mp,
                            d_subject_n, capacity, conn_capacity, d_counter_kf, d_counter_w, d_result, d_kf_map_id=None, d_subject_kf=None,
                            d_subject_map_id=None, th=15, d_ordered_kf=None, d_ordered_w=None):
        """KeyFrame::UpdateConnections (mode COVIS_UPDATE_CONNECTIONS; reference src/KeyFrame.cc:388-511) / the vote of
        Tracking::UpdateLocalKeyFrames (COVIS_LOCAL_KEYFRAMES; src/Tracking.cc:3030-3102) for n_subjects rows of MapPoints.  d_obs_off / d_obs:
        update_map_points_device's CSR; d_mp_flags / d_kf_flags: bit 0 isBad(); d_kf_key [f] uint64, the KeyFrame* order; d_subject_mp
        [s*capacity + i] MapPoint indices or -1, d_subject_n [s]; d_subject_kf / d_subject_map_id / d_kf_map_id (UPDATE_CONNECTIONS); d_counter_*
        [s*conn_capacity + j] the counter in key order, d_ordered_* the ordered list (UPDATE_CONNECTIONS); d_result one COVIS_RESULT_DTYPE row
        per subject."""
        self._check(self._L.orbx_covisibility_device(
            self._h, int(mode), n_points, _dev(d_obs_off), _dev(d_obs), _dev(d_mp_flags), n_frames, _dev(d_kf_flags), _dev(d_kf_map_id), _dev(d_kf_key),
            n_subjects, _dev(d_subject_mp), _dev(d_subject_n), capacity, _dev(d_subject_kf), _dev(d_subject_map_id), th, conn_capacity,
            _dev(d_counter_kf), _dev(d_counter_w), _dev(d_ordered_kf), _dev(d_ordered_w), _dev(d_result)))

    def keyframe_redundancy_device(self, n_points, d_obs_off, d_obs, d_mp_flags, n_frames, d_kf_flags, d_kps_un, d_n_out, n_subjects, d_subject_mp,
                                   d_subject_n, capacity, d_subject_kf, d_result, monocular=True, d_depth=None, d_th_depth=None, d_mp_nobs=None,
                                   th_obs=3, redundant_th=0.9, d_slot_state=None):
        """The test inside LocalMapping::KeyFrameCulling's loop (reference src/LocalMapping.cc:977-1043) for n_subjects keyframes (device frames
        d_subject_kf[s]) on covisibility_device's tables; d_kf_flags bit 1 = the map's initial keyframe; d_mp_nobs [m] MapPoint::Observations()
        (None = the list length); d_depth / d_th_depth when not monocular; d_result one REDUNDANCY_RESULT_DTYPE row per subject; d_slot_state
        [s*capacity + i] optional: 0 not counted, 1 counted, 2 redundant."""
        self._check(self._L.orbx_keyframe_redundancy_device(
            self._h, n_points, _dev(d_obs_off), _dev(d_obs), _dev(d_mp_flags), _dev(d_mp_nobs), n_frames, _dev(d_kf_flags), _dev(d_kps_un), _dev(d_n_out),
            _dev(d_depth), _dev(d_th_depth), n_subjects, _dev(d_subject_mp), _dev(d_subject_n), capacity, _dev(d_subject_kf), 1 if monocular else 0,
            th_obs, float(redundant_th), _dev(d_result), _dev(d_slot_state)))

    def debug_covisibility_launches(self, which):
        """launches so far in this process of k_covis_rank (0) / k_covis_vote (1) / k_keyframe_redundancy (2)"""
        return self._L.orbx_debug_covisibility_launches(which)

    def project_last_frame_device(self, n_pairs, last, cur, d_kps, d_kps_un, d_n, capacity, d_mp_flags, d_world, d_poses, cam, bounds,
                                  mbf, mb, th, mono, d_queries):
        """Front half of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (reference src/ORBmatcher.cc:1961-2023);
        last / cur = (first, step) of the last / current frame index of pair p."""
        self._check(self._L.orbx_project_last_frame_device(self._h, n_pairs, last[0], last[1], cur[0], cur[1], _dev(d_kps), _dev(d_kps_un), _dev(d_n),
                                                           capacity, _dev(d_mp_flags), _dev(d_world), _dev(d_poses), _host_f32(cam), _host_f32(bounds),
                                                           mbf, mb, th, int(mono), _dev(d_queries)))

    def search_by_projection_device(self, n_pairs, cur, d_queries, d_query_desc, desc_blocks, d_n_queries, query_capacity, d_kps_un, d_desc,
                                    d_n, capacity, d_grid_off, d_grid_idx, bounds, d_u_right, d_occupied, ratio_mode, nnratio,
                                    check_orientation, d_matches, d_n_matches, max_distance=100):
        """ORBmatcher::SearchByProjection, the search (reference src/ORBmatcher.cc:2025-2175 / :44-135); cur and desc_blocks = (first, step)."""
        self._check(self._L.orbx_search_by_projection_device(
            self._h, n_pairs, cur[0], cur[1], _dev(d_queries), _dev(d_query_desc), desc_blocks[0], desc_blocks[1], _dev(d_n_queries), query_capacity,
            _dev(d_kps_un), _dev(d_desc), _dev(d_n), capacity, _dev(d_grid_off), _dev(d_grid_idx), _host_f32(bounds), _dev(d_u_right), _dev(d_occupied),
            int(ratio_mode), nnratio, max_distance, int(check_orientation), _dev(d_matches), _dev(d_n_matches)))

    def search_by_projection_two_eyes_device(self, n_pairs, pairs, d_queries, d_query_desc, desc_blocks, d_n_queries, query_capacity, d_kps,
                                             d_desc, d_n, capacity, d_grid_off, d_grid_idx, bounds, d_left_to_right, d_right_to_left,
                                             d_occupied, nnratio, d_matches, d_n_matches, max_distance=100):
        """ORBmatcher::SearchByProjection(F, vpMapPoints, th, ...) for two-camera frames (reference src/ORBmatcher.cc:44-213, F.Nleft != -1);
        pairs = (first, step): pair q's left eye is frame 2*(first + q*step), its right eye the next frame; desc_blocks = (first, step).
        d_queries holds two requests per MapPoint (left, right); d_matches / d_occupied are [(2q + eye)*capacity + i]."""
        self._check(self._L.orbx_search_by_projection_two_eyes_device(
            self._h, n_pairs, pairs[0], pairs[1], _dev(d_queries), _dev(d_query_desc), desc_blocks[0], desc_blocks[1], _dev(d_n_queries), query_capacity,
            _dev(d_kps), _dev(d_desc), _dev(d_n), capacity, _dev(d_grid_off), _dev(d_grid_idx), _host_f32(bounds), _dev(d_left_to_right), _dev(d_right_to_left),
            _dev(d_occupied), nnratio, max_distance, _dev(d_matches), _dev(d_n_matches)))

    def kb8_project_device(self, n, d_xyz, cam, d_uv):
        """KannalaBrandt8::project (reference src/CameraModels/KannalaBrandt8.cpp:28-44) over n device-resident points; cam = camera_kb8(...)."""
        self._check(self._L.orbx_kb8_project_device(self._h, n, _dev(d_xyz), _host_f32(cam), _dev(d_uv)))

    def project_last_frame_two_eyes_device(self, n_pairs, last, cur, d_kps, d_n, capacity, d_mp_flags, d_world, d_poses, trl, cam, bounds, mb, th,
                                           mono, d_queries):
        """Front half of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) for two-camera frames (reference
        src/ORBmatcher.cc:1971-2023, :2084-2101); last / cur = (first, step) of the last / current RIG frame of pair p (device frames 2r, 2r + 1);
        d_poses per rig frame; trl = mTrl (3x4); cam = camera_kb8(...).  d_queries: 2 * capacity requests per pair, two records (L, R) each."""
        self._check(self._L.orbx_project_last_frame_two_eyes_device(self._h, n_pairs, last[0], last[1], cur[0], cur[1], _dev(d_kps), _dev(d_n), capacity,
                                                                    _dev(d_mp_flags), _dev(d_world), _dev(d_poses), _host_f32(trl), _host_f32(cam), _host_f32(bounds), mb, th,
                                                                    int(mono), _dev(d_queries)))

    def search_last_frame_two_eyes_device(self, n_pairs, cur, d_queries, d_query_desc, d_kps, d_desc, d_n, capacity, d_grid_off, d_grid_idx, bounds,
                                          d_occupied, check_orientation, d_matches, d_n_matches, max_distance=100):
        """ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) for two-camera frames, the search (reference
        src/ORBmatcher.cc:2013-2174); cur = (first, step) of the current RIG frame of pair q.  d_queries / d_query_desc: 2 * capacity requests
        per pair; d_matches / d_occupied are [(2q + eye)*capacity + i]."""
        self._check(self._L.orbx_search_last_frame_two_eyes_device(
            self._h, n_pairs, cur[0], cur[1], _dev(d_queries), _dev(d_query_desc), _dev(d_kps), _dev(d_desc), _dev(d_n), capacity, _dev(d_grid_off),
            _dev(d_grid_idx), _host_f32(bounds), _dev(d_occupied), max_distance, int(check_orientation), _dev(d_matches), _dev(d_n_matches)))

    def compute_bow_device(self, vocab, n_frames, d_desc, d_n, capacity, d_word_ids, d_word_weights, d_n_words, d_feat_nodes, d_feat_idx,
                           d_n_feat, levels_up=4):
        """Frame::ComputeBoW (reference src/Frame.cc:739-746) for n_frames device-resident frames."""
        self._check(self._L.orbx_compute_bow_device(self._h, vocab._v, n_frames, _dev(d_desc), _dev(d_n), capacity, levels_up, _dev(d_word_ids),
                                                    _dev(d_word_weights), _dev(d_n_words), _dev(d_feat_nodes), _dev(d_feat_idx), _dev(d_n_feat)))

    def search_by_bow_device(self, n_pairs, kf, cur, d_feat_nodes, d_feat_idx, d_n_feat, d_kf_mp_flags, d_kps, d_desc, d_n, capacity,
                             d_matches, d_n_matches, nnratio=0.7, th_low=50, check_orientation=True):
        """ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...) (reference src/ORBmatcher.cc:269-471); kf and cur = (first, step)."""
        self._check(self._L.orbx_search_by_bow_device(self._h, n_pairs, kf[0], kf[1], cur[0], cur[1], _dev(d_feat_nodes), _dev(d_feat_idx),
                                                      _dev(d_n_feat), _dev(d_kf_mp_flags), _dev(d_kps), _dev(d_desc), _dev(d_n), capacity,
                                                      C.c_float(nnratio), th_low, int(check_orientation), _dev(d_matches), _dev(d_n_matches)))

    def search_by_bow_keyframes_device(self, n_pairs, kf1, kf2, d_feat_nodes, d_feat_idx, d_n_feat, d_kf1_mp_flags, d_kf2_mp_flags, d_kps, d_desc,
                                       d_n, capacity, d_matches12, d_n_matches, nnratio=0.8, th_low=50, check_orientation=True):
        """ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, ...) (reference src/ORBmatcher.cc:823-963); kf1 and kf2 = (first, step)."""
        self._check(self._L.orbx_search_by_bow_keyframes_device(self._h, n_pairs, kf1[0], kf1[1], kf2[0], kf2[1], _dev(d_feat_nodes), _dev(d_feat_idx),
                                                                _dev(d_n_feat), _dev(d_kf1_mp_flags), _dev(d_kf2_mp_flags), _dev(d_kps), _dev(d_desc), _dev(d_n),
                                                                capacity, C.c_float(nnratio), th_low, int(check_orientation), _dev(d_matches12),
                                                                _dev(d_n_matches)))

    def search_by_bow_two_eyes_device(self, n_pairs, kf, cur, d_feat_nodes, d_feat_idx, d_n_feat, d_kf_mp_flags, d_kps, d_desc, d_n, capacity,
                                      d_matches, d_n_matches, nnratio=0.7, th_low=50, check_orientation=True):
        """ORBmatcher::SearchByBoW(KeyFrame*, Frame&, ...) for two-camera frames (reference src/ORBmatcher.cc:269-471, F.Nleft != -1); kf and
        cur = (first, step) in PAIRS: pair X is frame 2X (left eye) and 2X + 1 (right eye).  d_kf_mp_flags and d_matches are
        [(2p + eye)*capacity + i]; a match names the keyframe feature by its concatenated index (left: i, right: Nleft of the keyframe + j)."""
        self._check(self._L.orbx_search_by_bow_two_eyes_device(self._h, n_pairs, kf[0], kf[1], cur[0], cur[1], _dev(d_feat_nodes), _dev(d_feat_idx),
                                                               _dev(d_n_feat), _dev(d_kf_mp_flags), _dev(d_kps), _dev(d_desc), _dev(d_n), capacity,
                                                               C.c_float(nnratio), th_low, int(check_orientation), _dev(d_matches),
                                                               _dev(d_n_matches)))

    def search_for_triangulation_device(self, n_pairs, kf1, kf2, d_feat_nodes, d_feat_idx, d_n_feat, d_kf1_mp_flags, d_kf2_mp_flags, d_kps_un,
                                        d_u_right, d_desc, d_n, capacity, d_f12, d_epipole, d_matches12, d_pairs, d_n_matches,
                                        only_stereo=False, coarse=False, th_low=50, check_orientation=True):
        """ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse) for one-camera keyframes with the Pinhole
        model (reference src/ORBmatcher.cc:965-1206); kf1 and kf2 = (first, step), step 0 = one keyframe against many.  d_f12 [p*9] row-major
        and d_epipole [p*2] are inputs; d_u_right may be None (no feature is stereo).  d_matches12 is [p*capacity + i], d_pairs
        [(p*capacity + k)*2] holds d_n_matches[p] pairs (i, d_matches12[i]) in increasing i."""
        self._check(self._L.orbx_search_for_triangulation_device(
            self._h, n_pairs, kf1[0], kf1[1], kf2[0], kf2[1], _dev(d_feat_nodes), _dev(d_feat_idx), _dev(d_n_feat), _dev(d_kf1_mp_flags),
            _dev(d_kf2_mp_flags), _dev(d_kps_un), _dev(d_u_right), _dev(d_desc), _dev(d_n), capacity, _dev(d_f12), _dev(d_epipole), int(only_stereo),
            int(coarse), th_low, int(check_orientation), _dev(d_matches12), _dev(d_pairs), _dev(d_n_matches)))

    def fuse_device(self, n_pairs, kf, mp, d_mp_world, d_mp_normal, d_mp_dist, d_mp_desc, d_n_mp, mp_capacity, d_mp_flags, d_poses, d_kps_un,
                    d_u_right, d_desc, d_n, capacity, d_grid_off, d_grid_idx, bounds, cam, mbf, d_best_idx, d_best_dist, d_exit, d_n_fused,
                    th=3.0, th_low=50, reproj_check=True, nlevels=None):
        """The search half of ORBmatcher::Fuse (reference src/ORBmatcher.cc:1399-1609; reproj_check=False: the Sim3 overload, :1611-1733) for
        one-camera keyframes with the Pinhole model; kf and mp = (first, step) of the keyframe / MapPoint list of pair p, mp step 0 = one list
        into many keyframes.  d_n_mp, d_u_right and d_exit may be None.  The caller replays the map-changing tail on the host in list order."""
        self._check(self._L.orbx_fuse_device(
            self._h, n_pairs, kf[0], kf[1], mp[0], mp[1], _dev(d_mp_world), _dev(d_mp_normal), _dev(d_mp_dist), _dev(d_mp_desc), _dev(d_n_mp), mp_capacity,
            _dev(d_mp_flags), _dev(d_poses), _dev(d_kps_un), _dev(d_u_right), _dev(d_desc), _dev(d_n), capacity, _dev(d_grid_off), _dev(d_grid_idx), _host_f32(bounds),
            _host_f32(cam), self.nlevels if nlevels is None else nlevels, mbf, th, th_low, int(reproj_check), _dev(d_best_idx), _dev(d_best_dist),
            _dev(d_exit), _dev(d_n_fused)))

    def fuse_two_eyes_device(self, n_pairs, kf, mp, d_mp_world, d_mp_normal, d_mp_dist, d_mp_desc, d_n_mp, mp_capacity, d_mp_flags, d_poses, tlr,
                             cam_left, cam_right, d_kps, d_desc, d_n, capacity, d_grid_off, d_grid_idx, bounds, d_best_idx, d_best_dist, d_exit,
                             d_n_fused, th=3.0, th_low=50, reproj_check=True, eyes=3, nlevels=None):
        """The search half of ORBmatcher::Fuse for two-camera keyframes (NLeft != -1, a KannalaBrandt8 pair; reference
        src/ORBmatcher.cc:1399-1609 with bRight false and true; reproj_check=False: the loop-closing overload, which needs eyes=1).  kf and
        mp = (first, step) of the RIG keyframe (device frames 2r, 2r + 1: frame_finish_two_eyes_device) / MapPoint list of pair p; d_poses per
        rig; tlr = mTlr (3x4); cam_left / cam_right = camera_kb8(...) of mpCamera / mpCamera2; d_kps the RAW keypoints.  eyes: bit 0 the left
        search, bit 1 the right.  The outputs are [(p*2 + eye)*mp_capacity + i] and d_n_fused [p*2 + eye]; d_best_idx is in the keyframe's
        numbering (right keypoint i = NLeft + i).  d_n_mp and d_exit may be None.  The caller replays the tails: left, then right."""
        self._check(self._L.orbx_fuse_two_eyes_device(
            self._h, n_pairs, kf[0], kf[1], mp[0], mp[1], _dev(d_mp_world), _dev(d_mp_normal), _dev(d_mp_dist), _dev(d_mp_desc), _dev(d_n_mp), mp_capacity,
            _dev(d_mp_flags), _dev(d_poses), _host_f32(tlr), _host_f32(cam_left), _host_f32(cam_right), _dev(d_kps), _dev(d_desc), _dev(d_n), capacity,
            _dev(d_grid_off), _dev(d_grid_idx), _host_f32(bounds), self.nlevels if nlevels is None else nlevels, th, th_low, int(reproj_check), int(eyes),
            _dev(d_best_idx), _dev(d_best_dist), _dev(d_exit), _dev(d_n_fused)))

    def search_for_triangulation_two_eyes_device(self, n_pairs, kf1, kf2, d_feat_nodes, d_feat_idx, d_n_feat, d_kf1_mp_flags, d_kf2_mp_flags, d_poses,
                                                 tlr, cam_left, cam_right, d_kps, d_desc, d_n, capacity, d_matches12, d_pairs, d_n_matches,
                                                 only_stereo=False, coarse=False, th_low=50, check_orientation=True, nlevels=None):
        """ORBmatcher::SearchForTriangulation for two-camera keyframes (NLeft != -1, a KannalaBrandt8 pair; reference src/ORBmatcher.cc:965-1206
        with the branches :994-1004 and :1099-1129).  kf1 and kf2 = (first, step) of the RIG keyframes (device frames 2X, 2X + 1), step 0 = one
        keyframe against many; the FeatureVectors are per eye (compute_bow_device); d_poses per rig; tlr = mTlr (3x4); cam_left / cam_right =
        camera_kb8(...); d_kps the RAW keypoints.  Flags and d_matches12 are [(2p + eye)*capacity + i]; d_matches12 holds keyframe 2's
        stacked index (right keypoint j = NLeft + j); d_pairs [(p*2*capacity + k)*2] holds d_n_matches[p] pairs in stacked numbering."""
        self._check(self._L.orbx_search_for_triangulation_two_eyes_device(
            self._h, n_pairs, kf1[0], kf1[1], kf2[0], kf2[1], _dev(d_feat_nodes), _dev(d_feat_idx), _dev(d_n_feat), _dev(d_kf1_mp_flags),
            _dev(d_kf2_mp_flags), _dev(d_poses), _host_f32(tlr), _host_f32(cam_left), _host_f32(cam_right), _dev(d_kps), _dev(d_desc), _dev(d_n),
            capacity, self.nlevels if nlevels is None else nlevels, int(only_stereo), int(coarse), th_low, int(check_orientation),
            _dev(d_matches12), _dev(d_pairs), _dev(d_n_matches)))

    def search_triangulation_two_eyes_count(self, on=True):
        """switches the debug counters of search_for_triangulation_two_eyes_device on or off (process-wide; off by default)"""
        self._check(self._L.orbx_debug_search_triangulation_two_eyes_enable(int(on)))

    def search_triangulation_two_eyes_stats(self):
        """(kb8TriangulateMatches calls, candidates with dist <= th_low) of the last counted search_for_triangulation_two_eyes_device, all
        pairs; waits for the whole device."""
        out = (C.c_int * 2)()
        self._check(self._L.orbx_debug_search_triangulation_two_eyes_stats(out))
        return out[0], out[1]

    def kb8_unproject_device(self, n, d_uv, cam, d_rays):
        """KannalaBrandt8::unproject (reference src/CameraModels/KannalaBrandt8.cpp:103-130) over n device-resident pixels: d_uv [n*2] in,
        d_rays [n*3] out (x, y, 1); cam = camera_kb8(...)."""
        self._check(self._L.orbx_kb8_unproject_device(self._h, n, _dev(d_uv), _host_f32(cam), _dev(d_rays)))

    def kb8_triangulate_device(self, n, d_kp1, d_kp2, cam1, cam2, r12, t12, sigma1, sigma2, d_z, d_x3d):
        """KannalaBrandt8::TriangulateMatches (reference src/CameraModels/KannalaBrandt8.cpp:336-405) over n device-resident keypoint pairs:
        d_kp1 / d_kp2 [n*2] pixels, r12 (3x3) and t12 (3) on the host, sigma1 / sigma2 = mvLevelSigma2 of the two octaves; d_z [n] is the
        return value (z1, or -1), d_x3d [n*3] the point in camera 1 (zeros when the parallax test left)."""
        self._check(self._L.orbx_kb8_triangulate_device(self._h, n, _dev(d_kp1), _dev(d_kp2), _host_f32(cam1), _host_f32(cam2), _host_f32(r12),
                                                        _host_f32(t12), sigma1, sigma2, _dev(d_z), _dev(d_x3d)))

    def stereo_fisheye_match_device(self, n_rigs, rigs, d_kps, d_desc, d_n, d_mono, capacity, tlr, cam_left, cam_right, d_left_to_right,
                                    d_right_to_left, d_depth, d_x3d, d_n_matches, d_n_desc_matches=None, nlevels=None):
        """Frame::ComputeStereoFishEyeMatches (reference src/Frame.cc:1139-1179) for n_rigs two-camera frames: rigs = (first, step) of the RIG
        frames (device frames 2r, 2r + 1); d_kps / d_desc / d_n / d_mono as extract_batch_device wrote them (RAW keypoints, Nleft / Nright,
        monoLeft / monoRight); tlr = mTlr (3x4); cam_left / cam_right = camera_kb8(...).  d_left_to_right [(2r)*capacity + i] holds the raw
        right index, d_right_to_left [(2r + 1)*capacity + j] the raw left index (the largest accepted one: the arrays are not inverse),
        d_depth [(2r)*capacity + i] and d_x3d [((2r)*capacity + i)*3] mvDepth and mvStereo3Dpoints (zeros where nothing matched);
        d_n_matches [q] nMatches, d_n_desc_matches [q] (or None) the rows that passed the ratio test.  The layout is what
        search_by_projection_two_eyes_device reads."""
        self._check(self._L.orbx_stereo_fisheye_match_device(
            self._h, n_rigs, rigs[0], rigs[1], _dev(d_kps), _dev(d_desc), _dev(d_n), _dev(d_mono), capacity, _host_f32(tlr), _host_f32(cam_left),
            _host_f32(cam_right), self.nlevels if nlevels is None else nlevels, _dev(d_left_to_right), _dev(d_right_to_left), _dev(d_depth),
            _dev(d_x3d), _dev(d_n_matches), _dev(d_n_desc_matches)))

    def stereo_fisheye_count(self, on=True):
        """switches the debug counter of stereo_fisheye_match_device on or off (process-wide; off by default)"""
        self._check(self._L.orbx_debug_stereo_fisheye_enable(int(on)))

    def stereo_fisheye_stats(self):
        """kb8TriangulateMatches calls of the last counted stereo_fisheye_match_device, all rigs; waits for the whole device."""
        out = (C.c_int * 1)()
        self._check(self._L.orbx_debug_stereo_fisheye_stats(out))
        return out[0]

    def create_new_map_points_device(self, n_pairs, kf1, kf2, d_pairs, d_n_matches, d_poses, cam, d_kps_un, d_kps, d_u_right, d_depth, d_n, capacity,
                                     mb, mbf, d_exit, d_x3d, d_n_new, d_mark1=None, d_mark2=None, far_points=False, th_far_points=0.0,
                                     nlevels=None):
        """The triangulation loop of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:481-707) for one-camera keyframes with the
        Pinhole model, on the d_pairs / d_n_matches search_for_triangulation_device wrote; kf1 and kf2 = (first, step).  d_poses [f*12] per
        batch frame; cam = camera(...) (fx, fy, cx, cy are read); d_u_right None = monocular (d_kps and d_depth may be None then).  d_exit
        [p*capacity + k] holds the orbx_new_point_exit of match k, d_x3d [(p*capacity + k)*3] the world point (zeros on a rejection),
        d_n_new [p] the accepted count; d_mark1 / d_mark2 (or None): flag rows [p*capacity + i] in which bit 0 of every accepted match's
        keypoint is set."""
        self._check(self._L.orbx_create_new_map_points_device(
            self._h, n_pairs, kf1[0], kf1[1], kf2[0], kf2[1], _dev(d_pairs), _dev(d_n_matches), _dev(d_poses), _host_f32(cam), _dev(d_kps_un),
            _dev(d_kps), _dev(d_u_right), _dev(d_depth), _dev(d_n), capacity, self.nlevels if nlevels is None else nlevels, mb, mbf,
            int(far_points), th_far_points, _dev(d_exit), _dev(d_x3d), _dev(d_n_new), _dev(d_mark1), _dev(d_mark2)))

    def create_new_map_points_two_eyes_device(self, n_pairs, kf1, kf2, d_pairs, d_n_matches, d_poses, tlr, cam_left, cam_right, d_kps, d_n, capacity,
                                              d_exit, d_x3d, d_n_new, d_mark1=None, d_mark2=None, far_points=False, th_far_points=0.0,
                                              nlevels=None):
        """The same loop for two-camera keyframes (NLeft != -1, a KannalaBrandt8 pair), on the stacked d_pairs / d_n_matches
        search_for_triangulation_two_eyes_device wrote; kf1 and kf2 = (first, step) of the RIG keyframes.  The lists are 2 * capacity long:
        d_exit [p*2*capacity + k], d_x3d [(p*2*capacity + k)*3]; the marks are [(2p + eye)*capacity + i]."""
        self._check(self._L.orbx_create_new_map_points_two_eyes_device(
            self._h, n_pairs, kf1[0], kf1[1], kf2[0], kf2[1], _dev(d_pairs), _dev(d_n_matches), _dev(d_poses), _host_f32(tlr), _host_f32(cam_left),
            _host_f32(cam_right), _dev(d_kps), _dev(d_n), capacity, self.nlevels if nlevels is None else nlevels, int(far_points), th_far_points,
            _dev(d_exit), _dev(d_x3d), _dev(d_n_new), _dev(d_mark1), _dev(d_mark2)))

    def update_map_points_device(self, n_points, d_obs_off, d_obs, d_obs_flags, d_ref, d_slot, d_mp_world, d_poses, n_frames, d_kps_un, d_desc,
                                 d_n, capacity, d_mp_desc, d_mp_normal, d_mp_dist, d_best, d_best_median, d_status, what=3, nlevels=None):
        """MapPoint::ComputeDistinctiveDescriptors (what bit 0) and MapPoint::UpdateNormalAndDepth (what bit 1; reference src/MapPoint.cc:330-403,
        :427-494) for n_points listed MapPoints over one-camera keyframes.  d_obs_off [n_points + 1] is a CSR over d_obs [o*2] = (device frame,
        keypoint row), one entry per descriptor in the reference's iteration order of mObservations; d_obs_flags (or None) bit 0 =
        pKF->isBad(), left out of the descriptor but counted in the normal; d_ref [m] the position of mpRefKF's entry in the list; d_slot
        (or None = m) the row of the MapPoint tables the point reads (d_mp_world) and writes (d_mp_desc [slot*32], d_mp_normal [slot*3],
        d_mp_dist [slot*3] = fuse_device's triple).  d_poses [f*12] of the n_frames batch frames; d_kps_un: only the octave is read.
        d_best [m] holds BestIdx among the entries that took part (-1: none), d_best_median [m] its median, d_status [m] an
        orbx_map_point_update (0 OK, 1 EMPTY, 2 NO_DESCRIPTOR, 3 BAD_INDEX, 4 TOO_LONG: more than MAX_OBSERVATIONS entries)."""
        self._check(self._L.orbx_update_map_points_device(
            self._h, n_points, _dev(d_obs_off), _dev(d_obs), _dev(d_obs_flags), _dev(d_ref), _dev(d_slot), _dev(d_mp_world), _dev(d_poses), n_frames,
            _dev(d_kps_un), _dev(d_desc), _dev(d_n), capacity, self.nlevels if nlevels is None else nlevels, int(what), _dev(d_mp_desc),
            _dev(d_mp_normal), _dev(d_mp_dist), _dev(d_best), _dev(d_best_median), _dev(d_status)))

    def update_map_points_two_eyes_device(self, n_points, d_obs_off, d_obs, d_obs_flags, d_ref, d_slot, d_mp_world, d_poses, tlr, n_rigs, d_kps,
                                          d_desc, d_n, capacity, d_mp_desc, d_mp_normal, d_mp_dist, d_best, d_best_median, d_status, what=3,
                                          nlevels=None):
        """The same update for two-camera keyframes (NLeft != -1): rig keyframe r is device frames 2r, 2r + 1 (fuse_two_eyes_device's
        layout), d_poses [r*12] per rig, tlr = mTlr (3x4), d_kps the RAW keypoints.  A right keypoint NLeft + j is the entry (2r + 1, j);
        a keyframe with both indices gives its left entry, then its right entry.  d_ref names the left entry of mpRefKF if it has one, else
        the right; the reference centre is the rig's LEFT centre either way."""
        self._check(self._L.orbx_update_map_points_two_eyes_device(
            self._h, n_points, _dev(d_obs_off), _dev(d_obs), _dev(d_obs_flags), _dev(d_ref), _dev(d_slot), _dev(d_mp_world), _dev(d_poses),
            _host_f32(tlr), n_rigs, _dev(d_kps), _dev(d_desc), _dev(d_n), capacity, self.nlevels if nlevels is None else nlevels, int(what),
            _dev(d_mp_desc), _dev(d_mp_normal), _dev(d_mp_dist), _dev(d_best), _dev(d_best_median), _dev(d_status)))

    def two_view_shape(self, shape=1):
        """which hypothesis kernel reconstruct_two_views_device launches (process-wide): 1 rows over the lanes (default), 0 one lane out of LDS"""
        self._check(self._L.orbx_debug_two_view_shape(int(shape)))

    def new_map_points_count(self, on=True):
        """switches the debug counters of the two create_new_map_points entries on or off (process-wide; off by default)"""
        self._check(self._L.orbx_debug_new_map_points_enable(int(on)))

    def new_map_points_stats(self):
        """(matches that took the SVD branch, matches that took an UnprojectStereo branch) of the last counted launch, all pairs; waits
        for the whole device."""
        out = (C.c_int * 2)()
        self._check(self._L.orbx_debug_new_map_points_stats(out))
        return out[0], out[1]

    def sim3_solve_steps(self, mask=7):
        """which kernels sim3_solve_device launches (process-wide; tools/sim3_solver_rate.py): 1 prepare, 3 + hypotheses, 7 all (default)"""
        self._check(self._L.orbx_debug_sim3_solve_steps(int(mask)))

    def search_by_projection_sim3_device(self, n_pairs, kf, mp, d_mp_world, d_mp_normal, d_mp_dist, d_mp_desc, d_n_mp, mp_capacity, d_mp_flags,
                                         d_poses, d_kps_un, d_desc, d_n, capacity, d_grid_off, d_grid_idx, bounds, cam, d_occupied, d_matches,
                                         d_match_idx, d_match_dist, d_exit, d_n_matches, projection=0, th=3.0, th_low=50, ratio_hamming=1.0,
                                         nlevels=None):
        """The Sim3 overloads of ORBmatcher::SearchByProjection (reference src/ORBmatcher.cc:473-586, projection=0; :588-704, projection=1;
        loop closing) for one-camera keyframes with the Pinhole model; kf and mp = (first, step) of the keyframe / MapPoint list of pair p,
        kf step 0 = several candidates into one keyframe.  d_poses is [p*12], per pair.  d_n_mp, d_occupied and d_exit may be None.  A match
        closes its keypoint for the later MapPoints of the list, as in the reference; d_matches [p*capacity + idx] names the list index."""
        self._check(self._L.orbx_search_by_projection_sim3_device(
            self._h, n_pairs, kf[0], kf[1], mp[0], mp[1], _dev(d_mp_world), _dev(d_mp_normal), _dev(d_mp_dist), _dev(d_mp_desc), _dev(d_n_mp), mp_capacity,
            _dev(d_mp_flags), _dev(d_poses), _dev(d_kps_un), _dev(d_desc), _dev(d_n), capacity, _dev(d_grid_off), _dev(d_grid_idx), _host_f32(bounds), _host_f32(cam),
            self.nlevels if nlevels is None else nlevels, int(projection), th, th_low, ratio_hamming, _dev(d_occupied), _dev(d_matches),
            _dev(d_match_idx), _dev(d_match_dist), _dev(d_exit), _dev(d_n_matches)))

    def frustum_requests_device(self, n_pairs, cur, mp, d_mp_world, d_mp_normal, d_mp_dist, d_mp_desc, d_mp_angle, d_n_mp, mp_capacity, d_mp_flags,
                                d_poses, cam, bounds, d_queries, d_query_desc, d_query_src, d_n_queries, d_track, d_n_in_view,
                                mode=FRUSTUM_LOCAL_MAP, mbf=0.0, view_cos_limit=0.5, th=1.0, far_points=False, th_far_points=0.0, nlevels=None):
        """Frame::isInFrustum over a MapPoint list plus the prelude of ORBmatcher::SearchByProjection(F, vpMapPoints, ...) (reference
        src/Frame.cc:493-570, src/Tracking.cc:2941-2959, src/ORBmatcher.cc:50-73; mode=FRUSTUM_LOCAL_MAP), or the projection of a keyframe's
        MapPoints for Relocalization (src/ORBmatcher.cc:2183-2230; mode=FRUSTUM_RELOCALIZATION).  cur and mp = (first, step) of the frame /
        MapPoint list of pair p.  Writes the requests of every pair compacted in list order (d_queries of PROJ_QUERY_DTYPE, d_query_desc,
        d_query_src, d_n_queries: feed them to search_by_projection_device with query_capacity = mp_capacity and desc_blocks = (0, 1)), one
        TRACK_RECORD_DTYPE per list entry and nToMatch per pair.  d_n_mp may be None; d_mp_angle in the local-map mode and d_mp_normal in
        the relocalisation mode as well."""
        self._check(self._L.orbx_frustum_requests_device(
            self._h, n_pairs, cur[0], cur[1], mp[0], mp[1], _dev(d_mp_world), _dev(d_mp_normal), _dev(d_mp_dist), _dev(d_mp_desc), _dev(d_mp_angle), _dev(d_n_mp),
            mp_capacity, _dev(d_mp_flags), _dev(d_poses), _host_f32(cam), _host_f32(bounds), self.nlevels if nlevels is None else nlevels, int(mode), mbf,
            view_cos_limit, th, int(bool(far_points)), th_far_points, _dev(d_queries), _dev(d_query_desc), _dev(d_query_src), _dev(d_n_queries),
            _dev(d_track), _dev(d_n_in_view)))

    def frustum_requests_two_eyes_device(self, n_pairs, cur, mp, d_mp_world, d_mp_normal, d_mp_dist, d_mp_desc, d_n_mp, mp_capacity, d_mp_flags,
                                         d_mp_prev_depth, d_poses, trl, tlr, cam_left, cam_right, bounds, query_capacity, d_queries, d_query_desc,
                                         d_query_src, d_n_queries, d_n_wanted, d_track, d_n_in_view, view_cos_limit=0.5, th=1.0, far_points=False,
                                         th_far_points=0.0, nlevels=None):
        """Frame::isInFrustum's Nleft != -1 branch (isInFrustumChecks per eye) over a MapPoint list plus the prelude of
        ORBmatcher::SearchByProjection(F, vpMapPoints, ...) for two-camera rigs (reference src/Frame.cc:571-581, :1181-1254,
        src/Tracking.cc:2941-2959, src/ORBmatcher.cc:50-73, :145-151).  cur and mp = (first, step) of the RIG frame / MapPoint list of pair
        p; d_poses per rig frame; trl / tlr = mTrl / mTlr (3x4); cam_left / cam_right = camera_kb8(...) of mpCamera / mpCamera2.  Writes two
        TRACK_RECORD_DTYPE per list entry (left, right), the slots of every pair compacted in list order (two PROJ_QUERY_DTYPE each in
        d_queries, d_query_desc, d_query_src, d_n_queries: feed them to search_by_projection_two_eyes_device with the same query_capacity
        and desc_blocks = (0, 1)), the count the list produced (d_n_wanted) and nToMatch per pair.  d_n_mp, d_mp_prev_depth and d_n_wanted
        may be None."""
        self._check(self._L.orbx_frustum_requests_two_eyes_device(
            self._h, n_pairs, cur[0], cur[1], mp[0], mp[1], _dev(d_mp_world), _dev(d_mp_normal), _dev(d_mp_dist), _dev(d_mp_desc), _dev(d_n_mp), mp_capacity,
            _dev(d_mp_flags), _dev(d_mp_prev_depth), _dev(d_poses), _host_f32(trl), _host_f32(tlr), _host_f32(cam_left), _host_f32(cam_right), _host_f32(bounds),
            self.nlevels if nlevels is None else nlevels, view_cos_limit, th, int(bool(far_points)), th_far_points, query_capacity, _dev(d_queries),
            _dev(d_query_desc), _dev(d_query_src), _dev(d_n_queries), _dev(d_n_wanted), _dev(d_track), _dev(d_n_in_view)))

    def debug_sim3_search_stats(self):
        """(rounds of pair 0, requests settled by a re-scan, 100-MHz ticks of pair 0's settling workgroup, 0) of the last Sim3 search"""
        out = (C.c_int * 4)()
        self._check(self._L.orbx_debug_sim3_search_stats(out))
        return tuple(out)

    def stereo_from_rgbd_device(self, n_frames, d_kps, d_kps_un, d_n, capacity, d_depth, depth_is_u16, rows, cols, depth_map_factor, mbf,
                                d_u_right, d_depth_out, depth_stride_bytes=None, depth_frame_stride_bytes=None):
        """Frame::ComputeStereoFromRGBD with GrabImageRGBD's depth conversion (reference src/Frame.cc:994-1015, src/Tracking.cc:1003-1004)."""
        elem = 2 if depth_is_u16 else 4
        depth_stride_bytes = cols * elem if depth_stride_bytes is None else depth_stride_bytes
        depth_frame_stride_bytes = rows * depth_stride_bytes if depth_frame_stride_bytes is None else depth_frame_stride_bytes
        self._check(self._L.orbx_stereo_from_rgbd_device(self._h, n_frames, _dev(d_kps), _dev(d_kps_un), _dev(d_n), capacity, _dev(d_depth),
                                                         int(depth_is_u16), rows, cols, depth_stride_bytes, depth_frame_stride_bytes,
                                                         depth_map_factor, mbf, _dev(d_u_right), _dev(d_depth_out)))

    def gray_from_color_device(self, n_frames, d_src, rows, cols, channels, red_first, d_gray, src_stride=None, src_frame_stride=None,
                               gray_stride=None, gray_frame_stride=None):
        """cv::cvtColor(RGB/BGR/RGBA/BGRA -> GRAY) as Tracking::GrabImage* applies it (reference src/Tracking.cc:915-941)."""
        src_stride = cols * channels if src_stride is None else src_stride
        src_frame_stride = rows * src_stride if src_frame_stride is None else src_frame_stride
        gray_stride = cols if gray_stride is None else gray_stride
        gray_frame_stride = rows * gray_stride if gray_frame_stride is None else gray_frame_stride
        self._check(self._L.orbx_gray_from_color_device(self._h, n_frames, _dev(d_src), rows, cols, channels, int(red_first), src_stride,
                                                        src_frame_stride, _dev(d_gray), gray_stride, gray_frame_stride))

    def set_stream(self, stream_ptr):
        self._check(self._L.orbx_set_stream(self._h, C.c_void_p(int(stream_ptr))))

    def synchronize(self):
        self._check(self._L.orbx_synchronize(self._h))

    # ---- mvImagePyramid (inc/ORBextractor.h:85) ----
    def image_pyramid_level(self, level, frame=0, bordered=False):
        w, h = C.c_int(), C.c_int()
        sizes = compute_level_sizes(self.max_height, self.max_width, self.scaleFactor, self.nlevels)
        buf = np.zeros((sizes[0][1] + 38, sizes[0][0] + 38), np.uint8)
        self._check(self._L.orbx_get_level(self._h, frame, level, int(bordered), _ptr(buf), buf.strides[0], C.byref(w), C.byref(h)))
        if bordered:
            return buf[:h.value + 38, :w.value + 38].copy()
        return buf[:h.value, :w.value].copy()

    def fetch_pyramid(self, frame=0, bordered=False):
        """All levels of one frame in ONE device-to-host copy (orbx_fetch_pyramid): a list of arrays, each a copy of the w x h level (or of
        the (w + 38) x (h + 38) buffer with the BORDER_REFLECT_101 frame the reference's views sit in, ORBextractor.cc:1173-1177)."""
        base = C.c_void_p()
        off = np.zeros(self.nlevels, np.uint64); st = np.zeros(self.nlevels, np.int32)
        w = np.zeros(self.nlevels, np.int32); h = np.zeros(self.nlevels, np.int32)
        self._check(self._L.orbx_fetch_pyramid(self._h, frame, C.byref(base), _ptr(off), _ptr(st), _ptr(w), _ptr(h)))
        out = []
        for l in range(self.nlevels):
            e = 19 if bordered else 0
            rows, cols, stride = int(h[l]) + 2 * e, int(w[l]) + 2 * e, int(st[l])
            start = base.value + int(off[l]) - e * stride - e
            buf = (C.c_uint8 * (stride * rows)).from_address(start)
            out.append(np.frombuffer(buf, np.uint8).reshape(rows, stride)[:, :cols].copy())
        return out

    @property
    def mvImagePyramid(self):
        return self.fetch_pyramid()

    # ---- the two public stage methods (inc/ORBextractor.h:87-90; src/orb_extractor/main_orb_extractor.cpp:43-46 calls them) ----
    def ComputePyramid(self, image):
        image = np.asarray(image)
        if image.dtype != np.uint8 or image.ndim != 2 or image.strides[1] != 1 or image.size == 0:
            raise ValueError("image must be a non-empty 2-D uint8 array with contiguous rows (CV_8UC1)")
        self._check(self._L.orbx_compute_pyramid(self._h, _ptr(image), image.shape[0], image.shape[1], image.strides[0]))

    def ComputeKeyPointsOctTree(self):
        """allKeypoints: one array per level, level coordinates, angles set (ORBextractor.cc:773-888)."""
        cap = self.capacity
        lvl = np.zeros(cap, KEYPOINT_DTYPE); counts = np.zeros(self.nlevels, np.int32)
        self._check(self._L.orbx_compute_keypoints_octree(self._h, _ptr(lvl), cap, _ptr(counts)))
        return _split_levels(lvl, counts)

    def policy(self):
        """The launch-policy switches as orbx_create read them (include/orbx.h: orbx_debug_policy)."""
        return (self._L.orbx_debug_policy(self._h) or b"").decode()

    def clock_probe(self, slot):
        """Asynchronous sample of the shader clock beside the handle's running work (include/orbx.h: orbx_debug_clock_probe)."""
        self._check(self._L.orbx_debug_clock_probe(self._h, int(slot)))

    def clock_read(self, n_slots):
        ghz = np.zeros(n_slots, np.float64)
        self._check(self._L.orbx_debug_clock_read(self._h, int(n_slots), _ptr(ghz)))
        return ghz

    def last_forms(self):
        """(pyramid form, region side of k_pyr_cols, blur form) of the last call: include/orbx.h, orbx_debug_last_forms."""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._check(self._L.orbx_debug_last_forms(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def lds_pollutions(self):
        """Launches of the LDS polluter on this handle since it was made (include/orbx.h: orbx_debug_lds_pollutions)."""
        n = self._L.orbx_debug_lds_pollutions(self._h)
        self._check(min(n, 0))
        return n

    def blurred_level_exists(self, level):
        """whether the last call left a blurred image of `level` (it did not where the blur ran per keypoint inside k_describe)"""
        form = self.last_forms()[2]
        return form not in (3, 5) or (form == 5 and level >= self._L.orbx_debug_last_split_level(self._h))

    # ---- introspection for tests/bench ----
    def debug_candidates(self, level, frame=0):
        n = C.c_int()
        self._check(self._L.orbx_debug_num_candidates(self._h, frame, level, C.byref(n)))
        out = np.zeros(max(n.value, 1), KEYPOINT_DTYPE)
        self._check(self._L.orbx_debug_get_candidates(self._h, frame, level, _ptr(out), len(out)))
        return out[:n.value].copy()

    def debug_blurred(self, level, frame=0):
        w, h = self.image_pyramid_level(level, frame).shape[::-1]
        out = np.zeros((h, w), np.uint8)
        self._check(self._L.orbx_debug_get_blurred(self._h, frame, level, _ptr(out), out.strides[0]))
        return out

    def profile(self, enable=True):
        self._check(self._L.orbx_profile_enable(self._h, int(enable)))
        self._check(self._L.orbx_profile_reset(self._h))

    def profile_read(self):
        ms = np.zeros(ORBX_NUM_KERNELS, np.float64); n = np.zeros(ORBX_NUM_KERNELS, np.int64)
        self._check(self._L.orbx_profile_read(self._h, _ptr(ms), _ptr(n)))
        # keyed by the kernel that ran in each slot on this handle, as rocprofv3 names it (k_pyr_cols, k_octree_256, ...)
        return {self._L.orbx_profile_kernel_name_of(self._h, i).decode(): (float(ms[i]), int(n[i])) for i in range(ORBX_NUM_KERNELS)}

    def algorithmic_bytes(self, rows, cols, n_out):
        return int(self._L.orbx_algorithmic_bytes(self._h, rows, cols, n_out))
