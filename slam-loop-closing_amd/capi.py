"""ctypes binding of include/lcm.h — the C ABI of the MI355X loop-closure matcher.

This module is plumbing for tests, bench.py and __graft_entry__: the product is the shared library
`lib/liblcm_hip.so` (hand-written gfx950 kernels behind a C ABI).  There is no Python or CPU compute path here;
if the library is missing or no HIP device is present, everything raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# LCM_LIB_PATH: test plumbing only (e.g. the host-sanitizer build of the same sources, `make -C csrc asan`)
LIB_PATH = os.environ.get("LCM_LIB_PATH") or os.path.join(_HERE, "lib", "liblcm_hip.so")
DESC_BYTES = 32
SIFT_BYTES = 128          # a SIFT row: 128 uint8 (pair mode under L2)
KEY_SHIFT = 22
TUNE_ITEM_SLOTS, TUNE_ONLINE_SPLIT, TUNE_PACKED, TUNE_ONLINE_STREAMS, TUNE_PACKED_SCRATCH_MB = 0, 1, 2, 3, 4      # lcm_tuning
TUNE_PAIR_UPLOAD_KERNEL, TUNE_PAIR_HOST_FOLD = 5, 6


OK, ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_CAPACITY, ERR_ORDER, ERR_NOT_FOUND, ERR_OOM = 0, -1, -2, -3, -4, -5, -6, -7   # lcm_status


class LcmError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"lcm error {code}: {msg}")
        self.code = code


class Params(C.Structure):
    _fields_ = [("ratio", C.c_int32), ("dist_floor", C.c_int32), ("min_matches", C.c_int32),
                ("min_gap", C.c_int32), ("sim_threshold", C.c_double), ("cross_check", C.c_int32),
                ("reserved", C.c_int32)]


class Score(C.Structure):
    _fields_ = [("good_count", C.c_uint32), ("min_dist", C.c_uint16), ("n_train", C.c_uint16)]


class DMatch(C.Structure):
    _fields_ = [("query_idx", C.c_int32), ("train_idx", C.c_int32), ("img_idx", C.c_int32), ("distance", C.c_float)]


class LoopCandidate(C.Structure):
    _fields_ = [("current_frame_id", C.c_int32), ("matched_frame_id", C.c_int32), ("num_matches", C.c_int32),
                ("similarity_score", C.c_double)]


class RatioLoopParams(C.Structure):
    """lcm_ratio_loop_params: the reference's loop rule on the ratio-test score (src/main.cpp:1379-1388)."""
    _fields_ = [("ratio", C.c_double), ("min_rows", C.c_int32), ("min_matches", C.c_int32)]


class PointPair(C.Structure):
    """lcm_point_pair: the keypoints of one surviving match, kp[query_idx].pt and kp[train_idx].pt."""
    _fields_ = [("qx", C.c_float), ("qy", C.c_float), ("tx", C.c_float), ("ty", C.c_float)]


class EpiParams(C.Structure):
    """lcm_epi_params: the camera matrix and the settings of the essential-matrix RANSAC (64 bytes)."""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("threshold", C.c_double),
                ("min_ratio", C.c_double), ("iters", C.c_int32), ("min_inliers", C.c_int32), ("seed", C.c_uint32),
                ("reserved", C.c_uint32)]


class EpiResult(C.Structure):
    """lcm_epi_result: a pair's winning essential matrix (row-major) and its inlier count (88 bytes)."""
    _fields_ = [("E", C.c_double * 9), ("n_points", C.c_int32), ("n_inliers", C.c_int32), ("best_iter", C.c_int32),
                ("status", C.c_int32)]


EPI_OK, EPI_TOO_FEW = 0, 1               # lcm_epi_status


class PoseParams(C.Structure):
    """lcm_pose_params: the far limit of the depth test (in baselines) and the pose verdict's limit (32 bytes)."""
    _fields_ = [("max_depth", C.c_double), ("min_pose_inliers", C.c_int32), ("reserved", C.c_int32 * 5)]


class PoseResult(C.Structure):
    """lcm_pose_result: a pair's relative pose X2 = R X1 + t (R row-major, |t| = 1), the four hypotheses' counts, the records
    that took part, those in front of both cameras under the chosen hypothesis, that hypothesis, the status (128 bytes)."""
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("counts", C.c_int32 * 4), ("n_used", C.c_int32),
                ("n_good", C.c_int32), ("choice", C.c_int32), ("status", C.c_int32)]


POSE_OK, POSE_NO_MODEL = 0, 1            # lcm_pose_status


class PgoParams(C.Structure):
    """lcm_pgo_params: the Gauss-Newton correction's step, damping, stopping rule, the loop edge's weight and direction (64 bytes)."""
    _fields_ = [("eps", C.c_double), ("damping", C.c_double), ("min_update", C.c_double), ("loop_weight", C.c_double),
                ("max_iters", C.c_int32), ("loop_direction", C.c_int32), ("reserved", C.c_int32 * 6)]


class PgoInfo(C.Structure):
    """lcm_pgo_info: the first and last cost, the last update and damping, the iterations, the status, the sizes (48 bytes)."""
    _fields_ = [("cost_first", C.c_double), ("cost_last", C.c_double), ("max_update", C.c_double), ("lambda_", C.c_double),
                ("iterations", C.c_int32), ("status", C.c_int32), ("n_params", C.c_int32), ("n_border", C.c_int32)]


PGO_CONVERGED, PGO_MAX_ITERS, PGO_SOLVE_FAILED, PGO_HALF_TURN = 0, 1, 2, 3      # lcm_pgo_status
PGO_LOOP_AS_WRITTEN, PGO_LOOP_INVERTED = 0, 1                                   # lcm_pgo_loop_direction
PGO_MAX_POSES, PGO_MAX_LOOPS = 4096, 8


class BaParams(C.Structure):
    """lcm_ba_params: the camera matrix, the Gauss-Newton steps' constants, the outlier pass's thresholds, the iteration counts
    and the smallest observation counts of an adjusted camera and point (112 bytes)."""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("eps", C.c_double),
                ("damping", C.c_double), ("min_update", C.c_double), ("outlier_px", C.c_double), ("min_spread", C.c_double),
                ("spread_factor", C.c_double), ("outer_iters", C.c_int32), ("inner_iters", C.c_int32), ("min_cam_obs", C.c_int32),
                ("min_point_obs", C.c_int32), ("reserved", C.c_int32 * 4)]


class BaInfo(C.Structure):
    """lcm_ba_info: the mean error before the run and after every outer iteration, the rounds, the cameras and the points per
    status after the last round (184 bytes)."""
    _fields_ = [("mean_error", C.c_double * 17), ("outer_iters", C.c_int32), ("cameras", C.c_int32 * 5), ("points", C.c_int32 * 5),
                ("reserved", C.c_int32)]


class BaMapReport(C.Structure):
    """lcm_ba_map_report: lcm_ba_refine_map's four errors, the distance threshold, the outliers, what was kept (56 bytes)."""
    _fields_ = [("error_before", C.c_double), ("error_after", C.c_double), ("error_filtered", C.c_double), ("error_final", C.c_double),
                ("threshold", C.c_double), ("n_outliers", C.c_int32), ("n_points", C.c_int32), ("n_obs", C.c_int32), ("reserved", C.c_int32)]


BA_CONVERGED, BA_MAX_ITERS, BA_SOLVE_FAILED, BA_HALF_TURN, BA_SKIPPED = 0, 1, 2, 3, 4      # lcm_ba_status
BA_MAX_CAMERAS, BA_MAX_POINTS, BA_MAX_OBS, BA_MAX_ITERS_PER_LOOP = 4096, 1 << 24, 1 << 24, 16


class MapParams(C.Structure):
    """lcm_map_params: the camera matrix, the triangulation's filters and the keyframe gates (112 bytes)."""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("min_parallax_deg", C.c_double),
                ("max_reproj", C.c_double), ("min_depth", C.c_double), ("max_depth", C.c_double), ("min_displacement", C.c_double),
                ("max_displacement", C.c_double), ("min_inlier_ratio", C.c_double), ("min_tracked", C.c_int32), ("min_inliers", C.c_int32),
                ("min_pose_inliers", C.c_int32), ("reserved", C.c_int32 * 3)]


class MapKeyframeReport(C.Structure):
    """lcm_map_keyframe_report: the new keyframe's pose (R row-major, t), the median displacement, the baseline, the verdict, the
    list's length, the pose's inliers, the points created and merged, the records per status (168 bytes)."""
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("median", C.c_double), ("baseline", C.c_double), ("verdict", C.c_int32),
                ("n_matches", C.c_int32), ("n_inliers", C.c_int32), ("n_new", C.c_int32), ("n_merged", C.c_int32), ("reserved", C.c_int32),
                ("counts", C.c_int32 * 8)]


# lcm_map_status, lcm_map_verdict
MAP_NOT_INLIER, MAP_NO_POINT, MAP_REJ_DEPTH, MAP_REJ_PARALLAX, MAP_REJ_REPROJ, MAP_ACCEPTED, MAP_MERGED, MAP_NEW = range(8)
MAP_KEYFRAME, MAP_FEW_MATCHES, MAP_LITTLE_MOTION, MAP_MUCH_MOTION, MAP_NO_POSE, MAP_FEW_INLIERS = range(6)
MAP_MAX_PAIRS, MAP_MAX_RECORDS = 4096, 1 << 24
_MAP_FIELDS = tuple(f[0] for f in MapParams._fields_[:-1])


class SiftParams(C.Structure):
    """lcm_sift_params: the detector's thresholds and sigmas, the layers per octave, the first octave, the border, the steps (64 bytes)."""
    _fields_ = [("contrast_threshold", C.c_double), ("edge_threshold", C.c_double), ("sigma", C.c_double), ("init_sigma", C.c_double),
                ("n_octave_layers", C.c_int32), ("upsample", C.c_int32), ("n_octaves", C.c_int32), ("border", C.c_int32), ("max_steps", C.c_int32),
                ("reserved", C.c_int32 * 3)]


class SiftPlanInfo(C.Structure):
    """lcm_sift_plan_info: a scale space's octaves, sizes, sigmas and radii (320 bytes)."""
    _fields_ = [("n_octaves", C.c_int32), ("n_gauss", C.c_int32), ("n_dog", C.c_int32), ("base_w", C.c_int32), ("base_h", C.c_int32),
                ("first_radius", C.c_int32), ("max_radius", C.c_int32), ("reserved", C.c_int32), ("width", C.c_int32 * 16), ("height", C.c_int32 * 16),
                ("radius", C.c_int32 * 12), ("first_sigma", C.c_double), ("sig", C.c_double * 12), ("space_floats", C.c_uint64)]


class SiftSpaceInfo(C.Structure):
    """lcm_sift_space_info_t: what a space was made for, its last image, its device bytes and candidate room, the last build's plan."""
    _fields_ = [("max_w", C.c_int32), ("max_h", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("device_bytes", C.c_uint64),
                ("candidate_capacity", C.c_uint64), ("plan", SiftPlanInfo)]


SIFT_GAUSSIAN, SIFT_DOG = 0, 1                                                    # lcm_sift_kind
SIFT_MAX_SIDE, SIFT_MAX_OCTAVES, SIFT_MAX_RADIUS, SIFT_MAX_CANDIDATES = 4096, 16, 48, 1 << 20
_SIFT_FIELDS = tuple(f[0] for f in SiftParams._fields_[:-1])


class LoParams(C.Structure):
    """lcm_lo_params: the rounds of the RANSAC's local optimisation and their threshold multipliers (96 bytes)."""
    _fields_ = [("rounds", C.c_int32), ("seeds", C.c_int32), ("mult", C.c_double * 8), ("reserved", C.c_uint32 * 6)]


class LoInfo(C.Structure):
    """lcm_lo_info: which seed and round won a pair (round -1: the RANSAC's record kept), the RANSAC's count, the pair's
    status (16 bytes)."""
    _fields_ = [("seed_iter", C.c_int32), ("round", C.c_int32), ("n_inliers_ransac", C.c_int32), ("status", C.c_int32)]


LO_SEEDS = 64
LO_OK, LO_TOO_FEW, LO_DEGENERATE, LO_NO_MODEL = 0, 1, 2, 3      # lcm_lo_status


class L2DbInfo(C.Structure):
    """lcm_l2_db_info: the SIFT keyframe store's occupancy and the table bytes of its last search."""
    _fields_ = [("frames", C.c_int32), ("reserved_", C.c_int32), ("tiles_used", C.c_uint64), ("tiles_reserved", C.c_uint64),
                ("device_bytes", C.c_uint64), ("table_bytes", C.c_uint64)]


class LaunchInfo(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("pairs", C.c_uint64), ("distances", C.c_uint64),
                ("algo_bytes", C.c_uint64), ("launches", C.c_uint32), ("workgroups", C.c_uint32),
                ("aux_kernel_ms", C.c_double), ("route", C.c_uint32), ("launches_in_flight", C.c_uint32),
                ("score_ms_sum", C.c_double), ("score_launches", C.c_uint32), ("reserved_", C.c_uint32)]


ROUTE_PLAIN, ROUTE_PACKED, ROUTE_SPLIT, ROUTE_MATRIX, ROUTE_CROSS = range(5)      # lcm_route


class OnlineStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("launches", C.c_uint64), ("queries", C.c_uint64), ("pairs", C.c_uint64),
                ("distances", C.c_uint64), ("algo_bytes", C.c_uint64)]


class GroupInfo(C.Structure):
    _fields_ = [("n_devices", C.c_int32), ("rccl_ranks", C.c_int32), ("pairs", C.c_uint64), ("distances", C.c_uint64),
                ("algo_bytes", C.c_uint64), ("kernel_ms_max", C.c_double), ("gather_merge_ms", C.c_double),
                ("download_ms", C.c_double), ("gathered_query_bytes", C.c_uint64), ("gathered_score_bytes", C.c_uint64),
                ("allgather_ms", C.c_double), ("kernel_ms", C.c_double * 8), ("shard_pairs", C.c_uint64 * 8),
                ("arena_gather_skipped", C.c_int32), ("loopback", C.c_int32)]


SCORE_DTYPE = np.dtype([("good_count", "<u4"), ("min_dist", "<u2"), ("n_train", "<u2")])
DMATCH_DTYPE = np.dtype([("query_idx", "<i4"), ("train_idx", "<i4"), ("img_idx", "<i4"), ("distance", "<f4")])
CANDIDATE_DTYPE = np.dtype([("current_frame_id", "<i4"), ("matched_frame_id", "<i4"), ("num_matches", "<i4"),
                            ("_pad", "<i4"), ("similarity_score", "<f8")])
L2_SCORE_DTYPE = np.dtype([("good_count", "<u4"), ("min_dist_sq", "<u4")])      # lcm_l2_score
EPI_RESULT_DTYPE = np.dtype([("E", "<f8", (9,)), ("n_points", "<i4"), ("n_inliers", "<i4"), ("best_iter", "<i4"),
                             ("status", "<i4")])                              # lcm_epi_result
assert EPI_RESULT_DTYPE.itemsize == C.sizeof(EpiResult) == 88 and C.sizeof(EpiParams) == 64
POSE_RESULT_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("counts", "<i4", (4,)), ("n_used", "<i4"), ("n_good", "<i4"),
                              ("choice", "<i4"), ("status", "<i4")])          # lcm_pose_result
assert POSE_RESULT_DTYPE.itemsize == C.sizeof(PoseResult) == 128 and C.sizeof(PoseParams) == 32
PGO_POSE_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,))])             # lcm_pgo_pose
PGO_EDGE_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("weight", "<f8"), ("from", "<i4"), ("to", "<i4")])    # lcm_pgo_edge
assert PGO_POSE_DTYPE.itemsize == 96 and PGO_EDGE_DTYPE.itemsize == 112 and C.sizeof(PgoParams) == 64 and C.sizeof(PgoInfo) == 48
BA_POINT_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8")])                                     # lcm_ba_point
BA_OBS_DTYPE = np.dtype([("cam", "<i4"), ("point", "<i4"), ("u", "<f8"), ("v", "<f8")])                     # lcm_ba_obs
BA_ELEM_INFO_DTYPE = np.dtype([("last_update", "<f8"), ("cost", "<f8"), ("iterations", "<i4"), ("status", "<i4")])    # lcm_ba_elem_info
assert BA_POINT_DTYPE.itemsize == 24 and BA_OBS_DTYPE.itemsize == 24 and BA_ELEM_INFO_DTYPE.itemsize == 24
assert C.sizeof(BaParams) == 112 and C.sizeof(BaInfo) == 184 and C.sizeof(BaMapReport) == 56
MAP_TRI_DTYPE = np.dtype([("X", "<f8", (3,)), ("depth1", "<f8"), ("depth2", "<f8"), ("cos_parallax", "<f8"), ("err1", "<f8"),
                          ("err2", "<f8")])                                    # lcm_map_tri
MAP_PAIR_INFO_DTYPE = np.dtype([("baseline", "<f8"), ("cos_min", "<f8"), ("counts", "<i4", (8,))])      # lcm_map_pair_info
assert MAP_TRI_DTYPE.itemsize == 64 and MAP_PAIR_INFO_DTYPE.itemsize == 48 and C.sizeof(MapParams) == 112 and C.sizeof(MapKeyframeReport) == 168
SIFT_KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("response", "<f4"), ("xi", "<f4"), ("octave", "<i2"),
                                ("layer", "<i2"), ("col", "<i4"), ("row", "<i4")])                        # lcm_sift_keypoint
SIFT_CANDIDATE_DTYPE = np.dtype([("octave", "<i4"), ("layer", "<i4"), ("row", "<i4"), ("col", "<i4")])     # lcm_sift_candidate
assert SIFT_KEYPOINT_DTYPE.itemsize == 32 and SIFT_CANDIDATE_DTYPE.itemsize == 16 and C.sizeof(SiftParams) == 64 and C.sizeof(SiftPlanInfo) == 320
LO_INFO_DTYPE = np.dtype([("seed_iter", "<i4"), ("round", "<i4"), ("n_inliers_ransac", "<i4"), ("status", "<i4")])    # lcm_lo_info
assert LO_INFO_DTYPE.itemsize == C.sizeof(LoInfo) == 16 and C.sizeof(LoParams) == 96
assert SCORE_DTYPE.itemsize == C.sizeof(Score) == 8
assert L2_SCORE_DTYPE.itemsize == 8
assert C.sizeof(PointPair) == 16          # returned as float32[n, 4]: (qx, qy, tx, ty)
assert DMATCH_DTYPE.itemsize == C.sizeof(DMatch) == 16
assert CANDIDATE_DTYPE.itemsize == C.sizeof(LoopCandidate) == 24

_lib = None

_u8p = C.POINTER(C.c_uint8)
_i32p = C.POINTER(C.c_int32)
_vp = C.c_void_p
# a map as the lcm_ba_* calls take it: handle, poses, valid, n_poses, points, n_points, obs, n_obs, params
_BA_MAP = [_vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int, C.POINTER(BaParams)]

# name -> (restype, argtypes); mirrors include/lcm.h one to one (tests/test_abi.py checks the symbol list)
_SIGNATURES = {
    "lcm_params_default": (None, [C.POINTER(Params)]),
    "lcm_last_error": (C.c_char_p, []),
    "lcm_backend_name": (C.c_char_p, []),
    "lcm_device_count": (C.c_int, []),
    "lcm_create": (C.c_int, [C.POINTER(Params), C.c_int, _vp, C.POINTER(_vp)]),
    "lcm_destroy": (None, [_vp]),
    "lcm_set_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "lcm_get_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "lcm_sync": (C.c_int, [_vp]),
    "lcm_db_reserve": (C.c_int, [_vp, C.c_int, C.c_int]),
    "lcm_db_append": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int]),
    "lcm_db_append_device": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int]),
    "lcm_db_size": (C.c_int, [_vp]),
    "lcm_db_clear": (C.c_int, [_vp]),
    "lcm_db_truncate": (C.c_int, [_vp, C.c_int]),
    "lcm_db_frame_info": (C.c_int, [_vp, C.c_int, _i32p, _i32p, _i32p]),
    "lcm_db_read": (C.c_int, [_vp, C.c_int, _vp, C.c_int]),
    "lcm_db_save": (C.c_int, [_vp, C.c_char_p]),
    "lcm_db_load": (C.c_int, [_vp, C.c_char_p]),
    "lcm_match_pair": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _i32p]),
    "lcm_match_features": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, _i32p, _i32p]),
    "lcm_match_stored": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int, _i32p, _i32p]),
    "lcm_match_stored_batch": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_size_t, _vp, _vp]),
    "lcm_match_query_batch": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, C.c_size_t, _vp, _vp]),
    "lcm_knn2_pair": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _i32p]),
    "lcm_match_features_ratio": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_double, _vp, _i32p]),
    "lcm_match_stored_ratio": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, _vp, C.c_int, _i32p]),
    "lcm_match_stored_batch_ratio": (C.c_int, [_vp, _vp, C.c_int, C.c_double, _vp, C.c_size_t, _vp]),
    "lcm_match_query_batch_ratio": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_double, _vp, C.c_size_t, _vp]),
    "lcm_sift_pack_f32": (C.c_int, [_vp, C.c_int, _vp]),
    "lcm_knn2_pair_l2": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _i32p]),
    "lcm_match_features_ratio_l2": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_double, _vp, _i32p]),
    "lcm_match_pairs_ratio_l2": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, C.c_int, C.c_double, _vp, C.c_size_t, _vp]),
    "lcm_score_pairs_ratio_l2": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, C.c_int, C.c_double, _vp]),
    "lcm_loop_search_ratio_l2": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, C.c_int, C.POINTER(RatioLoopParams), _vp, C.c_size_t,
                                            C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "lcm_l2_ratio_test_device": (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_double, _vp]),
    "lcm_l2_db_append": (C.c_int, [_vp, _vp, C.c_int, _i32p]),
    "lcm_l2_db_size": (C.c_int, [_vp]),
    "lcm_l2_db_rows": (C.c_int, [_vp, C.c_int, _i32p]),
    "lcm_l2_db_read": (C.c_int, [_vp, C.c_int, _vp, C.c_int]),
    "lcm_l2_db_truncate": (C.c_int, [_vp, C.c_int]),
    "lcm_l2_db_clear": (C.c_int, [_vp]),
    "lcm_l2_db_info_read": (C.c_int, [_vp, C.POINTER(L2DbInfo)]),
    "lcm_l2_db_score_pairs": (C.c_int, [_vp, _vp, C.c_int, C.c_double, _vp]),
    "lcm_l2_db_match_pairs_ratio": (C.c_int, [_vp, _vp, C.c_int, C.c_double, _vp, C.c_size_t, _vp]),
    "lcm_l2_db_loop_search": (C.c_int, [_vp, _vp, C.c_int, C.POINTER(RatioLoopParams), _vp, C.c_size_t, C.POINTER(C.c_size_t),
                                         C.POINTER(C.c_size_t)]),
    "lcm_l2_db_detect_loops": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _vp, C.c_int, C.POINTER(RatioLoopParams), _vp, C.c_size_t,
                                          C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "lcm_l2_db_append_kp": (C.c_int, [_vp, _vp, _vp, C.c_int, _i32p]),
    "lcm_l2_db_read_kp": (C.c_int, [_vp, C.c_int, _vp, C.c_int]),
    "lcm_l2_db_match_points": (C.c_int, [_vp, _vp, C.c_int, C.c_double, _vp, _vp, C.c_size_t, _vp]),
    "lcm_l2_db_detect_loops_points": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, C.POINTER(RatioLoopParams), _vp,
                                                 C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), _vp, _vp, C.c_size_t, _vp]),
    "lcm_epi_params_default": (None, [C.POINTER(EpiParams)]),
    "lcm_epi_loop_test": (C.c_int, [C.POINTER(EpiResult), C.POINTER(EpiParams)]),
    "lcm_epi_verify_pairs": (C.c_int, [_vp, _vp, _vp, C.c_int, C.POINTER(EpiParams), _vp, _vp]),
    "lcm_epi_hypotheses": (C.c_int, [_vp, _vp, C.c_int, C.c_uint32, C.POINTER(EpiParams), _vp, _vp]),
    "lcm_epi_score_models": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.POINTER(EpiParams), _vp]),
    "lcm_epi_db_verify_pairs": (C.c_int, [_vp, _vp, C.c_int, C.c_double, C.POINTER(EpiParams), _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "lcm_epi_db_detect_loops": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, C.POINTER(RatioLoopParams),
                                           C.POINTER(EpiParams), _vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                           _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "lcm_lo_params_default": (None, [C.POINTER(LoParams)]),
    "lcm_lo_verify_pairs": (C.c_int, [_vp, _vp, _vp, C.c_int, C.POINTER(EpiParams), C.POINTER(LoParams), _vp, _vp, _vp]),
    "lcm_lo_select": (C.c_int, [_vp, _vp, C.c_int, _vp]),
    "lcm_lo_refit_models": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_double, C.POINTER(EpiParams), _vp, _vp, _vp]),
    "lcm_lo_db_verify_pairs": (C.c_int, [_vp, _vp, C.c_int, C.c_double, C.POINTER(EpiParams), C.POINTER(LoParams),
                                          C.POINTER(PoseParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "lcm_lo_db_detect_loops": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, C.POINTER(RatioLoopParams),
                                          C.POINTER(EpiParams), C.POINTER(LoParams), C.POINTER(PoseParams), _vp, C.c_size_t,
                                          C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                          C.c_size_t, _vp, C.c_int, _i32p]),
    "lcm_pose_params_default": (None, [C.POINTER(PoseParams)]),
    "lcm_pose_loop_test": (C.c_int, [C.POINTER(EpiResult), C.POINTER(PoseResult), C.POINTER(EpiParams), C.POINTER(PoseParams)]),
    "lcm_pose_best": (C.c_int, [_vp, _vp, C.c_int, C.POINTER(EpiParams), C.POINTER(PoseParams), C.c_int, _i32p]),
    "lcm_pose_recover_pairs": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, C.POINTER(EpiParams), C.POINTER(PoseParams), _vp, _vp]),
    "lcm_pose_candidates": (C.c_int, [_vp, _vp, C.c_int, _vp, _vp, _vp]),
    "lcm_pose_db_verify_pairs": (C.c_int, [_vp, _vp, C.c_int, C.c_double, C.POINTER(EpiParams), C.POINTER(PoseParams), _vp, _vp, _vp,
                                            _vp, _vp, _vp, C.c_size_t, _vp]),
    "lcm_pose_db_detect_loops": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, C.POINTER(RatioLoopParams),
                                            C.POINTER(EpiParams), C.POINTER(PoseParams), _vp, C.c_size_t, C.POINTER(C.c_size_t),
                                            C.POINTER(C.c_size_t), _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, C.c_int, _i32p]),
    "lcm_pgo_params_default": (None, [C.POINTER(PgoParams)]),
    "lcm_pgo_optimize": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, C.c_int, C.POINTER(PgoParams), _vp, C.POINTER(PgoInfo)]),
    "lcm_pgo_step": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, C.c_int, C.POINTER(PgoParams), _vp, _vp, _vp, _vp, C.POINTER(PgoInfo)]),
    "lcm_pgo_build_graph": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.POINTER(PgoParams), _vp, C.c_int, _i32p]),
    "lcm_pgo_rotation_drift": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, C.POINTER(C.c_double)]),
    "lcm_pgo_linear_correct": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    "lcm_pgo_close_loop": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.POINTER(PoseResult), C.POINTER(PgoParams), _vp,
                                      C.POINTER(PgoInfo)]),
    "lcm_ba_params_default": (None, [C.POINTER(BaParams)]),
    "lcm_ba_error": (C.c_int, _BA_MAP + [C.POINTER(C.c_double), _vp]),
    "lcm_ba_refine_cameras": (C.c_int, _BA_MAP + [_vp, _vp]),
    "lcm_ba_refine_points": (C.c_int, _BA_MAP + [_vp, _vp]),
    "lcm_ba_step_cameras": (C.c_int, _BA_MAP + [_vp, _vp, _vp, _vp, _vp, _vp]),
    "lcm_ba_step_points": (C.c_int, _BA_MAP + [_vp, _vp, _vp, _vp, _vp, _vp]),
    "lcm_ba_optimize": (C.c_int, _BA_MAP + [_vp, _vp, _vp, _vp, C.POINTER(BaInfo)]),
    "lcm_ba_outliers": (C.c_int, _BA_MAP + [_vp, _vp, C.POINTER(C.c_double), _i32p]),
    "lcm_ba_compact": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, _vp, _i32p, _i32p]),
    "lcm_ba_add_loop_observations": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int,
                                                C.c_int, _i32p]),
    "lcm_ba_refine_map": (C.c_int, _BA_MAP + [C.c_int, _vp, _vp, _vp, _vp, C.POINTER(BaMapReport)]),
    "lcm_map_params_default": (None, [C.POINTER(MapParams)]),
    "lcm_map_median_displacement": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp]),
    "lcm_map_triangulate_pairs": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.POINTER(MapParams), _vp, _vp, _vp]),
    "lcm_map_merge": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, _vp,
                                 C.c_int, _vp, _i32p, _i32p]),
    "lcm_map_add_keyframe": (C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.POINTER(MapParams),
                                        C.POINTER(EpiParams), C.POINTER(LoParams), C.POINTER(PoseParams), _vp, C.c_int, _vp, C.c_int, _vp,
                                        C.POINTER(MapKeyframeReport)]),
    "lcm_map_db_track": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, C.POINTER(EpiParams), C.POINTER(LoParams), C.POINTER(PoseParams), _vp, _vp,
                                    _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, C.POINTER(MapParams),
                                    _vp, C.c_int, _vp, C.c_int, _vp, C.POINTER(MapKeyframeReport)]),
    "lcm_sift_params_default": (None, [C.POINTER(SiftParams)]),
    "lcm_sift_plan": (C.c_int, [C.c_int, C.c_int, C.POINTER(SiftParams), C.POINTER(SiftPlanInfo)]),
    "lcm_sift_plan_read": (C.c_int, [C.c_int, C.c_int, C.POINTER(SiftParams), C.c_int, _vp, C.c_int, C.POINTER(C.c_int)]),
    "lcm_sift_space_create": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(SiftParams), C.POINTER(_vp)]),
    "lcm_sift_space_destroy": (None, [_vp]),
    "lcm_sift_space_build": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_size_t]),
    "lcm_sift_space_info": (C.c_int, [_vp, C.POINTER(SiftSpaceInfo)]),
    "lcm_sift_space_read": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp]),
    "lcm_sift_space_write": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp]),
    "lcm_sift_extrema": (C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "lcm_sift_detect": (C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "lcm_sift_detect_image": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_size_t, C.POINTER(SiftParams), _vp, C.c_size_t, C.POINTER(C.c_size_t)]),
    "lcm_query_scores": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, _vp, _i32p]),
    "lcm_query_submit": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _i32p]),
    "lcm_query_collect": (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int, _i32p]),
    "lcm_query_submit_batch": (C.c_int, [_vp, _vp, _i32p, _i32p, C.c_int, _i32p]),
    "lcm_query_collect_batch": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, C.POINTER(C.c_size_t), _vp]),
    "lcm_online_stats_read": (C.c_int, [_vp, C.POINTER(OnlineStats), C.c_int]),
    "lcm_detect_loops": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, _i32p]),
    "lcm_loop_test": (C.c_int, [C.POINTER(Params), C.POINTER(Score), C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "lcm_all_vs_all": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, C.c_size_t,
                                  C.POINTER(C.c_size_t), _vp]),
    "lcm_all_vs_all_argmin": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, C.c_size_t, _vp,
                                         C.POINTER(C.c_size_t), _vp]),
    "lcm_all_vs_all_loops": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, C.c_size_t,
                                        C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "lcm_all_vs_all_ratio": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_double, _vp, C.c_size_t,
                                        C.POINTER(C.c_size_t), _vp]),
    "lcm_query_scores_ratio": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_double, _vp, _vp, _i32p]),
    "lcm_ratio_loop_params_default": (None, [C.POINTER(RatioLoopParams)]),
    "lcm_ratio_loop_test": (C.c_int, [C.POINTER(RatioLoopParams), C.POINTER(Score), C.c_int, C.POINTER(C.c_double)]),
    "lcm_all_vs_all_loops_ratio": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.POINTER(RatioLoopParams), _vp,
                                              C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "lcm_detect_loops_ratio": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.POINTER(RatioLoopParams), _vp, C.c_int, _i32p]),
    "lcm_last_launch_info": (C.c_int, [_vp, C.POINTER(LaunchInfo)]),
    "lcm_last_bulk_scores": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "lcm_set_kernel_variant": (C.c_int, [_vp, C.c_int]),
    "lcm_set_tuning": (C.c_int, [_vp, C.c_int, C.c_int]),
    "lcm_group_create": (C.c_int, [C.POINTER(Params), C.c_int, _i32p, C.POINTER(_vp)]),
    "lcm_group_create_loopback": (C.c_int, [C.POINTER(Params), C.c_int, C.c_int, C.POINTER(_vp)]),
    "lcm_group_create_peer": (C.c_int, [C.POINTER(Params), C.c_int, _i32p, C.POINTER(_vp)]),
    "lcm_group_transport": (C.c_char_p, [_vp]),
    "lcm_group_destroy": (None, [_vp]),
    "lcm_group_size": (C.c_int, [_vp]),
    "lcm_group_db_size": (C.c_int, [_vp]),
    "lcm_group_handle": (C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    "lcm_group_set_params": (C.c_int, [_vp, C.POINTER(Params)]),
    "lcm_group_reserve": (C.c_int, [_vp, C.c_int, C.c_int]),
    "lcm_group_append": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int]),
    "lcm_group_clear": (C.c_int, [_vp]),
    "lcm_group_truncate": (C.c_int, [_vp, C.c_int]),
    "lcm_group_save": (C.c_int, [_vp, C.c_char_p]),
    "lcm_group_load": (C.c_int, [_vp, C.c_char_p]),
    "lcm_group_sync": (C.c_int, [_vp]),
    "lcm_group_set_tuning": (C.c_int, [_vp, C.c_int, C.c_int]),
    "lcm_group_set_kernel_variant": (C.c_int, [_vp, C.c_int]),
    "lcm_group_all_vs_all": (C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(C.c_size_t), _vp]),
    "lcm_group_all_vs_all_argmin": (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.POINTER(C.c_size_t), _vp]),
    "lcm_group_all_vs_all_loops": (C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "lcm_group_all_vs_all_ratio": (C.c_int, [_vp, C.c_double, _vp, C.c_size_t, C.POINTER(C.c_size_t), _vp]),
    "lcm_group_all_vs_all_loops_ratio": (C.c_int, [_vp, C.POINTER(RatioLoopParams), _vp, C.c_size_t, C.POINTER(C.c_size_t),
                                                    C.POINTER(C.c_size_t)]),
    "lcm_group_query_submit_batch": (C.c_int, [_vp, _vp, _i32p, _i32p, C.c_int, _i32p]),
    "lcm_group_query_collect_batch": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, C.POINTER(C.c_size_t), _vp]),
    "lcm_group_online_stats_read": (C.c_int, [_vp, C.POINTER(OnlineStats), C.c_int]),
    "lcm_group_last_info": (C.c_int, [_vp, C.POINTER(GroupInfo)]),
    "lcm_group_query_scores": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _vp, _vp, C.c_int, _i32p]),
    "lcm_group_query_scores_batch": (C.c_int, [_vp, _vp, _i32p, _i32p, C.c_int, _vp, C.c_size_t, C.POINTER(C.c_size_t), _vp]),
    "lcm_group_detect_loops": (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_int, _i32p]),
    "lcm_merge_shard_scores": (C.c_int, [_vp, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_size_t,
                                          C.POINTER(C.c_size_t), _vp]),
    "lcm_merge_shard_scores_device": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_size_t,
                                                 C.POINTER(C.c_size_t)]),
    "lcm_dev_alloc": (C.c_int, [_vp, C.c_size_t, C.POINTER(_vp)]),
    "lcm_dev_free": (C.c_int, [_vp, _vp]),
    "lcm_dev_upload": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
    "lcm_dev_download": (C.c_int, [_vp, _vp, _vp, C.c_size_t]),
}


def load_library(path: Optional[str] = None):
    """dlopen the C-ABI library.  Raises OSError if it has not been built (run __graft_entry__.build())."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise OSError(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(there is no CPU fallback)")
    lib = C.CDLL(p, mode=C.RTLD_GLOBAL)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def _check(rc: int):
    if rc != 0:
        raise LcmError(rc, load_library().lcm_last_error().decode("utf-8", "replace"))


def default_params() -> Params:
    p = Params()
    load_library().lcm_params_default(C.byref(p))
    return p


def default_ratio_loop_params() -> RatioLoopParams:
    p = RatioLoopParams()
    load_library().lcm_ratio_loop_params_default(C.byref(p))
    return p


def default_epi_params(fx: float = 0.0, fy: float = 0.0, cx: float = 0.0, cy: float = 0.0, **over) -> EpiParams:
    """lcm_epi_params_default (threshold 1.0, iters 1024, min_inliers 200, min_ratio 0.6, seed 0) with the camera matrix and
    any other field given by name.  The defaults leave K zero: a call with fx <= 0 or fy <= 0 is refused."""
    p = EpiParams()
    load_library().lcm_epi_params_default(C.byref(p))
    p.fx, p.fy, p.cx, p.cy = fx, fy, cx, cy
    for k, v in over.items():
        if k not in ("threshold", "min_ratio", "iters", "min_inliers", "seed"):
            raise TypeError(f"lcm_epi_params has no field {k!r}")
        setattr(p, k, v)
    return p


def epi_loop_test(result, ep: EpiParams) -> bool:
    """lcm_epi_loop_test (host only): n_inliers > min_inliers and n_inliers / n_points > min_ratio, both strict.  result: an
    EPI_RESULT_DTYPE record or an EpiResult."""
    if not isinstance(result, EpiResult):
        r = EpiResult()
        r.n_points, r.n_inliers, r.best_iter, r.status = (int(result[k]) for k in ("n_points", "n_inliers", "best_iter", "status"))
        result = r
    return bool(load_library().lcm_epi_loop_test(C.byref(result), C.byref(ep)))


def default_lo_params(rounds: Optional[int] = None, mult: Optional[Sequence[float]] = None) -> LoParams:
    """lcm_lo_params_default (4 rounds, multipliers 3, 2, 1.5, 1; 64 seeds) with the rounds and / or multipliers given."""
    p = LoParams()
    load_library().lcm_lo_params_default(C.byref(p))
    if mult is not None:
        for r, m in enumerate(mult):
            p.mult[r] = float(m)
        p.rounds = len(mult)
    if rounds is not None:
        p.rounds = int(rounds)
    return p


def default_pose_params(**over) -> PoseParams:
    """lcm_pose_params_default (max_depth 50.0, min_pose_inliers 100) with any field given by name."""
    p = PoseParams()
    load_library().lcm_pose_params_default(C.byref(p))
    for k, v in over.items():
        if k not in ("max_depth", "min_pose_inliers"):
            raise TypeError(f"lcm_pose_params has no field {k!r}")
        setattr(p, k, v)
    return p


def _pose_result(result) -> PoseResult:
    if isinstance(result, PoseResult):
        return result
    r = PoseResult()
    r.n_used, r.n_good, r.choice, r.status = (int(result[k]) for k in ("n_used", "n_good", "choice", "status"))
    return r


def pose_loop_test(epi_result, pose_result, ep: EpiParams, pp: Optional[PoseParams] = None) -> bool:
    """lcm_pose_loop_test (host only): epi_loop_test and n_good > min_pose_inliers, strict.  The results: records of
    EPI_RESULT_DTYPE / POSE_RESULT_DTYPE or the ctypes structures."""
    if not isinstance(epi_result, EpiResult):
        r = EpiResult()
        r.n_points, r.n_inliers, r.best_iter, r.status = (int(epi_result[k]) for k in ("n_points", "n_inliers", "best_iter", "status"))
        epi_result = r
    pr = _pose_result(pose_result)
    return bool(load_library().lcm_pose_loop_test(C.byref(epi_result), C.byref(pr), C.byref(ep), None if pp is None else C.byref(pp)))


def pose_best(epi_results, pose_results, ep: EpiParams, pp: Optional[PoseParams] = None, floor_inliers: int = -1) -> int:
    """lcm_pose_best (host only) over EPI_RESULT_DTYPE[n] and POSE_RESULT_DTYPE[n]: the index of the best loop among the
    candidates with more than floor_inliers inliers, or -1."""
    er = np.ascontiguousarray(epi_results, EPI_RESULT_DTYPE)
    pr = np.ascontiguousarray(pose_results, POSE_RESULT_DTYPE)
    assert len(er) == len(pr)
    best = C.c_int32(-2)
    _check(load_library().lcm_pose_best(er.ctypes.data_as(_vp), pr.ctypes.data_as(_vp), len(er), C.byref(ep),
                                        None if pp is None else C.byref(pp), floor_inliers, C.byref(best)))
    return best.value


def default_pgo_params(**over) -> PgoParams:
    """lcm_pgo_params_default (eps 1e-6, damping 1e-4, min_update 1e-6, loop_weight 10, max_iters 20, loop_direction 0) with any
    field given by name."""
    p = PgoParams()
    load_library().lcm_pgo_params_default(C.byref(p))
    for k, v in over.items():
        if k not in ("eps", "damping", "min_update", "loop_weight", "max_iters", "loop_direction"):
            raise TypeError(f"lcm_pgo_params has no field {k!r}")
        setattr(p, k, v)
    return p


def pgo_poses(R, t) -> np.ndarray:
    """PGO_POSE_DTYPE[n] from rotations [n, 3, 3] and translations [n, 3]."""
    R = np.asarray(R, np.float64)
    out = np.zeros(len(R), PGO_POSE_DTYPE)
    out["R"] = R.reshape(len(R), 9)
    out["t"] = np.asarray(t, np.float64).reshape(len(R), 3)
    return out


def pgo_edges(R, t, weight, ends) -> np.ndarray:
    """PGO_EDGE_DTYPE[n] from rotations [n, 3, 3], translations [n, 3], weights [n] and (from, to) pairs [n, 2]."""
    R = np.asarray(R, np.float64)
    out = np.zeros(len(R), PGO_EDGE_DTYPE)
    out["R"] = R.reshape(len(R), 9)
    out["t"] = np.asarray(t, np.float64).reshape(len(R), 3)
    out["weight"] = weight
    ends = np.asarray(ends, np.int32).reshape(len(R), 2)
    out["from"], out["to"] = ends[:, 0], ends[:, 1]
    return out


def _pgo_graph(poses, valid):
    p = np.ascontiguousarray(poses, PGO_POSE_DTYPE)
    v = None if valid is None else np.ascontiguousarray(valid, np.uint8)
    assert v is None or len(v) == len(p)
    return p, v


def pgo_build_graph(poses, past: int, curr: int, R_loop, t_loop, pp: Optional[PgoParams] = None, valid=None) -> np.ndarray:
    """lcm_pgo_build_graph (host only): the sequential edges of the valid poses and the loop edge past -> curr, PGO_EDGE_DTYPE[n]."""
    p, v = _pgo_graph(poses, valid)
    Rl, tl = np.ascontiguousarray(R_loop, np.float64).reshape(9), np.ascontiguousarray(t_loop, np.float64).reshape(3)
    out = np.zeros(max(len(p), 1), PGO_EDGE_DTYPE)
    n = C.c_int32(0)
    _check(load_library().lcm_pgo_build_graph(_ptr(p), _ptr(v), len(p), past, curr, _ptr(Rl), _ptr(tl), _ref(pp), _ptr(out), len(out),
                                              C.byref(n)))
    return out[:n.value]


def pgo_rotation_drift(poses, past: int, curr: int, R_loop) -> float:
    """lcm_pgo_rotation_drift (host only): |log(R_loop (R_curr R_past^T)^T)| in radians."""
    p, _ = _pgo_graph(poses, None)
    Rl = np.ascontiguousarray(R_loop, np.float64).reshape(9)
    angle = C.c_double(-1.0)
    _check(load_library().lcm_pgo_rotation_drift(_ptr(p), len(p), past, curr, _ptr(Rl), C.byref(angle)))
    return angle.value


def pgo_linear_correct(poses, past: int, curr: int, R_loop, valid=None) -> np.ndarray:
    """lcm_pgo_linear_correct (host only): the reference's simplePoseCorrection, PGO_POSE_DTYPE[n]."""
    p, v = _pgo_graph(poses, valid)
    Rl = np.ascontiguousarray(R_loop, np.float64).reshape(9)
    out = np.zeros(max(len(p), 1), PGO_POSE_DTYPE)
    _check(load_library().lcm_pgo_linear_correct(_ptr(p), _ptr(v), len(p), past, curr, _ptr(Rl), _ptr(out)))
    return out[:len(p)]


_BA_FIELDS = ("fx", "fy", "cx", "cy", "eps", "damping", "min_update", "outlier_px", "min_spread", "spread_factor", "outer_iters",
              "inner_iters", "min_cam_obs", "min_point_obs")


def default_ba_params(**over) -> BaParams:
    """lcm_ba_params_default (K zero, eps 1e-6, damping 1e-3, min_update 1e-6, outlier_px 5, min_spread 10, spread_factor 5,
    outer_iters 5, inner_iters 5, min_cam_obs 10, min_point_obs 2) with any field given by name."""
    p = BaParams()
    load_library().lcm_ba_params_default(C.byref(p))
    for k, v in over.items():
        if k not in _BA_FIELDS:
            raise TypeError(f"lcm_ba_params has no field {k!r}")
        setattr(p, k, v)
    return p


def ba_points(X) -> np.ndarray:
    """BA_POINT_DTYPE[n] from coordinates [n, 3]."""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    out = np.zeros(len(X), BA_POINT_DTYPE)
    out["x"], out["y"], out["z"] = X[:, 0], X[:, 1], X[:, 2]
    return out


def ba_xyz(points) -> np.ndarray:
    """float64[n, 3] from BA_POINT_DTYPE[n]."""
    p = np.ascontiguousarray(points, BA_POINT_DTYPE)
    return np.stack([p["x"], p["y"], p["z"]], 1) if len(p) else np.zeros((0, 3))


def ba_obs(cam, point, uv) -> np.ndarray:
    """BA_OBS_DTYPE[n] from camera indices [n], point indices [n] and pixels [n, 2]."""
    cam = np.asarray(cam, np.int32)
    out = np.zeros(len(cam), BA_OBS_DTYPE)
    uv = np.asarray(uv, np.float64).reshape(len(cam), 2)
    out["cam"], out["point"], out["u"], out["v"] = cam, np.asarray(point, np.int32), uv[:, 0], uv[:, 1]
    return out


def _ba_map(poses, valid, points, obs):
    p, v = _pgo_graph(poses, valid)
    return p, v, np.ascontiguousarray(points, BA_POINT_DTYPE), np.ascontiguousarray(obs, BA_OBS_DTYPE)


def ba_compact(points, obs, flags):
    """lcm_ba_compact (host only): (BA_POINT_DTYPE[kept], BA_OBS_DTYPE[kept observations], old_to_new int32[n])."""
    x, o = np.ascontiguousarray(points, BA_POINT_DTYPE), np.ascontiguousarray(obs, BA_OBS_DTYPE)
    f = np.ascontiguousarray(flags, np.uint8)
    assert len(f) == len(x)
    xo, oo, table = np.zeros(max(len(x), 1), BA_POINT_DTYPE), np.zeros(max(len(o), 1), BA_OBS_DTYPE), np.zeros(max(len(x), 1), np.int32)
    np_, no = C.c_int32(0), C.c_int32(0)
    _check(load_library().lcm_ba_compact(_ptr(x), len(x), _ptr(o), len(o), _ptr(f), _ptr(xo), len(x), _ptr(oo), len(o), _ptr(table),
                                         C.byref(np_), C.byref(no)))
    return xo[:np_.value], oo[:no.value], table[:len(x)]


def ba_add_loop_observations(matches, mask, past_table, curr_table, curr_kp, curr: int, n_points: int, obs):
    """lcm_ba_add_loop_observations (host only): the observation list with the loop's new observations appended (BA_OBS_DTYPE) and
    their number; curr_table (int32[n_curr_kp], C-contiguous) is updated in place."""
    m = np.ascontiguousarray(matches, DMATCH_DTYPE)
    k = np.ascontiguousarray(mask, np.uint8)
    assert len(k) == len(m) and curr_table.dtype == np.int32 and curr_table.flags["C_CONTIGUOUS"]
    past = np.ascontiguousarray(past_table, np.int32)
    kp = np.ascontiguousarray(curr_kp, np.float32).reshape(-1, 2)
    assert len(kp) == len(curr_table)
    o = np.ascontiguousarray(obs, BA_OBS_DTYPE)
    out = np.zeros(len(o) + int(np.count_nonzero(k)) + 1, BA_OBS_DTYPE)
    out[:len(o)] = o
    n = C.c_int32(0)
    _check(load_library().lcm_ba_add_loop_observations(_ptr(m), _ptr(k), len(m), _ptr(past), len(past), _ptr(curr_table), _ptr(kp), len(kp),
                                                       curr, n_points, _ptr(out), len(o), len(out), C.byref(n)))
    return out[:len(o) + n.value], n.value


def default_map_params(**over) -> MapParams:
    """lcm_map_params_default (K zero, min_parallax_deg 1, max_reproj 4, min_depth 0.1, max_depth 50, min_displacement 20,
    max_displacement 150, min_inlier_ratio 0.3, min_tracked 100, min_inliers 50, min_pose_inliers 10) with any field given by name."""
    p = MapParams()
    load_library().lcm_map_params_default(C.byref(p))
    for k, v in over.items():
        if k not in _MAP_FIELDS:
            raise TypeError(f"lcm_map_params has no field {k!r}")
        setattr(p, k, v)
    return p


def default_sift_params(**over) -> SiftParams:
    """lcm_sift_params_default (contrast 0.04, edge 10, sigma 1.6, init_sigma 0.5, 3 layers, upsample, derived octaves, border 5, 5 steps),
    then the given fields."""
    p = SiftParams()
    load_library().lcm_sift_params_default(C.byref(p))
    for k, v in over.items():
        if k not in _SIFT_FIELDS:
            raise TypeError(f"lcm_sift_params has no field {k!r}")
        setattr(p, k, v)
    return p


def sift_plan(w: int, h: int, sp: Optional[SiftParams] = None) -> SiftPlanInfo:
    """lcm_sift_plan: host only, no device needed."""
    out = SiftPlanInfo()
    _check(load_library().lcm_sift_plan(w, h, _ref(sp), C.byref(out)))
    return out


def sift_plan_taps(w: int, h: int, layer: int, sp: Optional[SiftParams] = None) -> np.ndarray:
    """lcm_sift_plan_read: the float taps of Gaussian layer `layer` (-1: the first blur)."""
    taps, n = np.zeros(2 * SIFT_MAX_RADIUS + 1, np.float32), C.c_int(0)
    _check(load_library().lcm_sift_plan_read(w, h, _ref(sp), layer, _ptr(taps), len(taps), C.byref(n)))
    return taps[:n.value].copy()


def _gray(img) -> np.ndarray:
    """A uint8 gray image whose rows are contiguous (a row stride above the width is kept)."""
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 2 or a.strides[1] != 1 or a.strides[0] < a.shape[1]:
        a = np.ascontiguousarray(a, np.uint8)
    assert a.ndim == 2
    return a


def _point_pairs(pts) -> np.ndarray:
    p = np.ascontiguousarray(pts, dtype=np.float32)
    if p.ndim != 2 or p.shape[1] != 4:
        raise ValueError(f"point pairs must be (n, 4) float32 (qx, qy, tx, ty), got {p.shape}")
    return p


def _ratio_loop_params(ratio, min_rows, min_matches) -> Optional[RatioLoopParams]:
    """None (the library's defaults: rp == NULL) when all three are None, else a structure with the given values over
    the defaults."""
    if ratio is None and min_rows is None and min_matches is None:
        return None
    p = default_ratio_loop_params()
    if ratio is not None:
        p.ratio = ratio
    if min_rows is not None:
        p.min_rows = min_rows
    if min_matches is not None:
        p.min_matches = min_matches
    return p


def ratio_loop_test(score, rows_query: int, ratio: Optional[float] = None, min_rows: Optional[int] = None,
                    min_matches: Optional[int] = None) -> Tuple[bool, float]:
    """lcm_ratio_loop_test (host-only, no device needed): (is a loop candidate, similarity) of one shipped record; the
    stored frame's row count is the record's n_train.  Parameters left at None: 0.7 / 100 / 300."""
    s = Score(int(score["good_count"]), int(score["min_dist"]), int(score["n_train"]))
    p = _ratio_loop_params(ratio, min_rows, min_matches)
    sim = C.c_double(0)
    r = load_library().lcm_ratio_loop_test(None if p is None else C.byref(p), C.byref(s), rows_query, C.byref(sim))
    return bool(r), sim.value


def _rows(a) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim != 2 or a.shape[1] != DESC_BYTES:
        raise ValueError(f"descriptor matrix must be (n, {DESC_BYTES}) uint8, got {a.shape}")
    return a


def _ptr(a: Optional[np.ndarray]):
    return None if a is None or a.size == 0 else a.ctypes.data_as(_vp)


def _ref(p: Optional[C.Structure]):
    return None if p is None else C.byref(p)


def _buffer(a: Optional[np.ndarray], dtype, rows: int, *tail, contiguous: bool = False) -> np.ndarray:
    """The caller's buffer a, checked (dtype, room for `rows` rows; row shape and layout where the call depends on them), or a
    new one of at least one row."""
    if a is None:
        return np.zeros((max(rows, 1), *tail), dtype)
    assert a.dtype == dtype and len(a) >= rows and (not contiguous or a.flags["C_CONTIGUOUS"]) and (not tail or a.shape[1:] == tail)
    return a


def _sift_rows(a) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype != np.uint8:
        raise ValueError(f"SIFT rows must be uint8 (sift_pack_f32 converts CV_32F rows), got {a.dtype}")
    a = np.ascontiguousarray(a)
    if a.ndim != 2 or a.shape[1] != SIFT_BYTES:
        raise ValueError(f"SIFT matrix must be (n, {SIFT_BYTES}) uint8, got {a.shape}")
    return a


def sift_pack_f32(rows) -> np.ndarray:
    """lcm_sift_pack_f32 (host only, no device needed): CV_32F SIFT rows (n, 128) -> uint8 (n, 128).  LcmError
    (ERR_INVALID_ARG) if any value is not an integer in [0, 255]."""
    a = np.asarray(rows)
    if a.dtype != np.float32:
        raise ValueError(f"expected float32 rows, got {a.dtype}")
    a = np.ascontiguousarray(a)
    if a.ndim != 2 or a.shape[1] != SIFT_BYTES:
        raise ValueError(f"SIFT matrix must be (n, {SIFT_BYTES}) float32, got {a.shape}")
    out = np.zeros(a.shape, np.uint8)
    _check(load_library().lcm_sift_pack_f32(_ptr(a), a.shape[0], _ptr(out)))
    return out


class Matcher:
    """One matcher handle bound to one HIP device (one process per GPU).

    `stream` is a hipStream_t handle as an int (e.g. `torch.cuda.Stream(...).cuda_stream`); None or 0 (the legacy default
    stream's handle) makes the library create its own non-blocking stream.  When results are consumed by another
    framework on the device (torch.distributed collectives on the buffers lcm_all_vs_all filled), pass that framework's
    CURRENT stream — an explicit one — so its work is ordered after the kernels; see bench.py."""

    def __init__(self, params: Optional[Params] = None, device: int = 0, stream: Optional[int] = None):
        self._lib = load_library()
        self._h = _vp()
        p = params if params is not None else default_params()
        _check(self._lib.lcm_create(C.byref(p), device, _vp(stream) if stream else None, C.byref(self._h)))

    # -- lifetime ----------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.lcm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- parameters --------------------------------------------------------------------------------
    @property
    def params(self) -> Params:
        p = Params()
        _check(self._lib.lcm_get_params(self._h, C.byref(p)))
        return p

    def set_params(self, **kw):
        p = self.params
        for k, v in kw.items():
            setattr(p, k, v)
        _check(self._lib.lcm_set_params(self._h, C.byref(p)))

    def set_kernel_variant(self, v: int):
        _check(self._lib.lcm_set_kernel_variant(self._h, v))

    def set_tuning(self, knob: int, value: int):
        _check(self._lib.lcm_set_tuning(self._h, knob, value))

    def sync(self):
        _check(self._lib.lcm_sync(self._h))

    # -- database ----------------------------------------------------------------------------------
    def reserve(self, n_frames: int, max_desc: int):
        _check(self._lib.lcm_db_reserve(self._h, n_frames, max_desc))

    def append(self, frame_id: int, desc, n_keypoints: int = -1):
        d = _rows(desc)
        _check(self._lib.lcm_db_append(self._h, frame_id, _ptr(d), d.shape[0], n_keypoints))

    def append_device(self, frame_id: int, d_ptr: int, n: int, n_keypoints: int = -1):
        _check(self._lib.lcm_db_append_device(self._h, frame_id, _vp(d_ptr), n, n_keypoints))

    def __len__(self):
        return self._lib.lcm_db_size(self._h)

    def clear(self):
        _check(self._lib.lcm_db_clear(self._h))

    def truncate(self, n_frames: int):
        _check(self._lib.lcm_db_truncate(self._h, n_frames))

    def frame_info(self, slot: int) -> Tuple[int, int, int]:
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        _check(self._lib.lcm_db_frame_info(self._h, slot, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def read_frame(self, slot: int) -> np.ndarray:
        _, n, _ = self.frame_info(slot)
        out = np.empty((n, DESC_BYTES), np.uint8)
        _check(self._lib.lcm_db_read(self._h, slot, _ptr(out) if n else None, n))
        return out

    def save(self, path: str):
        _check(self._lib.lcm_db_save(self._h, path.encode()))

    def load(self, path: str):
        _check(self._lib.lcm_db_load(self._h, path.encode()))

    # -- pair mode ---------------------------------------------------------------------------------
    def match_pair(self, query, train) -> Tuple[np.ndarray, np.ndarray]:
        """BFMatcher(NORM_HAMMING).match: (train_idx int32[n], dist uint16[n]); n = 0 if either side is empty."""
        q, t = _rows(query), _rows(train)
        idx = np.empty(q.shape[0], np.int32)
        dist = np.empty(q.shape[0], np.uint16)
        n = C.c_int32(0)
        _check(self._lib.lcm_match_pair(self._h, _ptr(q), q.shape[0], _ptr(t), t.shape[0], _ptr(idx), _ptr(dist),
                                        C.byref(n)))
        return idx[: n.value], dist[: n.value]

    def match_features(self, query, train) -> Tuple[np.ndarray, int]:
        """matchFeatures: structured array of DMatch records that survive the ratio*min filter, and min_dist."""
        q, t = _rows(query), _rows(train)
        out = np.zeros(max(q.shape[0], 1), DMATCH_DTYPE)
        n, m = C.c_int32(0), C.c_int32(0)
        _check(self._lib.lcm_match_features(self._h, _ptr(q), q.shape[0], _ptr(t), t.shape[0],
                                            out.ctypes.data_as(_vp), C.byref(n), C.byref(m)))
        return out[: n.value], m.value

    def match_stored(self, query_frame_id: int, train_frame_id: int, cap: int = 65536) -> Tuple[np.ndarray, int]:
        """matchFeatures between two stored frames (device-resident rows)."""
        out = np.zeros(cap, DMATCH_DTYPE)
        n, m = C.c_int32(0), C.c_int32(0)
        _check(self._lib.lcm_match_stored(self._h, query_frame_id, train_frame_id, out.ctypes.data_as(_vp), cap,
                                          C.byref(n), C.byref(m)))
        return out[: n.value], m.value

    def match_stored_batch(self, pairs: Sequence[Tuple[int, int]], cap: Optional[int] = None):
        """matchFeatures for many stored (query id, train id) pairs in one launch: (list of DMatch arrays, min_dists)."""
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n = pr.shape[0]
        cap = 2048 * max(n, 1) if cap is None else cap
        out = np.zeros(max(cap, 1), DMATCH_DTYPE)
        offs = np.zeros(n + 1, np.uintp)
        md = np.zeros(max(n, 1), np.int32)
        _check(self._lib.lcm_match_stored_batch(self._h, _ptr(pr), n, out.ctypes.data_as(_vp), cap,
                                                offs.ctypes.data_as(_vp), md.ctypes.data_as(_vp)))
        return [out[int(offs[i]): int(offs[i + 1])] for i in range(n)], md[:n]

    def match_query_batch(self, query, train_ids: Sequence[int], cap: Optional[int] = None):
        """One host query frame against many stored frames in one launch: (list of DMatch arrays, min_dists)."""
        q = _rows(query)
        ids = np.ascontiguousarray(train_ids, np.int32)
        n = ids.shape[0]
        cap = max(q.shape[0], 1) * max(n, 1) if cap is None else cap
        out = np.zeros(max(cap, 1), DMATCH_DTYPE)
        offs = np.zeros(n + 1, np.uintp)
        md = np.zeros(max(n, 1), np.int32)
        _check(self._lib.lcm_match_query_batch(self._h, _ptr(q), q.shape[0], _ptr(ids), n, out.ctypes.data_as(_vp), cap,
                                               offs.ctypes.data_as(_vp), md.ctypes.data_as(_vp)))
        return [out[int(offs[i]): int(offs[i + 1])] for i in range(n)], md[:n]

    # -- pair mode, two neighbours + Lowe's ratio test ----------------------------------------------
    def knn2_pair(self, query, train) -> Tuple[np.ndarray, np.ndarray]:
        """BFMatcher(NORM_HAMMING).knnMatch(k=2): (train_idx int32[nq, 2], dist uint16[nq, 2]), best first; a missing
        second neighbour (one train row) is (-1, 0xFFFF); nq = 0 rows if either side is empty."""
        q, t = _rows(query), _rows(train)
        idx = np.empty((q.shape[0], 2), np.int32)
        dist = np.empty((q.shape[0], 2), np.uint16)
        n = C.c_int32(0)
        _check(self._lib.lcm_knn2_pair(self._h, _ptr(q), q.shape[0], _ptr(t), t.shape[0], _ptr(idx), _ptr(dist),
                                       C.byref(n)))
        rows = q.shape[0] if n.value else 0
        return idx[:rows], dist[:rows]

    def match_features_ratio(self, query, train, ratio: float) -> np.ndarray:
        """matchFeatures(desc1, desc2, good, ratio): knnMatch(k=2) + Lowe's ratio test -> DMatch records, query order."""
        q, t = _rows(query), _rows(train)
        out = np.zeros(max(q.shape[0], 1), DMATCH_DTYPE)
        n = C.c_int32(0)
        _check(self._lib.lcm_match_features_ratio(self._h, _ptr(q), q.shape[0], _ptr(t), t.shape[0], ratio,
                                                  out.ctypes.data_as(_vp), C.byref(n)))
        return out[: n.value]

    def match_stored_ratio(self, query_frame_id: int, train_frame_id: int, ratio: float, cap: int = 65536) -> np.ndarray:
        """The same between two stored frames (device-resident rows)."""
        out = np.zeros(max(cap, 1), DMATCH_DTYPE)
        n = C.c_int32(0)
        _check(self._lib.lcm_match_stored_ratio(self._h, query_frame_id, train_frame_id, ratio, out.ctypes.data_as(_vp), cap,
                                                C.byref(n)))
        return out[: n.value]

    def match_stored_batch_ratio(self, pairs: Sequence[Tuple[int, int]], ratio: float, cap: Optional[int] = None):
        """Ratio-filtered match lists of many stored (query id, train id) pairs in one launch: (list of DMatch arrays,
        offsets[n + 1])."""
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n = pr.shape[0]
        cap = 2048 * max(n, 1) if cap is None else cap
        out = np.zeros(max(cap, 1), DMATCH_DTYPE)
        offs = np.zeros(n + 1, np.uintp)
        _check(self._lib.lcm_match_stored_batch_ratio(self._h, _ptr(pr), n, ratio, out.ctypes.data_as(_vp), cap,
                                                      offs.ctypes.data_as(_vp)))
        return [out[int(offs[i]): int(offs[i + 1])] for i in range(n)], offs

    def match_query_batch_ratio(self, query, train_ids: Sequence[int], ratio: float, cap: Optional[int] = None):
        """One host query frame against many stored frames in one launch: (list of DMatch arrays, offsets[n + 1])."""
        q = _rows(query)
        ids = np.ascontiguousarray(train_ids, np.int32)
        n = ids.shape[0]
        cap = max(q.shape[0], 1) * max(n, 1) if cap is None else cap
        out = np.zeros(max(cap, 1), DMATCH_DTYPE)
        offs = np.zeros(n + 1, np.uintp)
        _check(self._lib.lcm_match_query_batch_ratio(self._h, _ptr(q), q.shape[0], _ptr(ids), n, ratio,
                                                     out.ctypes.data_as(_vp), cap, offs.ctypes.data_as(_vp)))
        return [out[int(offs[i]): int(offs[i + 1])] for i in range(n)], offs

    # -- pair mode on SIFT rows (128 uint8, L2): knnMatch(k=2) + Lowe's ratio test ------------------
    sift_pack_f32 = staticmethod(sift_pack_f32)

    def knn2_pair_l2(self, query, train) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """BFMatcher(NORM_L2).knnMatch(k=2) on SIFT rows: (train_idx int32[nq, 2], dist float32[nq, 2], dist_sq
        uint32[nq, 2]), best first; a missing second neighbour (one train row) is (-1, inf, 0xFFFFFFFF); nq = 0 rows if
        either side is empty."""
        q, t = _sift_rows(query), _sift_rows(train)
        idx = np.empty((q.shape[0], 2), np.int32)
        dist = np.empty((q.shape[0], 2), np.float32)
        dsq = np.empty((q.shape[0], 2), np.uint32)
        n = C.c_int32(0)
        _check(self._lib.lcm_knn2_pair_l2(self._h, _ptr(q), q.shape[0], _ptr(t), t.shape[0], _ptr(idx), _ptr(dist), _ptr(dsq),
                                          C.byref(n)))
        rows = q.shape[0] if n.value else 0
        return idx[:rows], dist[:rows], dsq[:rows]

    def match_features_ratio_l2(self, query, train, ratio: float) -> np.ndarray:
        """matchFeatures(desc1, desc2, good, ratio) on SIFT rows -> DMatch records, query order."""
        q, t = _sift_rows(query), _sift_rows(train)
        out = np.zeros(max(q.shape[0], 1), DMATCH_DTYPE)
        n = C.c_int32(0)
        _check(self._lib.lcm_match_features_ratio_l2(self._h, _ptr(q), q.shape[0], _ptr(t), t.shape[0], ratio,
                                                     out.ctypes.data_as(_vp), C.byref(n)))
        return out[: n.value]

    def match_pairs_ratio_l2(self, frames: Sequence[np.ndarray], pairs: Sequence[Tuple[int, int]], ratio: float,
                             cap: Optional[int] = None):
        """Ratio-filtered match lists of many (query position, train position) pairs into `frames` (SIFT matrices, each
        uploaded once) in one launch: (list of DMatch arrays, offsets[n + 1])."""
        fr = [_sift_rows(f) for f in frames]
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n = pr.shape[0]
        ptrs = (_vp * max(len(fr), 1))(*[f.ctypes.data if f.size else None for f in fr])
        rows = np.array([f.shape[0] for f in fr] or [0], np.int32)
        if cap is None:
            cap = sum(fr[q].shape[0] for q in pr[:, 0] if 0 <= q < len(fr))
        out = np.zeros(max(cap, 1), DMATCH_DTYPE)
        offs = np.zeros(n + 1, np.uintp)
        _check(self._lib.lcm_match_pairs_ratio_l2(self._h, C.cast(ptrs, _vp), rows.ctypes.data_as(_vp), len(fr), _ptr(pr), n,
                                                  ratio, out.ctypes.data_as(_vp), cap, offs.ctypes.data_as(_vp)))
        return [out[int(offs[i]): int(offs[i + 1])] for i in range(n)], offs

    # -- loop search on SIFT rows: ratio-test counts per pair, decided on the device -----------------
    @staticmethod
    def _sift_frames(frames):
        fr = [_sift_rows(f) for f in frames]
        ptrs = (_vp * max(len(fr), 1))(*[f.ctypes.data if f.size else None for f in fr])
        rows = np.array([f.shape[0] for f in fr] or [0], np.int32)
        return fr, ptrs, rows

    def score_pairs_ratio_l2(self, frames: Sequence[np.ndarray], pairs: Sequence[Tuple[int, int]], ratio: float) -> np.ndarray:
        """Per (query position, train position) pair into `frames` (SIFT matrices, each uploaded once): the number of query
        rows that pass Lowe's ratio test and the smallest squared distance, L2_SCORE_DTYPE[n]; nothing else leaves the
        device."""
        fr, ptrs, rows = self._sift_frames(frames)
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n = pr.shape[0]
        out = np.zeros(max(n, 1), L2_SCORE_DTYPE)
        _check(self._lib.lcm_score_pairs_ratio_l2(self._h, C.cast(ptrs, _vp), rows.ctypes.data_as(_vp), len(fr), _ptr(pr), n,
                                                  ratio, out.ctypes.data_as(_vp)))
        return out[:n]

    def loop_search_ratio_l2(self, frames: Sequence[np.ndarray], loop_gap: int, skip=None, ratio: Optional[float] = None,
                             min_rows: Optional[int] = None, min_matches: Optional[int] = None, cap: Optional[int] = None,
                             out: Optional[np.ndarray] = None) -> Tuple[np.ndarray, int]:
        """The reference's loop search (src/main.cpp:1375-1388) over SIFT matrices by position: (candidates in (curr, past)
        order, pairs scored).  skip: optional flags, one per frame.  ratio / min_rows / min_matches left at None: 0.7 / 100
        / 300 (all three None: rp = NULL)."""
        fr, ptrs, rows = self._sift_frames(frames)
        rp = _ratio_loop_params(ratio, min_rows, min_matches)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        assert sk is None or sk.shape == (len(fr),)
        if out is None:
            cap = len(fr) * len(fr) if cap is None else cap
            out = np.zeros(max(cap, 1), CANDIDATE_DTYPE)
        else:
            assert out.dtype == CANDIDATE_DTYPE and out.flags["C_CONTIGUOUS"]
            cap = len(out) if cap is None else cap
        n, npairs = C.c_size_t(0), C.c_size_t(0)
        _check(self._lib.lcm_loop_search_ratio_l2(self._h, C.cast(ptrs, _vp), rows.ctypes.data_as(_vp), len(fr), _ptr(sk),
                                                  loop_gap, None if rp is None else C.byref(rp), out.ctypes.data_as(_vp), cap,
                                                  C.byref(n), C.byref(npairs)))
        return out[: n.value], npairs.value

    def l2_ratio_test_device(self, d1, d2, ratio: float) -> np.ndarray:
        """Diagnostic: the count kernel's ratio-test verdict on squared distances (d1[i], d2[i]) -> uint8[n] of 0 / 1."""
        a, b = np.ascontiguousarray(d1, np.uint32).ravel(), np.ascontiguousarray(d2, np.uint32).ravel()
        assert a.shape == b.shape
        out = np.full(max(a.size, 1), 0xFF, np.uint8)
        _check(self._lib.lcm_l2_ratio_test_device(self._h, _ptr(a), _ptr(b), a.size, ratio, out.ctypes.data_as(_vp)))
        return out[: a.size]

    # -- the SIFT keyframe store: rows uploaded and packed once, searched from the device ----------
    def l2_db_append(self, rows) -> int:
        """Stores a SIFT matrix (0..65535 rows); returns its slot."""
        r = _sift_rows(rows)
        slot = C.c_int32(-1)
        _check(self._lib.lcm_l2_db_append(self._h, _ptr(r), r.shape[0], C.byref(slot)))
        return slot.value

    def l2_db_size(self) -> int:
        return self._lib.lcm_l2_db_size(self._h)

    def l2_db_rows(self, slot: int) -> int:
        n = C.c_int32(-1)
        _check(self._lib.lcm_l2_db_rows(self._h, slot, C.byref(n)))
        return n.value

    def l2_db_read(self, slot: int) -> np.ndarray:
        """The raw rows of a slot, uint8[n, 128]."""
        out = np.zeros((self.l2_db_rows(slot), SIFT_BYTES), np.uint8)
        _check(self._lib.lcm_l2_db_read(self._h, slot, _ptr(out), out.shape[0]))
        return out

    def l2_db_truncate(self, n_frames: int):
        _check(self._lib.lcm_l2_db_truncate(self._h, n_frames))

    def l2_db_clear(self):
        _check(self._lib.lcm_l2_db_clear(self._h))

    def l2_db_info(self) -> L2DbInfo:
        info = L2DbInfo()
        _check(self._lib.lcm_l2_db_info_read(self._h, C.byref(info)))
        return info

    def l2_db_score_pairs(self, pairs: Sequence[Tuple[int, int]], ratio: float) -> np.ndarray:
        """score_pairs_ratio_l2 over stored (query slot, train slot) pairs: L2_SCORE_DTYPE[n]."""
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n = pr.shape[0]
        out = np.zeros(max(n, 1), L2_SCORE_DTYPE)
        _check(self._lib.lcm_l2_db_score_pairs(self._h, _ptr(pr), n, ratio, out.ctypes.data_as(_vp)))
        return out[:n]

    def l2_db_match_pairs_ratio(self, pairs: Sequence[Tuple[int, int]], ratio: float, cap: Optional[int] = None):
        """match_pairs_ratio_l2 over stored (query slot, train slot) pairs: (list of DMatch arrays, offsets[n + 1])."""
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n = pr.shape[0]
        if cap is None:
            size = self.l2_db_size()
            cap = sum(self.l2_db_rows(int(q)) for q in pr[:, 0] if 0 <= q < size)
        out = np.zeros(max(cap, 1), DMATCH_DTYPE)
        offs = np.zeros(n + 1, np.uintp)
        _check(self._lib.lcm_l2_db_match_pairs_ratio(self._h, _ptr(pr), n, ratio, out.ctypes.data_as(_vp), cap,
                                                     offs.ctypes.data_as(_vp)))
        return [out[int(offs[i]): int(offs[i + 1])] for i in range(n)], offs

    def _l2_db_search_args(self, skip, ratio, min_rows, min_matches, cap, out):
        rp = _ratio_loop_params(ratio, min_rows, min_matches)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
        assert sk is None or sk.shape == (self.l2_db_size(),)
        if out is None:
            cap = max(self.l2_db_size(), 1) ** 2 if cap is None else cap
            out = np.zeros(max(cap, 1), CANDIDATE_DTYPE)
        else:
            assert out.dtype == CANDIDATE_DTYPE and out.flags["C_CONTIGUOUS"]
            cap = len(out) if cap is None else cap
        return (None if rp is None else C.byref(rp)), rp, sk, cap, out

    def l2_db_loop_search(self, loop_gap: int, skip=None, ratio: Optional[float] = None, min_rows: Optional[int] = None,
                          min_matches: Optional[int] = None, cap: Optional[int] = None,
                          out: Optional[np.ndarray] = None) -> Tuple[np.ndarray, int]:
        """loop_search_ratio_l2 over the stored slots: (candidates in (curr, past) order, pairs scored).  skip: optional
        flags, one per slot."""
        rpp, _rp, sk, cap, out = self._l2_db_search_args(skip, ratio, min_rows, min_matches, cap, out)
        n, npairs = C.c_size_t(0), C.c_size_t(0)
        _check(self._lib.lcm_l2_db_loop_search(self._h, _ptr(sk), loop_gap, rpp, out.ctypes.data_as(_vp), cap, C.byref(n),
                                               C.byref(npairs)))
        return out[: n.value], npairs.value

    def l2_db_detect_loops(self, curr: int, loop_gap: int, query=None, skip=None, ratio: Optional[float] = None,
                           min_rows: Optional[int] = None, min_matches: Optional[int] = None, cap: Optional[int] = None,
                           out: Optional[np.ndarray] = None) -> Tuple[np.ndarray, int]:
        """One keyframe against the stored slots [0, curr - loop_gap]: (candidates, pairs scored).  query: host SIFT rows
        standing for position `curr` (not stored), or None for the stored slot `curr`."""
        rpp, _rp, sk, cap, out = self._l2_db_search_args(skip, ratio, min_rows, min_matches, cap, out)
        q = None if query is None else _sift_rows(query)
        # an empty host matrix is still the host form: the library tells the two apart by the pointer
        qp = None if q is None else (q if q.size else np.zeros((1, SIFT_BYTES), np.uint8)).ctypes.data_as(_vp)
        n, npairs = C.c_size_t(0), C.c_size_t(0)
        _check(self._lib.lcm_l2_db_detect_loops(self._h, curr, qp, 0 if q is None else q.shape[0], _ptr(sk), loop_gap, rpp,
                                                out.ctypes.data_as(_vp), cap, C.byref(n), C.byref(npairs)))
        return out[: n.value], npairs.value

    # -- the store's loop correspondences: ratio test, compaction and keypoint gather on the device --
    @staticmethod
    def _kp(pts, n: int) -> np.ndarray:
        p = np.ascontiguousarray(pts, dtype=np.float32)
        if p.shape != (n, 2):
            raise ValueError(f"keypoints must be ({n}, 2) float32 (x, y), got {p.shape}")
        return p

    def l2_db_append_kp(self, rows, pts) -> int:
        """Stores a SIFT matrix with its keypoint coordinates, float32[n, 2] of (x, y) carried bit for bit; returns its slot."""
        r = _sift_rows(rows)
        p = self._kp(pts, r.shape[0])
        slot = C.c_int32(-1)
        _check(self._lib.lcm_l2_db_append_kp(self._h, _ptr(r), _ptr(p), r.shape[0], C.byref(slot)))
        return slot.value

    def l2_db_read_kp(self, slot: int) -> np.ndarray:
        """The keypoints of a slot stored with l2_db_append_kp, float32[n, 2]."""
        out = np.zeros((self.l2_db_rows(slot), 2), np.float32)
        _check(self._lib.lcm_l2_db_read_kp(self._h, slot, out.ctypes.data_as(_vp), out.shape[0]))
        return out

    # -- what the store's list calls share.  Their C signatures are regular: [the stages' parameters], then (the candidate
    # search's arguments,) the per-pair records of the stages, out, pts, the stages' masks, cap, offsets (, floor_inliers, best) --
    @staticmethod
    def _list_buffers(cap: int, n: int, points: bool = True, epi: bool = False, lo: bool = False, pose: bool = False, out=None,
                      pts=None, results=None, info=None, mask=None, pose_results=None, pose_mask=None):
        """The buffers of a list call with room for cap records of n pairs (or candidates), the caller's (checked) or new ones,
        in the order of the C signatures and of the returned tuples: ([per-pair records of the stages epi / lo / pose that the
        call runs], [out, pts (None without points), the stages' masks])."""
        if points or pts is not None:
            pts = _buffer(pts, np.float32, cap, 4, contiguous=True)
        per_pair, per_record = [], [_buffer(out, DMATCH_DTYPE, cap, contiguous=True), pts if points else None]
        if epi:
            per_pair.append(_buffer(results, EPI_RESULT_DTYPE, n))
            per_record.append(_buffer(mask, np.uint8, cap))
        if lo:
            per_pair.append(_buffer(info, LO_INFO_DTYPE, n))
        if pose:
            per_pair.append(_buffer(pose_results, POSE_RESULT_DTYPE, n))
            per_record.append(_buffer(pose_mask, np.uint8, cap))
        return per_pair, per_record

    @staticmethod
    def _list_slices(per_pair, per_record, n: int, total: int) -> list:
        return [a[:n] for a in per_pair] + [None if a is None else a[:total] for a in per_record]

    def _db_pairs_call(self, fn, params: tuple, pairs, ratio: float, cap: Optional[int], out=None, **bufs):
        """fn over stored pairs: (the stages' per-pair records, out, pts, the stages' masks, offsets[n + 1]).  cap: given,
        else the caller's out, else the query sides' rows."""
        pr = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n = pr.shape[0]
        if cap is None and out is not None:
            cap = len(out)
        elif cap is None:
            size = self.l2_db_size()
            cap = sum(self.l2_db_rows(int(q)) for q in pr[:, 0] if 0 <= q < size)
        per_pair, per_record = self._list_buffers(cap, n, out=out, **bufs)
        ptrs = [None if a is None else a.ctypes.data_as(_vp) for a in per_pair + per_record]
        offs = np.zeros(n + 1, np.uintp)
        self.last_offsets = offs
        _check(fn(self._h, _ptr(pr), n, ratio, *params, *ptrs, cap, offs.ctypes.data_as(_vp)))
        return (*self._list_slices(per_pair, per_record, n, int(offs[n])), offs)

    def _db_detect_call(self, fn, params: tuple, curr: int, loop_gap: int, query, query_pts, skip, ratio, min_rows, min_matches,
                        cand_cap: Optional[int], cap: Optional[int], cands=None, floor_inliers: Optional[int] = None, out=None, **bufs):
        """fn for one keyframe: (candidates, pairs scored, then as _db_pairs_call with offsets[n_candidates + 1], then best when
        floor_inliers is given).  cap: given, else the caller's out, else the keyframe's rows x the candidates there is room for."""
        rpp, _rp, sk, cand_cap, cands = self._l2_db_search_args(skip, ratio, min_rows, min_matches, cand_cap, cands)
        q = None if query is None else _sift_rows(query)
        nq = 0 if q is None else q.shape[0]
        # an empty host matrix is still the host form: the library tells the two apart by the pointer
        qp = None if q is None else (q if q.size else np.zeros((1, SIFT_BYTES), np.uint8)).ctypes.data_as(_vp)
        kp = None if (q is None or query_pts is None) else self._kp(query_pts, nq)
        kpp = None if kp is None else (kp if kp.size else np.zeros((1, 2), np.float32)).ctypes.data_as(_vp)
        if cap is None and out is not None:
            cap = len(out)
        elif cap is None:
            rows_q = nq if q is not None else (self.l2_db_rows(curr) if 0 <= curr < self.l2_db_size() else 0)
            cap = rows_q * max(min(cand_cap, self.l2_db_size()), 1)
        per_pair, per_record = self._list_buffers(cap, cand_cap, out=out, **bufs)
        ptrs = [None if a is None else a.ctypes.data_as(_vp) for a in per_pair + per_record]
        offs = np.zeros(cand_cap + 1, np.uintp)
        n, npairs, best = C.c_size_t(0), C.c_size_t(0), C.c_int32(-1)
        self.last_offsets, self.last_n_cands = offs, n
        tail = () if floor_inliers is None else (floor_inliers, C.byref(best))
        _check(fn(self._h, curr, qp, kpp, nq, _ptr(sk), loop_gap, rpp, *params, cands.ctypes.data_as(_vp), cand_cap, C.byref(n), C.byref(npairs),
                  *ptrs, cap, offs.ctypes.data_as(_vp), *tail))
        lists = self._list_slices(per_pair, per_record, n.value, int(offs[n.value]))
        return (cands[: n.value], npairs.value, *lists, offs[: n.value + 1], *(() if floor_inliers is None else (best.value,)))

    def l2_db_match_points(self, pairs: Sequence[Tuple[int, int]], ratio: float, cap: Optional[int] = None, points: bool = True,
                           out: Optional[np.ndarray] = None, pts: Optional[np.ndarray] = None):
        """l2_db_match_pairs_ratio with the lists made on the device: (DMATCH_DTYPE[total], float32[total, 4] of (qx, qy, tx, ty)
        or None when points is False, offsets[n + 1]).  out / pts: the caller's buffers (cap = their length unless given).
        After LcmError(ERR_CAPACITY), `self.last_offsets[n]` holds the needed record count."""
        return self._db_pairs_call(self._lib.lcm_l2_db_match_points, (), pairs, ratio, cap, points=points, out=out, pts=pts)

    def l2_db_detect_loops_points(self, curr: int, loop_gap: int, query=None, query_pts=None, skip=None,
                                  ratio: Optional[float] = None, min_rows: Optional[int] = None, min_matches: Optional[int] = None,
                                  cand_cap: Optional[int] = None, cap: Optional[int] = None, points: bool = True,
                                  cands: Optional[np.ndarray] = None, out: Optional[np.ndarray] = None,
                                  pts: Optional[np.ndarray] = None):
        """One keyframe against the stored slots [0, curr - loop_gap] with the candidates' match lists and keypoints:
        (candidates, pairs scored, DMATCH_DTYPE[total], float32[total, 4] or None, offsets[n_candidates + 1]).  query /
        query_pts: host SIFT rows and their keypoints standing for position `curr` (not stored), or None for the stored
        slot `curr`.  After LcmError(ERR_CAPACITY), `self.last_offsets` / `self.last_n_cands` hold what the call reported."""
        return self._db_detect_call(self._lib.lcm_l2_db_detect_loops_points, (), curr, loop_gap, query, query_pts, skip, ratio, min_rows,
                                    min_matches, cand_cap, cap, cands=cands, points=points, out=out, pts=pts)

    # -- loop verification: essential-matrix RANSAC on the device (lcm_epi_*) --
    def epi_verify_pairs(self, pts, offsets, ep: EpiParams, want_mask: bool = True):
        """The RANSAC over host point pairs float32[total, 4] in the offsets layout of l2_db_match_points:
        (EPI_RESULT_DTYPE[n_pairs], uint8[total] inlier mask or None)."""
        offs = np.ascontiguousarray(offsets, np.uintp)
        n = len(offs) - 1
        p = _point_pairs(pts)
        assert n >= 0 and len(p) >= (int(offs[n]) if n >= 0 else 0)
        res = np.zeros(max(n, 1), EPI_RESULT_DTYPE)
        mask = np.zeros(max(int(offs[n]), 1), np.uint8) if want_mask else None
        _check(self._lib.lcm_epi_verify_pairs(self._h, _ptr(p), offs.ctypes.data_as(_vp), n, C.byref(ep), res.ctypes.data_as(_vp),
                                              None if mask is None else mask.ctypes.data_as(_vp)))
        return res[:n], (None if mask is None else mask[: int(offs[n])])

    def epi_hypotheses(self, pts, pair_index: int, ep: EpiParams):
        """What the solver kernel makes of one pair standing at position pair_index of a call: (int32[iters, 8] sample
        indices, float64[iters, 9] essential matrices, row-major)."""
        p = _point_pairs(pts)
        samples = np.zeros((ep.iters, 8), np.int32)
        E = np.zeros((ep.iters, 9), np.float64)
        _check(self._lib.lcm_epi_hypotheses(self._h, _ptr(p), len(p), pair_index, C.byref(ep), samples.ctypes.data_as(_vp),
                                            E.ctypes.data_as(_vp)))
        return samples, E

    def epi_score_models(self, pts, E, ep: EpiParams) -> np.ndarray:
        """The scoring kernel's inlier count of every matrix of E float64[n_models, 9] over the point pairs: int32[n_models]."""
        p = _point_pairs(pts)
        e = np.ascontiguousarray(E, np.float64).reshape(-1, 9)
        counts = np.zeros(len(e), np.int32)
        _check(self._lib.lcm_epi_score_models(self._h, _ptr(p), len(p), _ptr(e), len(e), C.byref(ep), counts.ctypes.data_as(_vp)))
        return counts

    def epi_db_verify_pairs(self, pairs: Sequence[Tuple[int, int]], ratio: float, ep: EpiParams, cap: Optional[int] = None,
                            out: Optional[np.ndarray] = None, pts: Optional[np.ndarray] = None,
                            results: Optional[np.ndarray] = None, mask: Optional[np.ndarray] = None):
        """l2_db_match_points followed by the RANSAC on the device's own point records: (EPI_RESULT_DTYPE[n], DMATCH_DTYPE[total],
        float32[total, 4], uint8[total] mask, offsets[n + 1]).  out / pts / results / mask: the caller's buffers."""
        return self._db_pairs_call(self._lib.lcm_epi_db_verify_pairs, (C.byref(ep),), pairs, ratio, cap, epi=True, out=out, pts=pts,
                                   results=results, mask=mask)

    def epi_db_detect_loops(self, curr: int, loop_gap: int, ep: EpiParams, query=None, query_pts=None, skip=None,
                            ratio: Optional[float] = None, min_rows: Optional[int] = None, min_matches: Optional[int] = None,
                            cand_cap: Optional[int] = None, cap: Optional[int] = None):
        """l2_db_detect_loops_points plus the verification of every candidate: (candidates, pairs scored, EPI_RESULT_DTYPE
        [n_candidates], DMATCH_DTYPE[total], float32[total, 4], uint8[total] mask, offsets[n_candidates + 1])."""
        return self._db_detect_call(self._lib.lcm_epi_db_detect_loops, (C.byref(ep),), curr, loop_gap, query, query_pts, skip, ratio,
                                    min_rows, min_matches, cand_cap, cap, epi=True)

    # -- loop verification, second step: the RANSAC's best hypotheses refitted on their inliers (lcm_lo_*) --
    def lo_verify_pairs(self, pts, offsets, ep: EpiParams, lp: Optional[LoParams] = None, want_mask: bool = True):
        """epi_verify_pairs plus the local optimisation: (EPI_RESULT_DTYPE[n_pairs], LO_INFO_DTYPE[n_pairs], uint8[total]
        inlier mask or None)."""
        offs = np.ascontiguousarray(offsets, np.uintp)
        n = len(offs) - 1
        p = _point_pairs(pts)
        assert n >= 0 and len(p) >= (int(offs[n]) if n >= 0 else 0)
        res = np.zeros(max(n, 1), EPI_RESULT_DTYPE)
        info = np.zeros(max(n, 1), LO_INFO_DTYPE)
        mask = np.zeros(max(int(offs[n]), 1), np.uint8) if want_mask else None
        _check(self._lib.lcm_lo_verify_pairs(self._h, _ptr(p), offs.ctypes.data_as(_vp), n, C.byref(ep),
                                             None if lp is None else C.byref(lp), res.ctypes.data_as(_vp), info.ctypes.data_as(_vp),
                                             None if mask is None else mask.ctypes.data_as(_vp)))
        return res[:n], info[:n], (None if mask is None else mask[: int(offs[n])])

    def lo_select(self, counts) -> np.ndarray:
        """The selection kernel on caller-supplied counts int32[iters]: int32[64], the hypotheses of the 64 largest keys
        (count << 16 | 0xFFFF - hypothesis), largest first."""
        c = np.ascontiguousarray(counts, np.int32)
        seeds = np.zeros(LO_SEEDS, np.int32)
        _check(self._lib.lcm_lo_select(self._h, _ptr(c), len(c), seeds.ctypes.data_as(_vp)))
        return seeds

    def lo_refit_models(self, pts, E, mult: float, ep: EpiParams):
        """ONE refit round under the multiplier `mult` for each of the models E float64[n_models <= 64, 9] over the point
        pairs: (float64[n_models, 9] refits, int32[n_models] records selected, int32[n_models] lcm_lo_status)."""
        p = _point_pairs(pts)
        e = np.ascontiguousarray(E, np.float64).reshape(-1, 9)
        n = len(e)
        out, n_sel, status = np.zeros((max(n, 1), 9)), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        _check(self._lib.lcm_lo_refit_models(self._h, _ptr(p), len(p), _ptr(e), n, float(mult), C.byref(ep), out.ctypes.data_as(_vp),
                                             n_sel.ctypes.data_as(_vp), status.ctypes.data_as(_vp)))
        return out[:n], n_sel[:n], status[:n]

    def lo_db_verify_pairs(self, pairs: Sequence[Tuple[int, int]], ratio: float, ep: EpiParams, lp: Optional[LoParams] = None,
                           pp: Optional[PoseParams] = None, cap: Optional[int] = None, out: Optional[np.ndarray] = None,
                           pts: Optional[np.ndarray] = None, results: Optional[np.ndarray] = None, info: Optional[np.ndarray] = None,
                           mask: Optional[np.ndarray] = None, pose_results: Optional[np.ndarray] = None,
                           pose_mask: Optional[np.ndarray] = None):
        """pose_db_verify_pairs with the local optimisation between the RANSAC and the pose recovery: (EPI_RESULT_DTYPE[n],
        LO_INFO_DTYPE[n], POSE_RESULT_DTYPE[n], DMATCH_DTYPE[total], float32[total, 4], uint8[total] inlier mask, uint8[total]
        pose mask, offsets[n + 1]).  out / pts / results / info / mask / pose_results / pose_mask: the caller's buffers."""
        return self._db_pairs_call(self._lib.lcm_lo_db_verify_pairs, (C.byref(ep), _ref(lp), _ref(pp)), pairs, ratio, cap, epi=True, lo=True,
                                   pose=True, out=out, pts=pts, results=results, info=info, mask=mask, pose_results=pose_results,
                                   pose_mask=pose_mask)

    def lo_db_detect_loops(self, curr: int, loop_gap: int, ep: EpiParams, lp: Optional[LoParams] = None,
                           pp: Optional[PoseParams] = None, floor_inliers: int = -1, query=None, query_pts=None, skip=None,
                           ratio: Optional[float] = None, min_rows: Optional[int] = None, min_matches: Optional[int] = None,
                           cand_cap: Optional[int] = None, cap: Optional[int] = None):
        """pose_db_detect_loops with the local optimisation between the RANSAC and the pose recovery: (candidates, pairs scored,
        EPI_RESULT_DTYPE[n_candidates], LO_INFO_DTYPE[n_candidates], POSE_RESULT_DTYPE[n_candidates], DMATCH_DTYPE[total],
        float32[total, 4], uint8[total] inlier mask, uint8[total] pose mask, offsets[n_candidates + 1], best)."""
        return self._db_detect_call(self._lib.lcm_lo_db_detect_loops, (C.byref(ep), _ref(lp), _ref(pp)), curr, loop_gap, query, query_pts,
                                    skip, ratio, min_rows, min_matches, cand_cap, cap, floor_inliers=floor_inliers, epi=True, lo=True,
                                    pose=True)

    # -- the loop's relative pose on the device and the best loop (lcm_pose_*) --
    def pose_recover_pairs(self, pts, offsets, E, ep: EpiParams, pp: Optional[PoseParams] = None, mask_in=None,
                           want_mask: bool = True):
        """recoverPose over host point pairs float32[total, 4] in the offsets layout of l2_db_match_points, pair p under
        E[p] (float64[n_pairs, 9], row-major); mask_in uint8[total] or None = every record.  ep supplies K only.
        (POSE_RESULT_DTYPE[n_pairs], uint8[total] mask of the records in front of both cameras, or None)."""
        offs = np.ascontiguousarray(offsets, np.uintp)
        n = len(offs) - 1
        p = _point_pairs(pts)
        e = np.ascontiguousarray(E, np.float64).reshape(-1, 9)
        total = int(offs[n]) if n >= 0 else 0
        assert n >= 0 and len(p) >= total and len(e) >= n
        mi = None if mask_in is None else np.ascontiguousarray(mask_in, np.uint8)
        assert mi is None or len(mi) >= total
        res = np.zeros(max(n, 1), POSE_RESULT_DTYPE)
        mask = np.zeros(max(total, 1), np.uint8) if want_mask else None
        _check(self._lib.lcm_pose_recover_pairs(self._h, _ptr(p), offs.ctypes.data_as(_vp), n, _ptr(e), None if mi is None else _ptr(mi),
                                                C.byref(ep), None if pp is None else C.byref(pp), res.ctypes.data_as(_vp),
                                                None if mask is None else mask.ctypes.data_as(_vp)))
        return res[:n], (None if mask is None else mask[:total])

    def pose_candidates(self, E):
        """The kernel's decomposition alone: (float64[n, 4, 9] rotations, float64[n, 4, 3] translations, int32[n] status) of
        the matrices E float64[n, 9]; hypothesis k = (Ra, t), (Rb, t), (Ra, -t), (Rb, -t)."""
        e = np.ascontiguousarray(E, np.float64).reshape(-1, 9)
        n = len(e)
        R4, t4, status = np.zeros((max(n, 1), 4, 9)), np.zeros((max(n, 1), 4, 3)), np.zeros(max(n, 1), np.int32)
        _check(self._lib.lcm_pose_candidates(self._h, _ptr(e), n, R4.ctypes.data_as(_vp), t4.ctypes.data_as(_vp), status.ctypes.data_as(_vp)))
        return R4[:n], t4[:n], status[:n]

    def pose_db_verify_pairs(self, pairs: Sequence[Tuple[int, int]], ratio: float, ep: EpiParams, pp: Optional[PoseParams] = None,
                             cap: Optional[int] = None, out: Optional[np.ndarray] = None, pts: Optional[np.ndarray] = None,
                             results: Optional[np.ndarray] = None, mask: Optional[np.ndarray] = None,
                             pose_results: Optional[np.ndarray] = None, pose_mask: Optional[np.ndarray] = None):
        """epi_db_verify_pairs followed by the pose recovery on the device's own records, matrices and mask:
        (EPI_RESULT_DTYPE[n], POSE_RESULT_DTYPE[n], DMATCH_DTYPE[total], float32[total, 4], uint8[total] inlier mask,
        uint8[total] pose mask, offsets[n + 1]).  out / pts / results / mask / pose_results / pose_mask: the caller's buffers."""
        return self._db_pairs_call(self._lib.lcm_pose_db_verify_pairs, (C.byref(ep), _ref(pp)), pairs, ratio, cap, epi=True, pose=True,
                                   out=out, pts=pts, results=results, mask=mask, pose_results=pose_results, pose_mask=pose_mask)

    def pose_db_detect_loops(self, curr: int, loop_gap: int, ep: EpiParams, pp: Optional[PoseParams] = None, floor_inliers: int = -1,
                             query=None, query_pts=None, skip=None, ratio: Optional[float] = None, min_rows: Optional[int] = None,
                             min_matches: Optional[int] = None, cand_cap: Optional[int] = None, cap: Optional[int] = None):
        """epi_db_detect_loops plus the pose recovery of every candidate and the choice of the best loop: (candidates, pairs
        scored, EPI_RESULT_DTYPE[n_candidates], POSE_RESULT_DTYPE[n_candidates], DMATCH_DTYPE[total], float32[total, 4],
        uint8[total] inlier mask, uint8[total] pose mask, offsets[n_candidates + 1], best).  best: the index of the candidate
        the reference's globalBest* update ends at when it starts from floor_inliers, or -1."""
        return self._db_detect_call(self._lib.lcm_pose_db_detect_loops, (C.byref(ep), _ref(pp)), curr, loop_gap, query, query_pts, skip,
                                    ratio, min_rows, min_matches, cand_cap, cap, floor_inliers=floor_inliers, epi=True, pose=True)

    @staticmethod
    def pose_best(epi_results, pose_results, ep: EpiParams, pp: Optional[PoseParams] = None, floor_inliers: int = -1) -> int:
        """lcm_pose_best (host only): see capi.pose_best."""
        return pose_best(epi_results, pose_results, ep, pp, floor_inliers)

    # -- closing the loop: pose-graph Gauss-Newton correction (lcm_pgo_*) --
    def pgo_optimize(self, poses, edges, pp: Optional[PgoParams] = None, valid=None):
        """optimizePoseGraph over PGO_POSE_DTYPE[n] and PGO_EDGE_DTYPE[m] (valid: uint8[n] or None = all): (PGO_POSE_DTYPE[n],
        PgoInfo)."""
        p, v = _pgo_graph(poses, valid)
        e = np.ascontiguousarray(edges, PGO_EDGE_DTYPE)
        out = np.zeros(max(len(p), 1), PGO_POSE_DTYPE)
        info = PgoInfo()
        _check(self._lib.lcm_pgo_optimize(self._h, _ptr(p), _ptr(v), len(p), _ptr(e), len(e), _ref(pp), _ptr(out), C.byref(info)))
        return out[:len(p)], info

    def pgo_step(self, poses, edges, pp: Optional[PgoParams] = None, valid=None):
        """The test seam, one iteration: (params float64[n, 6] before the update, residuals float64[m, 6], Jacobian
        float64[m, 6, 12], dp float64[n - 1, 6], PgoInfo)."""
        p, v = _pgo_graph(poses, valid)
        e = np.ascontiguousarray(edges, PGO_EDGE_DTYPE)
        n, m = len(p), len(e)
        params, res, jac, dp = np.zeros((max(n, 1), 6)), np.zeros((max(m, 1), 6)), np.zeros((max(m, 1), 6, 12)), np.zeros((max(n - 1, 1), 6))
        info = PgoInfo()
        _check(self._lib.lcm_pgo_step(self._h, _ptr(p), _ptr(v), n, _ptr(e), m, _ref(pp), _ptr(params), _ptr(res), _ptr(jac), _ptr(dp),
                                      C.byref(info)))
        return params[:n], res[:m], jac[:m], dp[:max(n - 1, 0)], info

    def pgo_close_loop(self, poses, past: int, curr: int, pose_result, pp: Optional[PgoParams] = None, valid=None):
        """lcm_pgo_build_graph on the relative pose (a PoseResult or a POSE_RESULT_DTYPE record) + lcm_pgo_optimize:
        (PGO_POSE_DTYPE[n], PgoInfo).  pp.loop_direction says how the pose becomes the loop edge."""
        p, v = _pgo_graph(poses, valid)
        if isinstance(pose_result, PoseResult):
            pr = pose_result
        else:
            pr = PoseResult.from_buffer_copy(np.ascontiguousarray(pose_result, POSE_RESULT_DTYPE).reshape(1)[0].tobytes())
        out = np.zeros(max(len(p), 1), PGO_POSE_DTYPE)
        info = PgoInfo()
        _check(self._lib.lcm_pgo_close_loop(self._h, _ptr(p), _ptr(v), len(p), past, curr, C.byref(pr), _ref(pp), _ptr(out), C.byref(info)))
        return out[:len(p)], info

    # -- after the loop: alternating bundle adjustment and outlier removal (lcm_ba_*) --
    def ba_error(self, poses, points, obs, bp: BaParams, valid=None, per_observation: bool = False):
        """computeReprojectionError: the mean, or (mean, float64[n_obs]) with per_observation."""
        p, v, x, o = _ba_map(poses, valid, points, obs)
        mean, each = C.c_double(-1.0), (np.zeros(max(len(o), 1)) if per_observation else None)
        _check(self._lib.lcm_ba_error(self._h, _ptr(p), _ptr(v), len(p), _ptr(x), len(x), _ptr(o), len(o), _ref(bp), C.byref(mean), _ptr(each)))
        return (mean.value, each[:len(o)]) if per_observation else mean.value

    def ba_refine_cameras(self, poses, points, obs, bp: BaParams, valid=None):
        """The camera phase: (PGO_POSE_DTYPE[n_poses], BA_ELEM_INFO_DTYPE[n_poses])."""
        p, v, x, o = _ba_map(poses, valid, points, obs)
        out, info = np.zeros(max(len(p), 1), PGO_POSE_DTYPE), np.zeros(max(len(p), 1), BA_ELEM_INFO_DTYPE)
        _check(self._lib.lcm_ba_refine_cameras(self._h, _ptr(p), _ptr(v), len(p), _ptr(x), len(x), _ptr(o), len(o), _ref(bp), _ptr(out), _ptr(info)))
        return out[:len(p)], info[:len(p)]

    def ba_refine_points(self, poses, points, obs, bp: BaParams, valid=None):
        """The point phase: (BA_POINT_DTYPE[n_points], BA_ELEM_INFO_DTYPE[n_points])."""
        p, v, x, o = _ba_map(poses, valid, points, obs)
        out, info = np.zeros(max(len(x), 1), BA_POINT_DTYPE), np.zeros(max(len(x), 1), BA_ELEM_INFO_DTYPE)
        _check(self._lib.lcm_ba_refine_points(self._h, _ptr(p), _ptr(v), len(p), _ptr(x), len(x), _ptr(o), len(o), _ref(bp), _ptr(out), _ptr(info)))
        return out[:len(x)], info[:len(x)]

    def _ba_step(self, call, width, n_elem, p, v, x, o, bp):
        n = max(n_elem, 1)
        r, J = np.zeros((max(len(o), 1), 2)), np.zeros((max(len(o), 1), 2, width))
        H, g, dp, info = np.zeros((n, width, width)), np.zeros((n, width)), np.zeros((n, width)), np.zeros(n, BA_ELEM_INFO_DTYPE)
        _check(call(self._h, _ptr(p), _ptr(v), len(p), _ptr(x), len(x), _ptr(o), len(o), _ref(bp), _ptr(r), _ptr(J), _ptr(H), _ptr(g), _ptr(dp),
                    _ptr(info)))
        return r[:len(o)], J[:len(o)], H[:n_elem], g[:n_elem], dp[:n_elem], info[:n_elem]

    def ba_step_cameras(self, poses, points, obs, bp: BaParams, valid=None):
        """The test seam, one linearisation of every camera: (r float64[n_obs, 2], J float64[n_obs, 2, 6], H float64[n_poses, 6, 6]
        before damping, g and dp float64[n_poses, 6], BA_ELEM_INFO_DTYPE[n_poses])."""
        p, v, x, o = _ba_map(poses, valid, points, obs)
        return self._ba_step(self._lib.lcm_ba_step_cameras, 6, len(p), p, v, x, o, bp)

    def ba_step_points(self, poses, points, obs, bp: BaParams, valid=None):
        """The test seam, one linearisation of every point: (r float64[n_obs, 2], J float64[n_obs, 2, 3], H float64[n_points, 3, 3]
        before damping, g and dp float64[n_points, 3], BA_ELEM_INFO_DTYPE[n_points])."""
        p, v, x, o = _ba_map(poses, valid, points, obs)
        return self._ba_step(self._lib.lcm_ba_step_points, 3, len(x), p, v, x, o, bp)

    def ba_optimize(self, poses, points, obs, bp: BaParams, valid=None):
        """alternatingBundleAdjustment: (PGO_POSE_DTYPE[n_poses], BA_POINT_DTYPE[n_points], BA_ELEM_INFO_DTYPE[n_poses],
        BA_ELEM_INFO_DTYPE[n_points], BaInfo)."""
        p, v, x, o = _ba_map(poses, valid, points, obs)
        po, xo = np.zeros(max(len(p), 1), PGO_POSE_DTYPE), np.zeros(max(len(x), 1), BA_POINT_DTYPE)
        ci, xi = np.zeros(max(len(p), 1), BA_ELEM_INFO_DTYPE), np.zeros(max(len(x), 1), BA_ELEM_INFO_DTYPE)
        info = BaInfo()
        _check(self._lib.lcm_ba_optimize(self._h, _ptr(p), _ptr(v), len(p), _ptr(x), len(x), _ptr(o), len(o), _ref(bp), _ptr(po), _ptr(xo),
                                         _ptr(ci), _ptr(xi), C.byref(info)))
        return po[:len(p)], xo[:len(x)], ci[:len(p)], xi[:len(x)], info

    def ba_outliers(self, poses, points, obs, bp: BaParams, valid=None):
        """The outlier flags: (flags uint8[n_points], max_err float64[n_points], threshold, count)."""
        p, v, x, o = _ba_map(poses, valid, points, obs)
        flags, worst = np.zeros(max(len(x), 1), np.uint8), np.zeros(max(len(x), 1))
        thr, n = C.c_double(-1.0), C.c_int32(-1)
        _check(self._lib.lcm_ba_outliers(self._h, _ptr(p), _ptr(v), len(p), _ptr(x), len(x), _ptr(o), len(o), _ref(bp), _ptr(flags), _ptr(worst),
                                         C.byref(thr), C.byref(n)))
        return flags[:len(x)], worst[:len(x)], thr.value, n.value

    def ba_refine_map(self, poses, points, obs, bp: BaParams, valid=None, second_outer_iters: int = 0):
        """src/main.cpp:1543-1669 in one call: (PGO_POSE_DTYPE[n_poses], BA_POINT_DTYPE[kept], BA_OBS_DTYPE[kept observations],
        old_to_new int32[n_points], BaMapReport)."""
        p, v, x, o = _ba_map(poses, valid, points, obs)
        po, xo, oo = np.zeros(max(len(p), 1), PGO_POSE_DTYPE), np.zeros(max(len(x), 1), BA_POINT_DTYPE), np.zeros(max(len(o), 1), BA_OBS_DTYPE)
        table, rep = np.zeros(max(len(x), 1), np.int32), BaMapReport()
        _check(self._lib.lcm_ba_refine_map(self._h, _ptr(p), _ptr(v), len(p), _ptr(x), len(x), _ptr(o), len(o), _ref(bp), second_outer_iters,
                                           _ptr(po), _ptr(xo), _ptr(oo), _ptr(table), C.byref(rep)))
        return po[:len(p)], xo[:rep.n_points], oo[:rep.n_obs], table[:len(x)], rep

    # -- loop search -------------------------------------------------------------------------------
    # -- before the loop: the map (lcm_map_*) --
    def map_median_displacement(self, pts, offsets) -> np.ndarray:
        """computeMedianDisplacement per pair of host point pairs float32[total, 4] in the offsets layout: float64[n_pairs]."""
        offs = np.ascontiguousarray(offsets, np.uintp)
        n = len(offs) - 1
        p = _point_pairs(pts)
        assert n >= 0 and len(p) >= int(offs[n])
        out = np.zeros(max(n, 1), np.float64)
        _check(self._lib.lcm_map_median_displacement(self._h, _ptr(p), offs.ctypes.data_as(_vp), n, _ptr(out)))
        return out[:n]

    def map_triangulate_pairs(self, pts, offsets, poses1, poses2, mp: MapParams, mask=None):
        """Triangulation and filters of every record of every pair: (MAP_TRI_DTYPE[total], uint8[total] statuses,
        MAP_PAIR_INFO_DTYPE[n_pairs]).  poses1 / poses2: PGO_POSE_DTYPE[n_pairs]; mask: uint8[total] or None (every record)."""
        offs = np.ascontiguousarray(offsets, np.uintp)
        n = len(offs) - 1
        p = _point_pairs(pts)
        total = int(offs[n])
        p1, p2 = np.ascontiguousarray(poses1, PGO_POSE_DTYPE), np.ascontiguousarray(poses2, PGO_POSE_DTYPE)
        k = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        assert len(p) >= total and len(p1) == n and len(p2) == n and (k is None or len(k) >= total)
        tri, status, info = np.zeros(max(total, 1), MAP_TRI_DTYPE), np.zeros(max(total, 1), np.uint8), np.zeros(max(n, 1), MAP_PAIR_INFO_DTYPE)
        _check(self._lib.lcm_map_triangulate_pairs(self._h, _ptr(p), offs.ctypes.data_as(_vp), n, _ptr(k), _ptr(p1), _ptr(p2), _ref(mp),
                                                   _ptr(tri), _ptr(status), _ptr(info)))
        return tri[:total], status[:total], info[:n]

    def map_merge(self, matches, pts, tri, status, kf1: int, kf2: int, table1, table2, n_points: int, cap_points: Optional[int] = None,
                  cap_obs: Optional[int] = None):
        """lcm_map_merge: (BA_POINT_DTYPE[n_new], BA_OBS_DTYPE[2 n_new + n_merged], uint8[n] statuses, n_new, n_merged); table1 and
        table2 (int32, C-contiguous) are updated in place."""
        m = np.ascontiguousarray(matches, DMATCH_DTYPE)
        n = len(m)
        p, t, s = _point_pairs(pts), np.ascontiguousarray(tri, MAP_TRI_DTYPE), np.ascontiguousarray(status, np.uint8)
        assert len(p) == n and len(t) == n and len(s) == n
        for tab in (table1, table2):
            assert tab.dtype == np.int32 and tab.flags["C_CONTIGUOUS"]
        cp, co = n if cap_points is None else cap_points, 2 * n if cap_obs is None else cap_obs
        points, obs, out = np.zeros(max(cp, 1), BA_POINT_DTYPE), np.zeros(max(co, 1), BA_OBS_DTYPE), np.zeros(max(n, 1), np.uint8)
        a, b = C.c_int32(0), C.c_int32(0)
        _check(self._lib.lcm_map_merge(self._h, _ptr(m), _ptr(p), _ptr(t), _ptr(s), n, kf1, kf2, _ptr(table1), len(table1), _ptr(table2),
                                       len(table2), n_points, _ptr(points), cp, _ptr(obs), co, _ptr(out), C.byref(a), C.byref(b)))
        return points[:a.value], obs[:2 * a.value + b.value], out[:n], a.value, b.value

    def map_add_keyframe(self, matches, pts, kf_last: int, pose_last, table_last, kf_new: int, table_new, n_points: int, mp: MapParams,
                         ep: EpiParams, lp: Optional[LoParams] = None, pp: Optional[PoseParams] = None, cap_points: Optional[int] = None,
                         cap_obs: Optional[int] = None):
        """lcm_map_add_keyframe: (MapKeyframeReport, BA_POINT_DTYPE[n_new], BA_OBS_DTYPE[new observations], uint8[n] statuses); the
        tables (int32, C-contiguous) are updated in place when the verdict is MAP_KEYFRAME.  pose_last: PGO_POSE_DTYPE[1]."""
        m = np.ascontiguousarray(matches, DMATCH_DTYPE)
        n = len(m)
        p, pose = _point_pairs(pts), np.ascontiguousarray(pose_last, PGO_POSE_DTYPE).reshape(1)
        assert len(p) == n
        for tab in (table_last, table_new):
            assert tab.dtype == np.int32 and tab.flags["C_CONTIGUOUS"]
        cp, co = n if cap_points is None else cap_points, 2 * n if cap_obs is None else cap_obs
        points, obs, out = np.zeros(max(cp, 1), BA_POINT_DTYPE), np.zeros(max(co, 1), BA_OBS_DTYPE), np.zeros(max(n, 1), np.uint8)
        rep = MapKeyframeReport()
        _check(self._lib.lcm_map_add_keyframe(self._h, _ptr(m), _ptr(p), n, kf_last, _ptr(pose), _ptr(table_last), len(table_last), kf_new,
                                              _ptr(table_new), len(table_new), n_points, _ref(mp), _ref(ep), _ref(lp), _ref(pp), _ptr(points),
                                              cp, _ptr(obs), co, _ptr(out), C.byref(rep)))
        return rep, points[:rep.n_new], obs[:2 * rep.n_new + rep.n_merged], out[:n]

    def map_db_track(self, last_slot: int, curr_slot: int, ratio: float, kf_last: int, pose_last, table_last, kf_new: int, table_new,
                     n_points: int, mp: MapParams, ep: EpiParams, lp: Optional[LoParams] = None, pp: Optional[PoseParams] = None,
                     cap: Optional[int] = None):
        """lcm_map_db_track on the stored pair (last_slot, curr_slot): (lists, report, points, observations, statuses) where lists is
        the dict of lcm_pose_db_verify_pairs's outputs (results, pose_results, info, out, pts, mask, pose_mask, offsets)."""
        cap = self.l2_db_rows(last_slot) if cap is None else cap
        pose = np.ascontiguousarray(pose_last, PGO_POSE_DTYPE).reshape(1)
        for tab in (table_last, table_new):
            assert tab.dtype == np.int32 and tab.flags["C_CONTIGUOUS"]
        res, pres, info = np.zeros(1, EPI_RESULT_DTYPE), np.zeros(1, POSE_RESULT_DTYPE), np.zeros(1, LO_INFO_DTYPE)
        out, pts = np.zeros(max(cap, 1), DMATCH_DTYPE), np.zeros((max(cap, 1), 4), np.float32)
        mask, pmask = np.zeros(max(cap, 1), np.uint8), np.zeros(max(cap, 1), np.uint8)
        offs = np.zeros(2, np.uintp)
        points, obs, status = np.zeros(max(cap, 1), BA_POINT_DTYPE), np.zeros(max(2 * cap, 1), BA_OBS_DTYPE), np.zeros(max(cap, 1), np.uint8)
        rep = MapKeyframeReport()
        _check(self._lib.lcm_map_db_track(self._h, last_slot, curr_slot, ratio, _ref(ep), _ref(lp), _ref(pp), _ptr(res), _ptr(info), _ptr(pres),
                                          _ptr(out), _ptr(pts), _ptr(mask), _ptr(pmask), cap, offs.ctypes.data_as(_vp), kf_last, _ptr(pose),
                                          _ptr(table_last), kf_new, _ptr(table_new), n_points, _ref(mp), _ptr(points), cap, _ptr(obs), 2 * cap,
                                          _ptr(status), C.byref(rep)))
        n = int(offs[1])
        lists = dict(results=res, pose_results=pres, info=info, out=out[:n], pts=pts[:n], mask=mask[:n], pose_mask=pmask[:n], offsets=offs)
        return lists, rep, points[:rep.n_new], obs[:2 * rep.n_new + rep.n_merged], status[:n]

    # -- the front end: SIFT keypoints (lcm_sift_*) --
    def sift_space(self, max_w: int, max_h: int, sp: Optional[SiftParams] = None) -> "SiftSpace":
        """lcm_sift_space_create: a scale space for images of up to max_w x max_h; close it before the matcher."""
        return SiftSpace(self, max_w, max_h, sp)

    def sift_detect_image(self, img, sp: Optional[SiftParams] = None, cap: int = 1 << 16) -> np.ndarray:
        """lcm_sift_detect_image: SIFT_KEYPOINT_DTYPE[n] of a uint8 gray image, on a space cached in the handle."""
        a = _gray(img)
        kp, n = np.zeros(max(cap, 1), SIFT_KEYPOINT_DTYPE), C.c_size_t(0)
        _check(self._lib.lcm_sift_detect_image(self._h, a.ctypes.data_as(_vp), a.shape[1], a.shape[0], a.strides[0], _ref(sp), _ptr(kp), cap,
                                               C.byref(n)))
        return kp[:n.value]

    def query_scores(self, query, query_frame_id: int) -> Tuple[np.ndarray, np.ndarray]:
        q = _rows(query)
        cap = max(len(self), 1)
        scores = np.zeros(cap, SCORE_DTYPE)
        ids = np.zeros(cap, np.int32)
        n = C.c_int32(0)
        _check(self._lib.lcm_query_scores(self._h, _ptr(q), q.shape[0], query_frame_id, scores.ctypes.data_as(_vp),
                                          ids.ctypes.data_as(_vp), C.byref(n)))
        return scores[: n.value], ids[: n.value]

    def query_scores_ratio(self, query, query_frame_id: int, ratio: float) -> Tuple[np.ndarray, np.ndarray]:
        """query_scores with good_count = number of rows that pass Lowe's ratio test (knnMatch(k=2), best < ratio *
        second) against each eligible stored frame: (records, stored frame ids)."""
        q = _rows(query)
        cap = max(len(self), 1)
        scores = np.zeros(cap, SCORE_DTYPE)
        ids = np.zeros(cap, np.int32)
        n = C.c_int32(0)
        _check(self._lib.lcm_query_scores_ratio(self._h, _ptr(q), q.shape[0], query_frame_id, ratio,
                                                scores.ctypes.data_as(_vp), ids.ctypes.data_as(_vp), C.byref(n)))
        return scores[: n.value], ids[: n.value]

    def query_submit(self, query, query_frame_id: int) -> int:
        """Asynchronous query: returns a ticket at once (the rows are copied before returning)."""
        q = _rows(query)
        t = C.c_int32(-1)
        _check(self._lib.lcm_query_submit(self._h, _ptr(q), q.shape[0], query_frame_id, C.byref(t)))
        return t.value

    def query_collect(self, ticket: int, cap: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        cap = max(len(self), 1) if cap is None else cap
        scores = np.zeros(cap, SCORE_DTYPE)
        ids = np.zeros(cap, np.int32)
        n = C.c_int32(0)
        _check(self._lib.lcm_query_collect(self._h, ticket, scores.ctypes.data_as(_vp), ids.ctypes.data_as(_vp), cap,
                                           C.byref(n)))
        return scores[: n.value], ids[: n.value]

    def query_submit_batch(self, queries: Sequence[np.ndarray], query_frame_ids: Sequence[int]) -> int:
        """Up to 16 query frames scored by ONE launch against the database as it stands now; returns one ticket."""
        qs = [_rows(q) for q in queries]
        B = len(qs)
        ptrs = (_vp * B)(*[q.ctypes.data if q.shape[0] else None for q in qs])
        nq = np.array([q.shape[0] for q in qs], np.int32)
        ids = np.ascontiguousarray(query_frame_ids, np.int32)
        assert ids.shape[0] == B
        t = C.c_int32(-1)
        _check(self._lib.lcm_query_submit_batch(self._h, ptrs, nq.ctypes.data_as(_i32p), ids.ctypes.data_as(_i32p), B,
                                                C.byref(t)))
        self._batch_sizes = getattr(self, "_batch_sizes", {})
        self._batch_sizes[t.value] = B
        return t.value

    def query_collect_batch(self, ticket: int, cap: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(records of all the batch's queries back to back, offsets[B + 1])."""
        B = self._batch_sizes[ticket]
        cap = max(len(self), 1) * B if cap is None else cap
        scores = np.zeros(max(cap, 1), SCORE_DTYPE)
        offs = np.zeros(B + 1, np.uintp)
        n = C.c_size_t(0)
        _check(self._lib.lcm_query_collect_batch(self._h, ticket, scores.ctypes.data_as(_vp), cap, C.byref(n),
                                                 offs.ctypes.data_as(_vp)))
        return scores[: n.value], offs

    def online_stats(self, reset: bool = False) -> OnlineStats:
        st = OnlineStats()
        _check(self._lib.lcm_online_stats_read(self._h, C.byref(st), 1 if reset else 0))
        return st

    def detect_loops(self, current_frame_id: int, query=None, n_keypoints: int = -1) -> np.ndarray:
        cap = max(len(self), 1)
        out = np.zeros(cap, CANDIDATE_DTYPE)
        n = C.c_int32(0)
        if query is None:
            qp, nq = None, 0
        else:
            q = _rows(query)
            nq = q.shape[0]
            # an explicit empty frame still needs a non-NULL pointer to be told apart from "use the stored frame"
            qp = q.ctypes.data_as(_vp) if nq else np.zeros((1, DESC_BYTES), np.uint8).ctypes.data_as(_vp)
        _check(self._lib.lcm_detect_loops(self._h, current_frame_id, qp, nq, n_keypoints, out.ctypes.data_as(_vp), cap,
                                          C.byref(n)))
        return out[: n.value]

    def loop_test(self, score, n_query_kp: int, n_train_kp: int) -> Tuple[bool, float]:
        s = Score(int(score["good_count"]), int(score["min_dist"]), int(score["n_train"]))
        p = self.params
        sim = C.c_double(0)
        r = self._lib.lcm_loop_test(C.byref(p), C.byref(s), n_query_kp, n_train_kp, C.byref(sim))
        return bool(r), sim.value

    # -- bulk --------------------------------------------------------------------------------------
    def all_vs_all_plan(self, d_query_rows: int = 0, d_query_counts: int = 0, q_ids: Optional[Sequence[int]] = None,
                        q_stride_rows: int = 0) -> Tuple[int, np.ndarray]:
        """Sizing call: returns (n_pairs, offsets[n_q_frames + 1])."""
        ids = None if q_ids is None else np.ascontiguousarray(q_ids, np.int32)
        nq = len(self) if ids is None else ids.shape[0]
        offs = np.zeros(nq + 1, np.uintp)
        n = C.c_size_t(0)
        _check(self._lib.lcm_all_vs_all(self._h, _vp(d_query_rows) if d_query_rows else None,
                                        _vp(d_query_counts) if d_query_counts else None, _ptr(ids), nq, q_stride_rows,
                                        None, 0, C.byref(n), offs.ctypes.data_as(_vp)))
        return n.value, offs

    def all_vs_all(self, d_scores: int, scores_cap: int, d_query_rows: int = 0, d_query_counts: int = 0,
                   q_ids: Optional[Sequence[int]] = None, q_stride_rows: int = 0) -> int:
        """Enqueue the bulk scoring on the handle's stream; scores land in device memory at d_scores."""
        ids = None if q_ids is None else np.ascontiguousarray(q_ids, np.int32)
        nq = len(self) if ids is None else ids.shape[0]
        n = C.c_size_t(0)
        _check(self._lib.lcm_all_vs_all(self._h, _vp(d_query_rows) if d_query_rows else None,
                                        _vp(d_query_counts) if d_query_counts else None, _ptr(ids), nq, q_stride_rows,
                                        _vp(d_scores), scores_cap, C.byref(n), None))
        return n.value

    def all_vs_all_argmin(self, d_scores: int, scores_cap: int, d_index_sums: int, d_query_rows: int = 0,
                          d_query_counts: int = 0, q_ids: Optional[Sequence[int]] = None, q_stride_rows: int = 0) -> int:
        """all_vs_all through the argmin kernel; d_index_sums receives one uint32 per pair (sum of the good matches'
        train indices mod 2^32)."""
        ids = None if q_ids is None else np.ascontiguousarray(q_ids, np.int32)
        nq = len(self) if ids is None else ids.shape[0]
        n = C.c_size_t(0)
        _check(self._lib.lcm_all_vs_all_argmin(self._h, _vp(d_query_rows) if d_query_rows else None,
                                               _vp(d_query_counts) if d_query_counts else None, _ptr(ids), nq,
                                               q_stride_rows, _vp(d_scores), scores_cap, _vp(d_index_sums),
                                               C.byref(n), None))
        return n.value

    def all_vs_all_ratio_plan(self, ratio: float, d_query_rows: int = 0, d_query_counts: int = 0,
                              q_ids: Optional[Sequence[int]] = None, q_stride_rows: int = 0) -> Tuple[int, np.ndarray]:
        """Sizing call of all_vs_all_ratio: returns (n_pairs, offsets[n_q_frames + 1])."""
        ids = None if q_ids is None else np.ascontiguousarray(q_ids, np.int32)
        nq = len(self) if ids is None else ids.shape[0]
        offs = np.zeros(nq + 1, np.uintp)
        n = C.c_size_t(0)
        _check(self._lib.lcm_all_vs_all_ratio(self._h, _vp(d_query_rows) if d_query_rows else None,
                                              _vp(d_query_counts) if d_query_counts else None, _ptr(ids), nq,
                                              q_stride_rows, ratio, None, 0, C.byref(n), offs.ctypes.data_as(_vp)))
        return n.value, offs

    def all_vs_all_ratio(self, ratio: float, d_scores: int, scores_cap: int, d_query_rows: int = 0,
                         d_query_counts: int = 0, q_ids: Optional[Sequence[int]] = None, q_stride_rows: int = 0) -> int:
        """all_vs_all with the reference's loop-search score: good_count = number of query rows that pass Lowe's ratio
        test (knnMatch(k=2), best < ratio * second).  Enqueued on the handle's stream; records land at d_scores."""
        ids = None if q_ids is None else np.ascontiguousarray(q_ids, np.int32)
        nq = len(self) if ids is None else ids.shape[0]
        n = C.c_size_t(0)
        _check(self._lib.lcm_all_vs_all_ratio(self._h, _vp(d_query_rows) if d_query_rows else None,
                                              _vp(d_query_counts) if d_query_counts else None, _ptr(ids), nq,
                                              q_stride_rows, ratio, _vp(d_scores), scores_cap, C.byref(n), None))
        return n.value

    def all_vs_all_loops(self, cap: int = 1 << 20, d_query_rows: int = 0, d_query_counts: int = 0,
                         q_ids: Optional[Sequence[int]] = None, q_keypoints: Optional[Sequence[int]] = None,
                         q_stride_rows: int = 0, out: Optional[np.ndarray] = None) -> Tuple[np.ndarray, int]:
        """Bulk loop search with the loop test fused on the device: (candidates sorted by (current, matched), n_pairs)."""
        ids = None if q_ids is None else np.ascontiguousarray(q_ids, np.int32)
        kps = None if q_keypoints is None else np.ascontiguousarray(q_keypoints, np.int32)
        nq = len(self) if ids is None else ids.shape[0]
        if out is None:
            out = np.zeros(max(cap, 1), CANDIDATE_DTYPE)
        else:
            assert out.dtype == CANDIDATE_DTYPE and out.flags["C_CONTIGUOUS"]
            cap = len(out)
        n, npairs = C.c_size_t(0), C.c_size_t(0)
        _check(self._lib.lcm_all_vs_all_loops(self._h, _vp(d_query_rows) if d_query_rows else None,
                                              _vp(d_query_counts) if d_query_counts else None, _ptr(ids), _ptr(kps), nq,
                                              q_stride_rows, out.ctypes.data_as(_vp), cap, C.byref(n), C.byref(npairs)))
        return out[: n.value], npairs.value

    def all_vs_all_loops_ratio(self, ratio: Optional[float] = None, min_rows: Optional[int] = None,
                               min_matches: Optional[int] = None, cap: int = 1 << 20, d_query_rows: int = 0,
                               d_query_counts: int = 0, q_ids: Optional[Sequence[int]] = None, q_stride_rows: int = 0,
                               out: Optional[np.ndarray] = None) -> Tuple[np.ndarray, int]:
        """The reference's loop search (src/main.cpp:1375-1388) in one call: ratio-test scores + `rows >= min_rows` on both
        frames + `good_count >= min_matches`, decided and compacted on the device: (candidates sorted by (current,
        matched), n_pairs).  ratio / min_rows / min_matches left at None: 0.7 / 100 / 300 (all three None: rp = NULL)."""
        rp = _ratio_loop_params(ratio, min_rows, min_matches)
        ids = None if q_ids is None else np.ascontiguousarray(q_ids, np.int32)
        nq = len(self) if ids is None else ids.shape[0]
        if out is None:
            out = np.zeros(max(cap, 1), CANDIDATE_DTYPE)
        else:
            assert out.dtype == CANDIDATE_DTYPE and out.flags["C_CONTIGUOUS"]
            cap = len(out)
        n, npairs = C.c_size_t(0), C.c_size_t(0)
        _check(self._lib.lcm_all_vs_all_loops_ratio(self._h, _vp(d_query_rows) if d_query_rows else None,
                                                    _vp(d_query_counts) if d_query_counts else None, _ptr(ids), nq,
                                                    q_stride_rows, None if rp is None else C.byref(rp),
                                                    out.ctypes.data_as(_vp), cap, C.byref(n), C.byref(npairs)))
        return out[: n.value], npairs.value

    def detect_loops_ratio(self, current_frame_id: int, query=None, ratio: Optional[float] = None,
                           min_rows: Optional[int] = None, min_matches: Optional[int] = None,
                           cap: Optional[int] = None) -> np.ndarray:
        """One frame of all_vs_all_loops_ratio: `query` (host rows), or the stored frame with that id (query=None, its
        rows used in place on the device), against every eligible stored frame."""
        rp = _ratio_loop_params(ratio, min_rows, min_matches)
        cap = max(len(self), 1) if cap is None else cap
        out = np.zeros(max(cap, 1), CANDIDATE_DTYPE)
        n = C.c_int32(0)
        if query is None:
            qp, nq = None, 0
        else:
            q = _rows(query)
            nq = q.shape[0]
            # an explicit empty frame still needs a non-NULL pointer to be told apart from "use the stored frame"
            qp = q.ctypes.data_as(_vp) if nq else np.zeros((1, DESC_BYTES), np.uint8).ctypes.data_as(_vp)
        _check(self._lib.lcm_detect_loops_ratio(self._h, current_frame_id, qp, nq, None if rp is None else C.byref(rp),
                                                out.ctypes.data_as(_vp), cap, C.byref(n)))
        return out[: n.value]

    def last_bulk_scores(self) -> np.ndarray:
        """Download the score records the last all_vs_all_loops call left on the device."""
        p, n = _vp(), C.c_size_t(0)
        _check(self._lib.lcm_last_bulk_scores(self._h, C.byref(p), C.byref(n)))
        out = np.zeros(n.value, SCORE_DTYPE)
        if n.value:
            self.sync()
            self.dev_download(p.value, out)
        return out

    def merge_shards_device(self, d_gathered: int, shard_counts: Sequence[int], ids, min_gap: int, d_merged: int, cap: int) -> int:
        world = len(shard_counts)
        counts = (C.c_size_t * world)(*[int(c) for c in shard_counts])
        ids = np.ascontiguousarray(ids, np.int32)
        n = C.c_size_t(0)
        _check(self._lib.lcm_merge_shard_scores_device(self._h, _vp(d_gathered), counts, world, _ptr(ids), len(ids), min_gap,
                                                       _vp(d_merged), cap, C.byref(n)))
        return n.value

    def launch_info(self) -> LaunchInfo:
        info = LaunchInfo()
        _check(self._lib.lcm_last_launch_info(self._h, C.byref(info)))
        return info

    # -- device scratch ----------------------------------------------------------------------------
    def dev_alloc(self, nbytes: int) -> int:
        p = _vp()
        _check(self._lib.lcm_dev_alloc(self._h, nbytes, C.byref(p)))
        return p.value

    def dev_free(self, d_ptr: int):
        _check(self._lib.lcm_dev_free(self._h, _vp(d_ptr)))

    def dev_upload(self, d_ptr: int, arr: np.ndarray):
        a = np.ascontiguousarray(arr)
        _check(self._lib.lcm_dev_upload(self._h, _vp(d_ptr), a.ctypes.data_as(_vp), a.nbytes))

    def dev_download(self, d_ptr: int, out: np.ndarray):
        assert out.flags["C_CONTIGUOUS"]
        _check(self._lib.lcm_dev_download(self._h, out.ctypes.data_as(_vp), _vp(d_ptr), out.nbytes))


class SiftSpace:
    """A lcm_sift_space: the Gaussian and DoG pyramid of one image at a time, on the device."""

    def __init__(self, matcher: Matcher, max_w: int, max_h: int, sp: Optional[SiftParams] = None):
        self._lib, self._m, self._s = matcher._lib, matcher, _vp()
        _check(self._lib.lcm_sift_space_create(matcher._h, max_w, max_h, _ref(sp), C.byref(self._s)))

    def close(self):
        if self._s:
            self._lib.lcm_sift_space_destroy(self._s)
            self._s = _vp()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def build(self, img):
        a = _gray(img)
        _check(self._lib.lcm_sift_space_build(self._s, a.ctypes.data_as(_vp), a.shape[1], a.shape[0], a.strides[0]))

    def info(self) -> SiftSpaceInfo:
        out = SiftSpaceInfo()
        _check(self._lib.lcm_sift_space_info(self._s, C.byref(out)))
        return out

    def read(self, kind: int, octave: int, layer: int) -> np.ndarray:
        pl = self.info().plan
        if not 0 <= octave < max(pl.n_octaves, 1):
            raise LcmError(-1, "no such octave")
        out = np.zeros((pl.height[octave], pl.width[octave]), np.float32)
        _check(self._lib.lcm_sift_space_read(self._s, kind, octave, layer, _ptr(out)))
        return out

    def write(self, kind: int, octave: int, layer: int, values):
        pl = self.info().plan
        a = np.ascontiguousarray(values, np.float32)
        assert 0 <= octave < pl.n_octaves and a.shape == (pl.height[octave], pl.width[octave])
        _check(self._lib.lcm_sift_space_write(self._s, kind, octave, layer, _ptr(a)))

    def extrema(self, cap: Optional[int] = None, out: Optional[np.ndarray] = None) -> np.ndarray:
        """lcm_sift_extrema: SIFT_CANDIDATE_DTYPE[n], in (octave, layer, row, col) order."""
        cap = int(self.info().candidate_capacity) if cap is None else cap
        out, n = np.zeros(max(cap, 1), SIFT_CANDIDATE_DTYPE) if out is None else out, C.c_size_t(0)
        _check(self._lib.lcm_sift_extrema(self._s, _ptr(out), cap, C.byref(n)))
        return out[:n.value]

    def detect(self, cap: Optional[int] = None, out: Optional[np.ndarray] = None) -> Tuple[np.ndarray, int]:
        """lcm_sift_detect: (SIFT_KEYPOINT_DTYPE[n], the candidates' number)."""
        cap = int(self.info().candidate_capacity) if cap is None else cap
        kp = np.zeros(max(cap, 1), SIFT_KEYPOINT_DTYPE) if out is None else out
        n, nc = C.c_size_t(0), C.c_size_t(0)
        _check(self._lib.lcm_sift_detect(self._s, _ptr(kp), cap, C.byref(n), C.byref(nc)))
        return kp[:n.value], nc.value


def merge_shard_scores_host(shard_scores: Sequence[np.ndarray], ids, min_gap: int) -> Tuple[np.ndarray, np.ndarray]:
    """lcm_merge_shard_scores (host-only C function): W per-shard arrays -> (merged, offsets[n_frames + 1])."""
    lib = load_library()
    world = len(shard_scores)
    arrs = [np.ascontiguousarray(a, SCORE_DTYPE) for a in shard_scores]
    ptrs = (_vp * world)(*[a.ctypes.data if a.size else None for a in arrs])
    counts = (C.c_size_t * world)(*[len(a) for a in arrs])
    ids = np.ascontiguousarray(ids, np.int32)
    n = C.c_size_t(0)
    offs = np.zeros(len(ids) + 1, np.uintp)
    _check(lib.lcm_merge_shard_scores(ptrs, counts, world, _ptr(ids), len(ids), min_gap, None, 0, C.byref(n),
                                      offs.ctypes.data_as(_vp)))
    out = np.zeros(max(n.value, 1), SCORE_DTYPE)
    _check(lib.lcm_merge_shard_scores(ptrs, counts, world, _ptr(ids), len(ids), min_gap, out.ctypes.data_as(_vp),
                                      len(out), C.byref(n), None))
    return out[: n.value], offs


class Group:
    """lcm_group: one process, W devices, stored frames sharded cyclically by arrival position, RCCL inside."""

    def __init__(self, params: Optional[Params] = None, n_devices: int = 1, device_ids: Optional[Sequence[int]] = None,
                 loopback_device: Optional[int] = None, peer_copies: bool = False):
        """loopback_device: rehearsal form — n_devices shards on that ONE device, exchange steps as device-local copies.
        peer_copies: a real group whose exchange steps are device-to-device copies instead of RCCL calls."""
        self._lib = load_library()
        self._g = _vp()
        p = params if params is not None else default_params()
        if loopback_device is not None:
            _check(self._lib.lcm_group_create_loopback(C.byref(p), n_devices, loopback_device, C.byref(self._g)))
            return
        ids = None if device_ids is None else np.ascontiguousarray(device_ids, np.int32)
        create = self._lib.lcm_group_create_peer if peer_copies else self._lib.lcm_group_create
        _check(create(C.byref(p), n_devices, None if ids is None else ids.ctypes.data_as(_i32p), C.byref(self._g)))

    @property
    def transport(self) -> str:
        return self._lib.lcm_group_transport(self._g).decode()

    def close(self):
        if getattr(self, "_g", None):
            self._lib.lcm_group_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self):
        return self._lib.lcm_group_db_size(self._g)

    @property
    def world(self) -> int:
        return self._lib.lcm_group_size(self._g)

    def set_params(self, p: Params):
        _check(self._lib.lcm_group_set_params(self._g, C.byref(p)))

    def reserve(self, n_frames: int, max_desc: int):
        _check(self._lib.lcm_group_reserve(self._g, n_frames, max_desc))

    def append(self, frame_id: int, desc, n_keypoints: int = -1):
        d = _rows(desc)
        _check(self._lib.lcm_group_append(self._g, frame_id, _ptr(d), d.shape[0], n_keypoints))

    def clear(self):
        _check(self._lib.lcm_group_clear(self._g))

    def all_vs_all(self) -> Tuple[np.ndarray, np.ndarray]:
        """(merged scores in (query asc, stored asc) order, offsets[len + 1])."""
        n = C.c_size_t(0)
        offs = np.zeros(len(self) + 1, np.uintp)
        _check(self._lib.lcm_group_all_vs_all(self._g, None, 0, C.byref(n), offs.ctypes.data_as(_vp)))
        out = np.zeros(max(n.value, 1), SCORE_DTYPE)
        _check(self._lib.lcm_group_all_vs_all(self._g, out.ctypes.data_as(_vp), len(out), C.byref(n), None))
        return out[: n.value], offs

    def all_vs_all_ratio(self, ratio: float) -> Tuple[np.ndarray, np.ndarray]:
        """all_vs_all with the ratio-test score (lcm_group_all_vs_all_ratio): (merged scores, offsets[len + 1])."""
        n = C.c_size_t(0)
        offs = np.zeros(len(self) + 1, np.uintp)
        _check(self._lib.lcm_group_all_vs_all_ratio(self._g, ratio, None, 0, C.byref(n), offs.ctypes.data_as(_vp)))
        out = np.zeros(max(n.value, 1), SCORE_DTYPE)
        _check(self._lib.lcm_group_all_vs_all_ratio(self._g, ratio, out.ctypes.data_as(_vp), len(out), C.byref(n), None))
        return out[: n.value], offs

    def all_vs_all_loops_ratio(self, ratio: Optional[float] = None, min_rows: Optional[int] = None,
                               min_matches: Optional[int] = None, cap: int = 1 << 20,
                               out: Optional[np.ndarray] = None) -> Tuple[np.ndarray, int]:
        """(loop candidates of the reference's rule in (current, matched) order, pairs scored) —
        lcm_group_all_vs_all_loops_ratio; parameters as Matcher.all_vs_all_loops_ratio."""
        rp = _ratio_loop_params(ratio, min_rows, min_matches)
        if out is None:
            out = np.zeros(max(cap, 1), CANDIDATE_DTYPE)
        n, npairs = C.c_size_t(0), C.c_size_t(0)
        _check(self._lib.lcm_group_all_vs_all_loops_ratio(self._g, None if rp is None else C.byref(rp), out.ctypes.data_as(_vp),
                                                          len(out), C.byref(n), C.byref(npairs)))
        return out[: n.value], npairs.value

    def truncate(self, n_frames: int):
        _check(self._lib.lcm_group_truncate(self._g, n_frames))

    def save(self, path: str):
        _check(self._lib.lcm_group_save(self._g, path.encode()))

    def load(self, path: str):
        _check(self._lib.lcm_group_load(self._g, path.encode()))

    def sync(self):
        _check(self._lib.lcm_group_sync(self._g))

    def set_tuning(self, knob: int, value: int):
        _check(self._lib.lcm_group_set_tuning(self._g, knob, value))

    def set_kernel_variant(self, v: int):
        _check(self._lib.lcm_group_set_kernel_variant(self._g, v))

    def all_vs_all_argmin(self, out: Optional[np.ndarray] = None, out_idx: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(merged scores, merged per-pair index checksums, offsets[len + 1]) — lcm_group_all_vs_all_argmin.
        `out` / `out_idx`: reusable host buffers (SCORE_DTYPE / uint32) of at least the pair count."""
        n = C.c_size_t(0)
        offs = np.zeros(len(self) + 1, np.uintp)
        _check(self._lib.lcm_group_all_vs_all_argmin(self._g, None, None, 0, C.byref(n), offs.ctypes.data_as(_vp)))
        if out is None or len(out) < n.value:
            out = np.zeros(max(n.value, 1), SCORE_DTYPE)
        if out_idx is None or len(out_idx) < n.value:
            out_idx = np.zeros(max(n.value, 1), np.uint32)
        _check(self._lib.lcm_group_all_vs_all_argmin(self._g, out.ctypes.data_as(_vp), out_idx.ctypes.data_as(_vp),
                                                     min(len(out), len(out_idx)), C.byref(n), None))
        return out[: n.value], out_idx[: n.value], offs

    def all_vs_all_loops(self, cap: int = 1 << 20, out: Optional[np.ndarray] = None) -> Tuple[np.ndarray, int]:
        """(loop candidates in (current, matched) order, pairs scored) — lcm_group_all_vs_all_loops."""
        if out is None:
            out = np.zeros(max(cap, 1), CANDIDATE_DTYPE)
        n, npairs = C.c_size_t(0), C.c_size_t(0)
        _check(self._lib.lcm_group_all_vs_all_loops(self._g, out.ctypes.data_as(_vp), len(out), C.byref(n), C.byref(npairs)))
        return out[: n.value], npairs.value

    def query_submit_batch(self, queries: Sequence[np.ndarray], query_frame_ids: Sequence[int]) -> int:
        qs = [_rows(q) for q in queries]
        B = len(qs)
        ptrs = (_vp * B)(*[q.ctypes.data if q.shape[0] else None for q in qs])
        nq = np.array([q.shape[0] for q in qs], np.int32)
        ids = np.ascontiguousarray(query_frame_ids, np.int32)
        t = C.c_int32(-1)
        _check(self._lib.lcm_group_query_submit_batch(self._g, ptrs, nq.ctypes.data_as(_i32p), ids.ctypes.data_as(_i32p), B, C.byref(t)))
        return t.value

    def query_collect_batch(self, ticket: int, cap: int, n_queries: int = 16) -> Tuple[np.ndarray, np.ndarray]:
        scores = np.zeros(max(cap, 1), SCORE_DTYPE)
        offs = np.zeros(n_queries + 1, np.uintp)
        n = C.c_size_t(0)
        _check(self._lib.lcm_group_query_collect_batch(self._g, ticket, scores.ctypes.data_as(_vp), len(scores), C.byref(n),
                                                       offs.ctypes.data_as(_vp)))
        return scores[: n.value], offs

    def online_stats(self, reset: bool = False) -> OnlineStats:
        st = OnlineStats()
        _check(self._lib.lcm_group_online_stats_read(self._g, C.byref(st), 1 if reset else 0))
        return st

    def shard_launch_info(self, rank: int) -> LaunchInfo:
        """lcm_last_launch_info of shard `rank`'s own matcher (its last bulk launch: route, chunks, per-launch times)."""
        h = _vp()
        _check(self._lib.lcm_group_handle(self._g, rank, C.byref(h)))
        info = LaunchInfo()
        _check(self._lib.lcm_last_launch_info(h, C.byref(info)))
        return info

    def info(self) -> GroupInfo:
        gi = GroupInfo()
        _check(self._lib.lcm_group_last_info(self._g, C.byref(gi)))
        return gi

    def query_scores(self, query, query_frame_id: int) -> Tuple[np.ndarray, np.ndarray]:
        q = _rows(query)
        cap = max(len(self), 1)
        scores = np.zeros(cap, SCORE_DTYPE)
        ids = np.zeros(cap, np.int32)
        n = C.c_int32(0)
        _check(self._lib.lcm_group_query_scores(self._g, _ptr(q), q.shape[0], query_frame_id, scores.ctypes.data_as(_vp),
                                                ids.ctypes.data_as(_vp), cap, C.byref(n)))
        return scores[: n.value], ids[: n.value]

    def query_scores_batch(self, queries: Sequence[np.ndarray], query_frame_ids: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
        qs = [_rows(q) for q in queries]
        B = len(qs)
        ptrs = (_vp * B)(*[q.ctypes.data if q.shape[0] else None for q in qs])
        nq = np.array([q.shape[0] for q in qs], np.int32)
        ids = np.ascontiguousarray(query_frame_ids, np.int32)
        cap = max(len(self), 1) * B
        scores = np.zeros(cap, SCORE_DTYPE)
        offs = np.zeros(B + 1, np.uintp)
        n = C.c_size_t(0)
        _check(self._lib.lcm_group_query_scores_batch(self._g, ptrs, nq.ctypes.data_as(_i32p), ids.ctypes.data_as(_i32p), B,
                                                      scores.ctypes.data_as(_vp), cap, C.byref(n), offs.ctypes.data_as(_vp)))
        return scores[: n.value], offs

    def detect_loops(self, current_frame_id: int, query, n_keypoints: int = -1) -> np.ndarray:
        q = _rows(query)
        cap = max(len(self), 1)
        out = np.zeros(cap, CANDIDATE_DTYPE)
        n = C.c_int32(0)
        qp = q.ctypes.data_as(_vp) if q.shape[0] else np.zeros((1, DESC_BYTES), np.uint8).ctypes.data_as(_vp)
        _check(self._lib.lcm_group_detect_loops(self._g, current_frame_id, qp, q.shape[0], n_keypoints,
                                                out.ctypes.data_as(_vp), cap, C.byref(n)))
        return out[: n.value]


# ---------------------------------------------------------------------------------------------------------
# include/lcm_host.h: the C shim over the C++ host class loop_closing::LoopClosingSystem
# ---------------------------------------------------------------------------------------------------------
_HOST_SIGNATURES = {
    "lcs_create": (C.c_int, [C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_vp)]),
    "lcs_create_group": (C.c_int, [C.c_double, C.c_int, C.c_int, _i32p, C.c_int, C.POINTER(_vp)]),
    "lcs_destroy": (None, [_vp]),
    "lcs_process_frame": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int]),
    "lcs_process_frames": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int]),
    "lcs_match_features": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int, _i32p]),
    "lcs_detect_loops": (C.c_int, [_vp, C.c_int, _vp, C.c_int, _i32p]),
    "lcs_get_consecutive_matches": (C.c_int, [_vp, _vp, C.c_int, _i32p]),
    "lcs_match_loop_closures": (C.c_int, [_vp, C.c_int, _vp, C.c_size_t, _vp, C.c_int, _i32p]),
    "lcs_set_gap_by_position": (C.c_int, [_vp, C.c_int]),
    "lcs_num_frames": (C.c_int, [_vp]),
    "lcs_num_loop_closures": (C.c_int, [_vp]),
    "lcs_get_loop_closures": (C.c_int, [_vp, _vp, C.c_int, _i32p]),
    "lcs_save_results": (C.c_int, [_vp, C.c_char_p]),
}


class LoopClosingSystem:
    """Python handle on the C++ loop_closing::LoopClosingSystem (csrc/loop_closing_system.hpp) — same method names as
    the reference class (include/loop_closing.hpp:29-80), driven through the C shim."""

    def __init__(self, loop_threshold: float = 0.7, min_loop_gap: int = 30, device: int = 0, shard_rank: int = 0,
                 shard_world: int = 1, group_devices: Optional[Sequence[int]] = None, loopback_shards: int = 0):
        """group_devices: the multi-device constructor (one process, an lcm_group over those devices);
        loopback_shards > 0: its rehearsal form, that many shards on `device`."""
        self._lib = load_library()
        for name, (res, args) in _HOST_SIGNATURES.items():
            fn = getattr(self._lib, name)
            fn.restype, fn.argtypes = res, args
        self._s = _vp()
        if loopback_shards > 0:
            _check(self._lib.lcs_create_group(loop_threshold, min_loop_gap, loopback_shards, None, device, C.byref(self._s)))
        elif group_devices is not None:
            ids = np.ascontiguousarray(group_devices, np.int32)
            _check(self._lib.lcs_create_group(loop_threshold, min_loop_gap, len(ids), ids.ctypes.data_as(_i32p), -1, C.byref(self._s)))
        else:
            _check(self._lib.lcs_create(loop_threshold, min_loop_gap, device, shard_rank, shard_world, C.byref(self._s)))

    def close(self):
        if getattr(self, "_s", None):
            self._lib.lcs_destroy(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _hcheck(self, rc):
        if rc != 0:
            raise LcmError(rc, self._lib.lcm_last_error().decode("utf-8", "replace"))

    def processFrame(self, descriptors, frame_id: int, num_keypoints: int = -1):
        d = _rows(descriptors)
        self._hcheck(self._lib.lcs_process_frame(self._s, _ptr(d), d.shape[0], num_keypoints, frame_id))

    def processFrames(self, descriptor_list, frame_ids, num_keypoints=None):
        """Several frames in order, scored in micro-batches (same result as processFrame for each)."""
        ds = [_rows(d) for d in descriptor_list]
        n = len(ds)
        ptrs = (_vp * max(n, 1))(*[d.ctypes.data if d.shape[0] else None for d in ds])
        rows = np.array([d.shape[0] for d in ds], np.int32)
        ids = np.ascontiguousarray(frame_ids, np.int32)
        kps = None if num_keypoints is None else np.ascontiguousarray(num_keypoints, np.int32)
        self._hcheck(self._lib.lcs_process_frames(self._s, ptrs, _ptr(rows), _ptr(kps), _ptr(ids), n))

    def matchFeatures(self, frame1_id: int, frame2_id: int, cap: int = 65536) -> np.ndarray:
        out = np.zeros(cap, DMATCH_DTYPE)
        n = C.c_int32(0)
        self._hcheck(self._lib.lcs_match_features(self._s, frame1_id, frame2_id, out.ctypes.data_as(_vp), cap, C.byref(n)))
        return out[: n.value]

    def detectLoops(self, current_frame_id: int) -> np.ndarray:
        cap = max(self._lib.lcs_num_frames(self._s), 1)
        out = np.zeros(cap, CANDIDATE_DTYPE)
        n = C.c_int32(0)
        self._hcheck(self._lib.lcs_detect_loops(self._s, current_frame_id, out.ctypes.data_as(_vp), cap, C.byref(n)))
        return out[: n.value]

    def getLoopClosures(self) -> np.ndarray:
        cap = max(self._lib.lcs_num_loop_closures(self._s), 1)
        out = np.zeros(cap, CANDIDATE_DTYPE)
        n = C.c_int32(0)
        self._hcheck(self._lib.lcs_get_loop_closures(self._s, out.ctypes.data_as(_vp), cap, C.byref(n)))
        return out[: n.value]

    def getConsecutiveMatches(self, cap: int = 65536) -> np.ndarray:
        out = np.zeros(cap, DMATCH_DTYPE)
        n = C.c_int32(0)
        self._hcheck(self._lib.lcs_get_consecutive_matches(self._s, out.ctypes.data_as(_vp), cap, C.byref(n)))
        return out[: n.value]

    def matchLoopClosures(self, current_frame_id: int, cap: int = 1 << 20):
        out = np.zeros(cap, DMATCH_DTYPE)
        offs = np.zeros(4096, np.uintp)
        n = C.c_int32(0)
        self._hcheck(self._lib.lcs_match_loop_closures(self._s, current_frame_id, out.ctypes.data_as(_vp), cap,
                                                       offs.ctypes.data_as(_vp), len(offs), C.byref(n)))
        return [out[int(offs[i]): int(offs[i + 1])] for i in range(n.value)]

    def setGapByPosition(self, on: bool = True):
        """Count min_loop_gap on arrival positions (the tree's own loop, src/main.cpp:1375-1379) instead of frame ids."""
        self._hcheck(self._lib.lcs_set_gap_by_position(self._s, 1 if on else 0))

    def numFrames(self) -> int:
        return self._lib.lcs_num_frames(self._s)

    def saveResults(self, output_dir: str):
        self._hcheck(self._lib.lcs_save_results(self._s, output_dir.encode()))
