"""ctypes binding of include/icpk.h (lib/libicpk.so).  No torch types cross the
boundary: device buffers are passed as integer addresses.

There is no CPU fallback: if the library is missing `load()` raises, and
`Context()` raises when no HIP device is usable (ICPK_E_NO_DEVICE).
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ICPK_LIB_PATH") or os.path.join(HERE, "lib", "libicpk.so")  # (ICPK_LIB_PATH: a diagnostic variant build)

OK = 0
W_TOO_FEW_PAIRS = 1
E_ARG, E_EMPTY_TARGET, E_HIP, E_NOT_SET, E_NO_DEVICE, E_RCCL = -1, -2, -3, -4, -5, -6
COMM_ID_BYTES = 128
SOLVE_REFERENCE, SOLVE_KABSCH, SOLVE_POINT_TO_PLANE, SOLVE_PLANE_TO_PLANE = 0, 1, 2, 3
W_DEGENERATE = 2
W_EMPTY_MAP = 3
W_NOT_CONVERGED = 4  # icpk_pose_graph_optimize ran into max_iterations
PG_PRUNE = 1  # icpk_pg_params.flags: drop the uncertain edges the line process switched off, optimise once more
PG_MAX_NODES, PG_MAX_EDGES = 1 << 20, 1 << 22
TSDF_COLOR = 1  # icpk_tsdf_params.flags: one intensity per voxel
TSDF_MAX_VOXELS, TSDF_MAX_SURFACE = 1 << 30, 1 << 28
TSDF_MAX_RAY_SAMPLES, TSDF_MAX_RAYCAST_PIXELS = 4096, 1 << 21
DEPTH_SCALE = 5000.0  # pointcloud.cpp:37
MAX_NN_KEYPOINT_DISTANCE = 0.1  # icp.hpp:10
NORMALS_CROSS, NORMALS_REFERENCE = 0, 1
SUBSAMPLE_FACTOR = 40  # pointcloud.hpp:11
NP2L = 28
NN_EXACT, NN_FILTERED, NN_PRUNED, NN_GRID, NN_MAP = 0, 1, 2, 3, 4
NSUM = 19
NSUM_W, NP2L_W = 21, 30  # icpk_reduce_weighted: the weighted sums, then W and the kept count
ROBUST_NONE, ROBUST_HUBER, ROBUST_TUKEY = 0, 1, 2
SCALE_FIXED, SCALE_MEDIAN = 0, 1
VOXEL_FIRST, VOXEL_CENTROID = 0, 1  # icpk_voxel_downsample: the representative / the fixed-point centroid
NORMALS_KEEP_MOMENTS = 1  # icpk_estimate_target_normals: keep the 10 int64 per point for icpk_get_normal_stats
FILTER_STATISTICAL, FILTER_RADIUS = 0, 1  # icpk_remove_outliers: mean k-NN distance / neighbour count within a radius
FILTER_MAX_K = 64
FILTER_STATS_ONLY = 1  # icpk_remove_outliers: compute and keep the statistics, leave the cloud as it is
SCORE_MAX_POSES = 4096  # icpk_score_poses: poses per call
NSCORE = 11  # ... sums per pose: sum d, sum d^2, sum q (3), sum q q^T (upper triangle, 6)
SCORE_KEEP_ASSOC = 1  # ... keep every pose's (index, distance) for icpk_get_score_associations
FPFH_BINS = 33  # icpk_compute_fpfh: floats per descriptor (three sub-histograms of 11 bins)
COLOR_KEEP_SUMS = 1  # icpk_estimate_target_color_gradients: keep the ten sums per point
FPFH_KEEP_SPFH = 1  # ... keep the SPFH counts and m for icpk_get_spfh
MATCH_MUTUAL = 1  # icpk_match_features: keep a pair only if each is the other's best
GLOBAL_MAX_HYPOTHESES = 1 << 20  # icpk_register_global
BRIEF_WORDS = 8  # K32: uint32 words per descriptor
BRIEF_MAX_KEYPOINTS = 65536
BRIEF_UPRIGHT = 1  # the describe calls: bin 0 everywhere
BRIEF_MUTUAL, BRIEF_TO_CLOUDS = 1, 2  # BriefMatchParams.flags
CLUSTER_LABELS_ONLY = 1  # icpk_cluster_dbscan (K33): compute and keep the record, leave the cloud as it is
PLANE_LABELS_ONLY, PLANE_KEEP_INLIERS = 1, 2  # icpk_segment_planes (K34): leave the cloud as it is / select the plane points
PLANE_MAX_HYPOTHESES, PLANE_MAX_PLANES = 65536, 16

# every symbol include/icpk.h declares (tests/test_abi.py checks the header against this list)
SYMBOLS = [
    "icpk_version", "icpk_create", "icpk_destroy", "icpk_last_error", "icpk_default_params",
    "icpk_set_log_callback", "icpk_stream", "icpk_set_target", "icpk_set_source", "icpk_set_target_device",
    "icpk_set_source_device", "icpk_reset_source", "icpk_commit_source", "icpk_get_source", "icpk_get_target", "icpk_source_size", "icpk_target_size",
    "icpk_nn", "icpk_reduce", "icpk_transform_source", "icpk_transform_target", "icpk_get_trace",
    "icpk_get_associations", "icpk_align",
    "icpk_align_batch", "icpk_align_batch_device", "icpk_backproject", "icpk_backproject_with_normals", "icpk_set_target_normals",
    "icpk_get_target_normals", "icpk_reduce_p2l", "icpk_solve_point_to_plane", "icpk_pair_distance", "icpk_pair_distance3", "icpk_distance3", "icpk_make_rotation_matrix",
    "icpk_matrix_to_quaternion", "icpk_quaternion_to_euler", "icpk_solve_reference", "icpk_solve_kabsch",
    "icpk_associate_keypoints", "icpk_filter_depth_image", "icpk_backproject_filtered", "icpk_backproject_pair", "icpk_set_subsample", "icpk_backproject_keypoints", "icpk_register_host_buffer", "icpk_unregister_host_buffer",
    "icpk_comm_unique_id", "icpk_comm_init_rccl", "icpk_comm_destroy", "icpk_comm_rank", "icpk_comm_world",
    "icpk_comm_partition", "icpk_comm_broadcast_target", "icpk_comm_gather_results", "icpk_comm_allreduce_sums",
    "icpk_comm_barrier", "icpk_align_query_sharded",
    "icpk_map_reset", "icpk_map_release", "icpk_map_update", "icpk_map_update_points", "icpk_map_set_points",
    "icpk_map_size", "icpk_map_get_list", "icpk_map_get_certainty", "icpk_map_query", "icpk_map_list_to_target",
    "icpk_map_voxel", "icpk_align_to_map", "icpk_map_nearest", "icpk_map_lookup_to_target", "icpk_align_to_map_dense",
    "icpk_bgr_to_gray", "icpk_detect_fast", "icpk_detected_to_cloud",
    "icpk_align_frames_batch", "icpk_get_frames_trace", "icpk_release_frame_streams",
    "icpk_set_robust", "icpk_get_robust_trace", "icpk_reduce_weighted",
    "icpk_voxel_downsample", "icpk_get_voxel_groups",
    "icpk_estimate_target_normals", "icpk_get_normal_stats",
    "icpk_remove_outliers", "icpk_get_outlier_stats",
    "icpk_estimate_source_normals", "icpk_set_source_normals", "icpk_get_source_normals", "icpk_set_plane_to_plane",
    "icpk_reduce_plane_to_plane",
    "icpk_intensity_from_bgr", "icpk_set_target_colors", "icpk_set_source_colors", "icpk_get_target_colors",
    "icpk_get_source_colors", "icpk_estimate_target_color_gradients", "icpk_get_target_color_gradients",
    "icpk_get_color_gradient_sums", "icpk_set_colored", "icpk_reduce_colored",
    "icpk_score_poses", "icpk_get_score_associations", "icpk_score_metrics", "icpk_information_matrix",
    "icpk_default_global_params", "icpk_compute_fpfh", "icpk_get_fpfh", "icpk_get_spfh", "icpk_match_features",
    "icpk_get_feature_matches", "icpk_register_global", "icpk_global_hypotheses",
    "icpk_default_pg_params", "icpk_pose_graph_check", "icpk_pose_graph_optimize", "icpk_pose_graph_evaluate",
    "icpk_get_pose_graph_trace",
    "icpk_default_tsdf_params", "icpk_tsdf_create", "icpk_tsdf_reset", "icpk_tsdf_release", "icpk_tsdf_integrate",
    "icpk_tsdf_get", "icpk_tsdf_extract_surface", "icpk_tsdf_get_surface", "icpk_tsdf_surface_to_target",
    "icpk_tsdf_invert_pose", "icpk_tsdf_voxel_update",
    "icpk_default_tsdf_raycast_params", "icpk_tsdf_raycast", "icpk_tsdf_get_raycast", "icpk_tsdf_raycast_to_target",
    "icpk_tsdf_raycast_pixels",
    "icpk_tsdf_extract_mesh", "icpk_tsdf_get_mesh", "icpk_tsdf_set", "icpk_tsdf_mesh_host",
    "icpk_tsdf_shift", "icpk_tsdf_extract_leaving", "icpk_tsdf_get_params", "icpk_tsdf_get_box",
    "icpk_tsdf_apply", "icpk_tsdf_deintegrate", "icpk_tsdf_voxel_apply",
    "icpk_default_bilateral_params", "icpk_bilateral_depth_image", "icpk_backproject_smoothed", "icpk_bilateral_tables",
    "icpk_bilateral_host",
    "icpk_default_pyramid_params", "icpk_depth_pyramid_build", "icpk_depth_pyramid_shape", "icpk_depth_pyramid_get",
    "icpk_depth_pyramid_backproject", "icpk_depth_pyramid_host",
    "icpk_default_projective_params", "icpk_projective_associate", "icpk_projective_reduce", "icpk_align_projective",
    "icpk_get_projective_trace", "icpk_projective_pixels",
    "icpk_default_projective_color_params", "icpk_depth_pyramid_set_intensity", "icpk_depth_pyramid_get_intensity",
    "icpk_intensity_pyramid_host", "icpk_tsdf_raycast_color_gradients", "icpk_tsdf_get_raycast_color_gradients",
    "icpk_tsdf_get_raycast_color_gradient_sums", "icpk_raycast_color_gradients_host", "icpk_projective_reduce_colored",
    "icpk_align_projective_colored", "icpk_projective_pixels_colored",
    "icpk_default_fern_params", "icpk_fern_create", "icpk_fern_reset", "icpk_fern_destroy", "icpk_fern_count",
    "icpk_fern_encode", "icpk_fern_query", "icpk_fern_add", "icpk_fern_process", "icpk_fern_add_code",
    "icpk_fern_get_keyframe", "icpk_fern_table", "icpk_fern_encode_host", "icpk_fern_dissimilarity_host",
    "icpk_frame_view_build", "icpk_frame_view_levels", "icpk_frame_view_shape", "icpk_frame_view_get",
    "icpk_frame_view_release", "icpk_frame_view_color_gradients", "icpk_frame_view_get_color_gradients",
    "icpk_projective_set_view", "icpk_frame_view_pixels",
    "icpk_default_sdf_params", "icpk_sdf_associate", "icpk_sdf_reduce", "icpk_align_sdf", "icpk_get_sdf_trace",
    "icpk_sdf_pixels",
    "icpk_default_esdf_params", "icpk_esdf_compute", "icpk_esdf_get", "icpk_esdf_get_box", "icpk_esdf_query",
    "icpk_esdf_release", "icpk_esdf_host", "icpk_esdf_query_host",
    "icpk_default_brief_match_params", "icpk_describe_keypoints", "icpk_describe_points", "icpk_get_descriptors",
    "icpk_set_descriptors", "icpk_described_to_cloud", "icpk_get_descriptor_cloud_map", "icpk_match_descriptors",
    "icpk_get_descriptor_matches", "icpk_brief_pattern", "icpk_brief_boundaries", "icpk_brief_bin",
    "icpk_brief_describe_host", "icpk_brief_match_host",
    "icpk_cluster_dbscan", "icpk_get_clusters", "icpk_cluster_host",
    "icpk_default_plane_params", "icpk_segment_planes", "icpk_get_planes", "icpk_segment_planes_host", "icpk_plane_fit_host",
]
MAX_FRAME_STREAMS = 256

# voxel certainty map (map.hpp:9-13)
MAP_HEIGHT = 300
MAP_CELLS = MAP_HEIGHT ** 3
MAP_MAX_CONFIDENCE = 180
MAP_DELTA_CONFIDENCE = 25
MAP_KEYPOINTS, MAP_POINTS = 0, 1
MAP_FROM_SOURCE, MAP_FROM_TARGET = 0, 1
MAP_ADD_CLOUD, MAP_ADD_ASSOCIATED, MAP_ADD_UNASSOCIATED = 0, 1, 2
MAP_NN_EMPTY, MAP_NN_NONE = -1, -2  # icpk_map_nearest: an empty voxel's zero point won / nothing beat 0.75

# FAST key points (SLAM.cpp:256: threshold 60, suppression on, TYPE_7_12)
FAST_TYPE_5_8, FAST_TYPE_7_12, FAST_TYPE_9_16 = 0, 1, 2


class Params(C.Structure):
    _fields_ = [
        ("max_iterations", C.c_int32),
        ("threshold", C.c_float),
        ("max_nn_dist", C.c_float),
        ("min_pairs", C.c_int32),
        ("solve", C.c_int32),
        ("fixed_iterations", C.c_int32),
        ("nn_mode", C.c_int32),
        ("profile", C.c_int32),
        ("last_rotation", C.c_float * 9),
        ("last_translation", C.c_float * 3),
        ("host_loop", C.c_int32),
        ("profile_stride", C.c_int32),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("iterations", C.c_int32),
        ("status", C.c_int32),
        ("final_pairs", C.c_int32),
        ("final_mse", C.c_float),
        ("nn_launches", C.c_int32),
        ("nn_timed_launches", C.c_int32),
        ("nn_ms_total", C.c_float),
        ("reduce_ms_total", C.c_float),
        ("transform_ms_total", C.c_float),
        ("total_ms", C.c_float),
    ]


class Pair(C.Structure):
    _fields_ = [
        ("sx", C.POINTER(C.c_float)), ("sy", C.POINTER(C.c_float)), ("sz", C.POINTER(C.c_float)),
        ("ns", C.c_int32),
        ("tx", C.POINTER(C.c_float)), ("ty", C.POINTER(C.c_float)), ("tz", C.POINTER(C.c_float)),
        ("nt", C.c_int32),
        ("idx_out", C.POINTER(C.c_int32)), ("dist_out", C.POINTER(C.c_float)),
    ]


class GlobalParams(C.Structure):
    """icpk_global_params"""
    _fields_ = [("seed", C.c_uint64), ("n_hypotheses", C.c_int32), ("max_dist", C.c_float),
                ("edge_similarity", C.c_float), ("reserved", C.c_int32)]


class GlobalResult(C.Structure):
    """icpk_global_result"""
    _fields_ = [("T", C.c_float * 16), ("hypothesis", C.c_int32), ("n_valid", C.c_int32), ("n_matches", C.c_int32),
                ("reserved", C.c_int32), ("inliers", C.c_int64), ("sums", C.c_double * 11)]


class PgEdge(C.Structure):
    """icpk_pg_edge: T moves cloud `source` onto cloud `target`; info is the 6 x 6 information matrix, rotation first."""
    _fields_ = [("source", C.c_int32), ("target", C.c_int32), ("uncertain", C.c_int32), ("reserved", C.c_int32),
                ("T", C.c_double * 16), ("info", C.c_double * 36)]


class PgParams(C.Structure):
    """icpk_pg_params"""
    _fields_ = [("max_iterations", C.c_int32), ("max_pcg_iterations", C.c_int32), ("pcg_tolerance", C.c_double),
                ("tau", C.c_double), ("cost_tolerance", C.c_double), ("step_tolerance", C.c_double),
                ("gradient_tolerance", C.c_double), ("preference_loop_closure", C.c_double),
                ("edge_prune_threshold", C.c_double), ("reference_node", C.c_int32), ("flags", C.c_int32)]


class PgResult(C.Structure):
    """icpk_pg_result"""
    _fields_ = [("iterations", C.c_int32), ("accepted", C.c_int32), ("pcg_iterations", C.c_int32),
                ("n_pruned", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("final_lambda", C.c_double)]


class TsdfParams(C.Structure):
    """icpk_tsdf_params"""
    _fields_ = [("dims", C.c_int32 * 3), ("voxel", C.c_float), ("origin", C.c_float * 3), ("trunc", C.c_float),
                ("max_weight", C.c_int32), ("depth_scale", C.c_float), ("flags", C.c_int32)]


class TsdfOp(C.Structure):
    _fields_ = [("sign", C.c_int32), ("frame", C.c_int32), ("pose", C.c_double * 16)]


ESDF_UNKNOWN_OCCUPIED = 1  # icpk_esdf_params.flags: a voxel of unknown class counts as an obstacle
ESDF_MAX_RADIUS = 1024     # the largest max_distance / voxel
ESDF_FAR = 2 ** 31 - 1     # |q| of a voxel with nothing of the other kind within the radius
ESDF_UNKNOWN, ESDF_FREE, ESDF_OCCUPIED = 0, 1, 2  # the class plane
ESDF_Q_FAR, ESDF_Q_UNKNOWN, ESDF_Q_OUTSIDE = 1, 2, 0x80  # the query's status bits
ESDF_MAX_QUERY = 1 << 24   # points per icpk_esdf_query


class EsdfParams(C.Structure):
    """icpk_esdf_params"""
    _fields_ = [("min_weight", C.c_int32), ("max_distance", C.c_float), ("flags", C.c_int32)]


class TsdfRaycastParams(C.Structure):
    """icpk_tsdf_raycast_params"""
    _fields_ = [("rows", C.c_int32), ("cols", C.c_int32), ("fx", C.c_float), ("cx", C.c_float), ("z_near", C.c_float),
                ("z_far", C.c_float), ("step", C.c_float), ("min_weight", C.c_int32)]


BILATERAL_MAX_RADIUS = 6  # icpk_bilateral_params.radius
BILATERAL_MAX_RANGE = 4096  # ... and the largest K: entries of the range table


class BilateralParams(C.Structure):
    """icpk_bilateral_params"""
    _fields_ = [("radius", C.c_int32), ("sigma_space", C.c_float), ("sigma_range", C.c_float), ("range_cutoff", C.c_int32)]


PYRAMID_MAX_LEVELS = 8  # icpk_pyramid_params.levels


class PyramidParams(C.Structure):
    """icpk_pyramid_params"""
    _fields_ = [("levels", C.c_int32), ("range_cutoff", C.c_int32)]


PROJECTIVE_MAX_ITERATIONS = 64  # icpk_projective_params.max_iterations
VIEW_RAYCAST, VIEW_FRAME = 0, 1  # icpk_projective_set_view: which planes the projective calls read (K28)
# icpk_projective_associate: why a pixel has no pair
PROJ_NO_DEPTH, PROJ_BEHIND, PROJ_OUTSIDE, PROJ_NO_MODEL, PROJ_TOO_FAR, PROJ_NO_NORMAL, PROJ_NORMAL = -1, -2, -3, -4, -5, -6, -7


class ProjectiveParams(C.Structure):
    """icpk_projective_params"""
    _fields_ = [("level", C.c_int32), ("fx", C.c_float), ("cx", C.c_float), ("max_iterations", C.c_int32),
                ("max_dist", C.c_float), ("min_normal_cos", C.c_float), ("min_pairs", C.c_int32)]


class ProjectiveResult(C.Structure):
    """icpk_projective_result: count and mean_dist are those of the last evaluated iteration"""
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("count", C.c_int64), ("mean_dist", C.c_double)]


class ProjectiveIter(C.Structure):
    """icpk_projective_iter"""
    _fields_ = [("pose", C.c_double * 12), ("sums", C.c_double * 28), ("count", C.c_int64), ("status", C.c_int32),
                ("reserved", C.c_int32)]


# icpk_sdf_associate: why a pixel is rejected (K29)
SDF_NO_DEPTH, SDF_OUTSIDE, SDF_UNKNOWN, SDF_TOO_FAR, SDF_NO_GRADIENT, SDF_NO_NORMAL, SDF_NORMAL = -1, -2, -3, -4, -5, -6, -7


class SdfParams(C.Structure):
    """icpk_sdf_params"""
    _fields_ = [("level", C.c_int32), ("fx", C.c_float), ("cx", C.c_float), ("max_iterations", C.c_int32),
                ("max_abs_tsdf", C.c_float), ("min_weight", C.c_int32), ("min_normal_cos", C.c_float),
                ("min_pairs", C.c_int32)]


class ProjectiveColorParams(C.Structure):
    """icpk_projective_color_params"""
    _fields_ = [("lambda_geometric", C.c_float)]


FERN_MAX_K = 8  # icpk_fern_query / icpk_fern_process: the most keyframes a search returns
FERN_MAX_FERNS, FERN_MAX_KEYFRAMES = 1024, 65536


class FernParams(C.Structure):
    """icpk_fern_params"""
    _fields_ = [("level", C.c_int32), ("n_ferns", C.c_int32), ("seed", C.c_uint64), ("d_min", C.c_int32), ("d_max", C.c_int32),
                ("capacity", C.c_int32), ("harvest_above", C.c_int32), ("min_valid", C.c_int32), ("reserved", C.c_int32)]


class FrameJob(C.Structure):
    """icpk_frame_job: one stream's next frame pair for icpk_align_frames_batch."""
    _fields_ = [
        ("stream", C.c_int32),
        ("depth_source", C.POINTER(C.c_uint16)),
        ("depth_target", C.POINTER(C.c_uint16)),
        ("R", C.c_float * 9), ("t", C.c_float * 3),
        ("last_rotation", C.c_float * 9), ("last_translation", C.c_float * 3),
    ]


LOG_FN = C.CFUNCTYPE(None, C.c_int, C.c_int, C.c_double, C.c_void_p)

_lib = None


class Robust(C.Structure):
    """icpk_robust: kernel ROBUST_*, scale_mode SCALE_*, scale (> 0), trim_fraction (0, 1]."""
    _fields_ = [
        ("kernel", C.c_int32),
        ("scale_mode", C.c_int32),
        ("scale", C.c_float),
        ("trim_fraction", C.c_float),
    ]


class OutlierFilter(C.Structure):
    """icpk_outlier_filter: kind FILTER_*, k and std_ratio (statistical), radius and min_neighbors (radius)."""
    _fields_ = [
        ("kind", C.c_int32),
        ("k", C.c_int32),
        ("std_ratio", C.c_float),
        ("radius", C.c_float),
        ("min_neighbors", C.c_int32),
    ]


class IcpkError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"icpk status {code}: {msg}")
        self.code = code


class PlaneParams(C.Structure):
    """icpk_plane_params (K34): seed, t, hypotheses per round, rounds and min_inliers of THE PLANE RULE, select_plane of its
    selection"""
    _fields_ = [("seed", C.c_uint64), ("distance_threshold", C.c_float), ("n_hypotheses", C.c_int32), ("max_planes", C.c_int32),
                ("min_inliers", C.c_int32), ("select_plane", C.c_int32), ("reserved", C.c_int32)]


class ClusterParams(C.Structure):
    """icpk_cluster_params (K33): eps and min_points of THE CLUSTER RULE, min_size / max_size / largest_only of its selection"""
    _fields_ = [("eps", C.c_float), ("min_points", C.c_int32), ("min_size", C.c_int32), ("max_size", C.c_int32),
                ("largest_only", C.c_int32)]


class BriefMatchParams(C.Structure):
    """icpk_brief_match_params (K32)"""
    _fields_ = [("max_hamming", C.c_int32), ("ratio_num", C.c_int32), ("ratio_den", C.c_int32), ("flags", C.c_int32)]


def load():
    """Load libicpk.so.  Raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    lib = C.CDLL(LIB_PATH)
    lib.icpk_version.restype = C.c_char_p
    lib.icpk_last_error.restype = C.c_char_p
    lib.icpk_last_error.argtypes = [C.c_void_p]
    lib.icpk_stream.restype = C.c_void_p
    lib.icpk_stream.argtypes = [C.c_void_p]
    lib.icpk_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    lib.icpk_destroy.argtypes = [C.c_void_p]
    lib.icpk_destroy.restype = None
    fp = C.POINTER(C.c_float)
    for name in ("icpk_set_target", "icpk_set_source"):
        getattr(lib, name).argtypes = [C.c_void_p, fp, fp, fp, C.c_int32]
    for name in ("icpk_set_target_device", "icpk_set_source_device"):
        getattr(lib, name).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    lib.icpk_reset_source.argtypes = [C.c_void_p]
    lib.icpk_commit_source.argtypes = [C.c_void_p]
    lib.icpk_get_source.argtypes = [C.c_void_p, fp, fp, fp]
    lib.icpk_get_target.argtypes = [C.c_void_p, fp, fp, fp]
    lib.icpk_source_size.argtypes = [C.c_void_p]
    lib.icpk_target_size.argtypes = [C.c_void_p]
    lib.icpk_nn.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), fp]
    lib.icpk_reduce.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.icpk_transform_source.argtypes = [C.c_void_p, fp, fp]
    lib.icpk_transform_target.argtypes = [C.c_void_p, fp, fp]
    lib.icpk_get_trace.argtypes = [C.c_void_p, C.POINTER(C.c_int32), fp, fp, C.POINTER(C.c_int32), fp]
    lib.icpk_get_associations.argtypes = [C.c_void_p, C.POINTER(C.c_int32), fp]
    lib.icpk_align.argtypes = [C.c_void_p, C.POINTER(Params), fp, C.POINTER(Stats)]
    lib.icpk_align_batch.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Pair), C.POINTER(Params), fp, C.POINTER(Stats)]
    lib.icpk_align_batch_device.argtypes = lib.icpk_align_batch.argtypes
    lib.icpk_set_subsample.argtypes = [C.c_void_p, C.c_int32, C.c_uint64]
    lib.icpk_register_host_buffer.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.icpk_unregister_host_buffer.argtypes = [C.c_void_p, C.c_void_p]
    lib.icpk_backproject.argtypes = [C.c_void_p, C.POINTER(C.c_uint16), C.c_int32, C.c_int32, C.c_float, C.c_float,
                                     fp, C.c_int32]
    lib.icpk_pair_distance.argtypes = [C.c_void_p, fp, fp, fp, C.c_int32]
    lib.icpk_pair_distance3.argtypes = [C.c_void_p, fp, fp, fp, C.c_int32]
    lib.icpk_distance3.argtypes = [fp, fp]
    lib.icpk_distance3.restype = C.c_float
    lib.icpk_backproject_with_normals.argtypes = [C.c_void_p, C.POINTER(C.c_uint16), C.c_int32, C.c_int32, C.c_float,
                                                  C.c_float, fp, C.c_int32]
    lib.icpk_set_target_normals.argtypes = [C.c_void_p, fp, fp, fp, C.c_int32]
    lib.icpk_get_target_normals.argtypes = [C.c_void_p, fp, fp, fp]
    lib.icpk_reduce_p2l.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.icpk_solve_point_to_plane.argtypes = [C.POINTER(C.c_double)] * 3
    lib.icpk_default_params.argtypes = [C.POINTER(Params)]
    lib.icpk_default_params.restype = None
    lib.icpk_set_log_callback.argtypes = [C.c_void_p, LOG_FN, C.c_void_p]
    lib.icpk_make_rotation_matrix.argtypes = [C.c_float, C.c_float, C.c_float, fp]
    lib.icpk_backproject_keypoints.argtypes = [C.POINTER(C.c_uint16), C.c_int32, C.c_int32, fp, C.c_int32, C.c_float, C.c_float, fp,
                                               C.POINTER(C.c_int32)]
    lib.icpk_make_rotation_matrix.restype = None
    lib.icpk_matrix_to_quaternion.argtypes = [fp, fp]
    lib.icpk_matrix_to_quaternion.restype = None
    lib.icpk_quaternion_to_euler.argtypes = [fp, fp]
    lib.icpk_quaternion_to_euler.restype = None
    lib.icpk_solve_reference.argtypes = [fp, fp]
    lib.icpk_solve_reference.restype = None
    dp = C.POINTER(C.c_double)
    lib.icpk_solve_kabsch.argtypes = [C.c_int64, dp, dp, dp, dp, dp]
    lib.icpk_solve_kabsch.restype = None
    ip = C.POINTER(C.c_int32)
    lib.icpk_associate_keypoints.argtypes = [C.c_void_p, C.c_int32, C.c_float, ip, ip, fp, ip, ip, C.c_int32, ip]
    u16 = C.POINTER(C.c_uint16)
    lib.icpk_filter_depth_image.argtypes = [C.c_void_p, u16, u16, C.c_int32, C.c_int32] + [C.c_int32] * 5
    lib.icpk_backproject_filtered.argtypes = [C.c_void_p, u16, C.c_int32, C.c_int32, C.c_float, C.c_float, fp,
                                              C.c_int32, C.c_int32] + [C.c_int32] * 5
    lib.icpk_backproject_pair.argtypes = [C.c_void_p, u16, u16, C.c_int32, C.c_int32, C.c_float, C.c_float, fp, fp, fp] + \
        [C.c_int32] * 6 + [C.POINTER(C.c_int32)] * 2
    lib.icpk_align_frames_batch.argtypes = [C.c_void_p, C.c_int32, C.POINTER(FrameJob), C.c_int32, C.c_int32, C.c_float,
                                            C.c_float, fp] + [C.c_int32] * 6 + [C.POINTER(Params), fp, C.POINTER(Stats)]
    lib.icpk_get_frames_trace.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), fp, fp, C.POINTER(C.c_int32), fp]
    lib.icpk_release_frame_streams.argtypes = [C.c_void_p]
    lib.icpk_comm_unique_id.argtypes = [C.c_void_p]
    lib.icpk_comm_init_rccl.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.icpk_comm_destroy.argtypes = [C.c_void_p]
    lib.icpk_comm_rank.argtypes = [C.c_void_p]
    lib.icpk_comm_world.argtypes = [C.c_void_p]
    lib.icpk_comm_partition.argtypes = [C.c_int32, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.icpk_comm_partition.restype = None
    lib.icpk_comm_broadcast_target.argtypes = [C.c_void_p, C.c_int]
    lib.icpk_comm_gather_results.argtypes = [C.c_void_p, fp, C.POINTER(Stats), C.c_int32, C.c_int32, fp, fp]
    lib.icpk_comm_allreduce_sums.argtypes = [C.c_void_p, dp, C.c_int32, C.POINTER(C.c_int64)]
    lib.icpk_comm_barrier.argtypes = [C.c_void_p]
    lib.icpk_align_query_sharded.argtypes = [C.c_void_p, C.POINTER(Params), fp, C.POINTER(Stats)]
    u8 = C.POINTER(C.c_uint8)
    lib.icpk_map_reset.argtypes = [C.c_void_p]
    lib.icpk_map_release.argtypes = [C.c_void_p]
    lib.icpk_map_update.argtypes = [C.c_void_p, C.c_int32, C.c_int32, ip, C.c_int32, C.c_int32]
    lib.icpk_map_update_points.argtypes = [C.c_void_p, C.c_int32, fp, fp, fp, C.c_int32, C.c_int32]
    lib.icpk_map_set_points.argtypes = [C.c_void_p, C.c_int32]
    lib.icpk_map_size.argtypes = [C.c_void_p, C.c_int32]
    lib.icpk_map_get_list.argtypes = [C.c_void_p, C.c_int32, fp, fp, fp]
    lib.icpk_map_get_certainty.argtypes = [C.c_void_p, u8]
    lib.icpk_map_query.argtypes = [C.c_void_p, fp, fp, fp, C.c_int32, u8, u8, ip, ip]
    lib.icpk_map_list_to_target.argtypes = [C.c_void_p, C.c_int32]
    lib.icpk_map_voxel.argtypes = [fp, ip]
    lib.icpk_map_voxel.restype = None
    lib.icpk_align_to_map.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int32, fp, C.POINTER(Stats)]
    lib.icpk_map_nearest.argtypes = [C.c_void_p, fp, fp, fp, C.c_int32, fp, ip, ip]
    lib.icpk_map_lookup_to_target.argtypes = [C.c_void_p]
    lib.icpk_align_to_map_dense.argtypes = lib.icpk_align_to_map.argtypes
    lib.icpk_bgr_to_gray.argtypes = [C.c_void_p, u8, C.c_int32, C.c_int32, u8]
    lib.icpk_detect_fast.argtypes = [C.c_void_p, u8] + [C.c_int32] * 7 + [fp, fp, ip]
    lib.icpk_detected_to_cloud.argtypes = [C.c_void_p, u16, C.c_int32, C.c_int32, C.c_float, C.c_float, fp, fp, C.c_int32, ip]
    lib.icpk_set_robust.argtypes = [C.c_void_p, C.POINTER(Robust)]
    lib.icpk_get_robust_trace.argtypes = [C.c_void_p, ip, ip, fp, dp, dp]
    lib.icpk_reduce_weighted.argtypes = [C.c_void_p, C.c_float, C.c_int32, dp, C.POINTER(C.c_int64),
                                         C.POINTER(C.c_int64), fp, fp, dp]
    lib.icpk_voxel_downsample.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_int32, ip, ip]
    lib.icpk_get_voxel_groups.argtypes = [C.c_void_p, ip, ip, ip, ip, ip]
    lib.icpk_estimate_target_normals.argtypes = [C.c_void_p, C.c_float, C.c_int32, fp, C.c_int32]
    lib.icpk_get_normal_stats.argtypes = [C.c_void_p, ip, ip, ip, fp, C.POINTER(C.c_int64)]
    lib.icpk_remove_outliers.argtypes = [C.c_void_p, C.c_int32, C.POINTER(OutlierFilter), C.c_int32, ip, ip]
    lib.icpk_get_outlier_stats.argtypes = [C.c_void_p, ip, ip, C.POINTER(C.c_double), fp, ip, C.POINTER(C.c_double)]
    lib.icpk_estimate_source_normals.argtypes = [C.c_void_p, C.c_float, C.c_int32, fp, C.c_int32]
    lib.icpk_set_source_normals.argtypes = [C.c_void_p, fp, fp, fp, C.c_int32]
    lib.icpk_get_source_normals.argtypes = [C.c_void_p, fp, fp, fp]
    lib.icpk_set_plane_to_plane.argtypes = [C.c_void_p, C.c_float]
    lib.icpk_reduce_plane_to_plane.argtypes = [C.c_void_p, C.c_float, fp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.icpk_intensity_from_bgr.argtypes = [C.POINTER(C.c_uint8), C.c_int32, fp]
    lib.icpk_intensity_from_bgr.restype = None
    lib.icpk_set_target_colors.argtypes = [C.c_void_p, fp, C.c_int32]
    lib.icpk_set_source_colors.argtypes = [C.c_void_p, fp, C.c_int32]
    lib.icpk_get_target_colors.argtypes = [C.c_void_p, fp]
    lib.icpk_get_source_colors.argtypes = [C.c_void_p, fp]
    lib.icpk_estimate_target_color_gradients.argtypes = [C.c_void_p, C.c_float, C.c_int32, C.c_int32]
    lib.icpk_get_target_color_gradients.argtypes = [C.c_void_p, fp, fp, fp]
    lib.icpk_get_color_gradient_sums.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    lib.icpk_set_colored.argtypes = [C.c_void_p, C.c_int32, C.c_float]
    lib.icpk_reduce_colored.argtypes = [C.c_void_p, C.c_float, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    lib.icpk_score_poses.argtypes = [C.c_void_p, C.c_int32, fp, C.c_float, C.c_int32, dp, C.POINTER(C.c_int64)]
    lib.icpk_get_score_associations.argtypes = [C.c_void_p, C.c_int32, ip, fp]
    lib.icpk_score_metrics.argtypes = [dp, C.c_int64, C.c_int32, fp, fp, fp]
    lib.icpk_score_metrics.restype = None
    lib.icpk_information_matrix.argtypes = [dp, C.c_int64, dp]
    lib.icpk_information_matrix.restype = None
    lib.icpk_default_global_params.argtypes = [C.POINTER(GlobalParams)]
    lib.icpk_default_global_params.restype = None
    lib.icpk_compute_fpfh.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_int32]
    lib.icpk_get_fpfh.argtypes = [C.c_void_p, C.c_int32, fp, u8, ip]
    lib.icpk_get_spfh.argtypes = [C.c_void_p, C.c_int32, ip, ip]
    lib.icpk_match_features.argtypes = [C.c_void_p, C.c_int32]
    lib.icpk_get_feature_matches.argtypes = [C.c_void_p, ip, ip, fp, ip]
    lib.icpk_register_global.argtypes = [C.c_void_p, C.POINTER(GlobalParams), C.POINTER(GlobalResult)]
    lib.icpk_global_hypotheses.argtypes = [ip, ip, C.c_int32, fp, fp, fp, C.c_int32, fp, fp, fp, C.c_int32, C.c_uint64,
                                           C.c_float, C.c_int64, C.c_int32, ip, u8, fp]
    lib.icpk_default_pg_params.argtypes = [C.POINTER(PgParams)]
    lib.icpk_default_pg_params.restype = None
    lib.icpk_pose_graph_check.argtypes = [C.c_int32, dp, C.c_int32, C.POINTER(PgEdge), C.POINTER(PgParams)]
    lib.icpk_pose_graph_optimize.argtypes = [C.c_void_p, C.c_int32, dp, C.c_int32, C.POINTER(PgEdge), C.POINTER(PgParams),
                                             C.POINTER(PgResult), dp, dp, u8]
    lib.icpk_pose_graph_evaluate.argtypes = [C.c_void_p, C.c_int32, dp, C.c_int32, C.POINTER(PgEdge), C.c_double, dp, dp,
                                             dp, dp]
    lib.icpk_get_pose_graph_trace.argtypes = [C.c_void_p, ip, dp, dp, ip, ip]
    u16 = C.POINTER(C.c_uint16)
    lib.icpk_default_tsdf_params.argtypes = [C.POINTER(TsdfParams)]
    lib.icpk_default_tsdf_params.restype = None
    lib.icpk_tsdf_create.argtypes = [C.c_void_p, C.POINTER(TsdfParams)]
    lib.icpk_tsdf_reset.argtypes = [C.c_void_p]
    lib.icpk_tsdf_release.argtypes = [C.c_void_p]
    lib.icpk_tsdf_integrate.argtypes = [C.c_void_p, u16, fp, C.c_int32, C.c_int32, C.c_float, C.c_float, dp, ip]
    lib.icpk_tsdf_get.argtypes = [C.c_void_p, fp, u16, fp]
    lib.icpk_tsdf_extract_surface.argtypes = [C.c_void_p, C.c_int32, ip, ip]
    lib.icpk_tsdf_get_surface.argtypes = [C.c_void_p, fp, fp, fp, fp, fp, fp, fp, ip, u8]
    lib.icpk_tsdf_surface_to_target.argtypes = [C.c_void_p]
    lib.icpk_tsdf_invert_pose.argtypes = [dp, fp, fp]
    lib.icpk_tsdf_voxel_update.argtypes = [C.POINTER(TsdfParams), fp, fp, u16, fp, C.c_int32, C.c_int32, C.c_float,
                                           C.c_float, C.c_int64, C.c_int32, fp, u16, fp]
    lib.icpk_default_tsdf_raycast_params.argtypes = [C.POINTER(TsdfRaycastParams)]
    lib.icpk_default_tsdf_raycast_params.restype = None
    lib.icpk_tsdf_raycast.argtypes = [C.c_void_p, C.POINTER(TsdfRaycastParams), dp, ip, ip]
    lib.icpk_tsdf_get_raycast.argtypes = [C.c_void_p, fp, fp, fp, fp, fp, fp, fp, fp]
    lib.icpk_tsdf_raycast_to_target.argtypes = [C.c_void_p]
    lib.icpk_tsdf_raycast_pixels.argtypes = [C.POINTER(TsdfParams), C.POINTER(TsdfRaycastParams), dp, fp, u16, fp,
                                             C.c_int64, C.c_int32, fp]
    lib.icpk_tsdf_extract_mesh.argtypes = [C.c_void_p, C.c_int32, ip, ip, ip]
    lib.icpk_tsdf_get_mesh.argtypes = [C.c_void_p, fp, fp, fp, fp, fp, fp, fp, ip, u8, ip]
    lib.icpk_tsdf_set.argtypes = [C.c_void_p, fp, u16, fp]
    lib.icpk_tsdf_mesh_host.argtypes = [C.POINTER(TsdfParams), C.c_int32, fp, u16, fp, C.c_int64, C.c_int64, fp, fp, fp,
                                        fp, fp, fp, fp, ip, u8, ip, C.POINTER(C.c_int64)]
    lib.icpk_tsdf_shift.argtypes = [C.c_void_p, ip]
    lib.icpk_tsdf_extract_leaving.argtypes = [C.c_void_p, C.c_int32, ip, ip, ip]
    lib.icpk_tsdf_get_params.argtypes = [C.c_void_p, C.POINTER(TsdfParams), C.POINTER(C.c_int64)]
    lib.icpk_tsdf_get_box.argtypes = [C.c_void_p, ip, ip, fp, u16, fp]
    lib.icpk_tsdf_apply.argtypes = [C.c_void_p, C.c_int32, C.POINTER(u16), C.POINTER(fp), C.c_int32, C.c_int32, C.c_float,
                                    C.c_float, C.c_int32, C.POINTER(TsdfOp), C.POINTER(C.c_int64)]
    lib.icpk_tsdf_deintegrate.argtypes = lib.icpk_tsdf_integrate.argtypes
    lib.icpk_tsdf_voxel_apply.argtypes = [C.POINTER(TsdfParams), C.c_int32, C.POINTER(u16), C.POINTER(fp), C.c_int32,
                                          C.c_int32, C.c_float, C.c_float, C.c_int32, C.POINTER(TsdfOp), C.c_int64,
                                          C.c_int32, fp, u16, fp, C.POINTER(C.c_int64)]
    bp = C.POINTER(BilateralParams)
    lib.icpk_default_bilateral_params.argtypes = [bp]
    lib.icpk_default_bilateral_params.restype = None
    lib.icpk_bilateral_depth_image.argtypes = [C.c_void_p, bp, u16, u16, C.c_int32, C.c_int32]
    lib.icpk_backproject_smoothed.argtypes = [C.c_void_p, u16, C.c_int32, C.c_int32, C.c_float, C.c_float, fp, C.c_int32,
                                              C.c_int32, bp]
    lib.icpk_bilateral_tables.argtypes = [bp, u16, u16, ip]
    lib.icpk_bilateral_host.argtypes = [bp, u16, C.c_int32, C.c_int32, u16]
    pp = C.POINTER(PyramidParams)
    lib.icpk_default_pyramid_params.argtypes = [pp]
    lib.icpk_default_pyramid_params.restype = None
    lib.icpk_depth_pyramid_build.argtypes = [C.c_void_p, u16, C.c_int32, C.c_int32, pp, bp]
    lib.icpk_depth_pyramid_shape.argtypes = [C.c_void_p, C.c_int32, ip, ip]
    lib.icpk_depth_pyramid_get.argtypes = [C.c_void_p, C.c_int32, u16]
    lib.icpk_depth_pyramid_backproject.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_float, fp, C.c_int32, C.c_int32]
    lib.icpk_depth_pyramid_host.argtypes = [pp, u16, C.c_int32, C.c_int32, C.c_int32, u16]
    jp = C.POINTER(ProjectiveParams)
    lib.icpk_default_projective_params.argtypes = [jp]
    lib.icpk_default_projective_params.restype = None
    lib.icpk_projective_associate.argtypes = [C.c_void_p, jp, dp, ip, fp]
    lib.icpk_projective_reduce.argtypes = [C.c_void_p, jp, dp, dp, C.POINTER(C.c_int64)]
    lib.icpk_align_projective.argtypes = [C.c_void_p, jp, dp, dp, C.POINTER(ProjectiveResult)]
    lib.icpk_get_projective_trace.argtypes = [C.c_void_p, C.POINTER(ProjectiveIter), C.c_int32]
    lib.icpk_projective_pixels.argtypes = [jp, dp, u16, C.c_int32, C.c_int32, C.POINTER(fp), C.c_int32, C.c_int32,
                                           C.c_float, C.c_float, dp, C.c_int64, C.c_int32, ip, fp, dp]
    kp = C.POINTER(ProjectiveColorParams)
    i64 = C.POINTER(C.c_int64)
    lib.icpk_default_projective_color_params.argtypes = [kp]
    lib.icpk_default_projective_color_params.restype = None
    lib.icpk_depth_pyramid_set_intensity.argtypes = [C.c_void_p, fp, C.c_int32, C.c_int32]
    lib.icpk_depth_pyramid_get_intensity.argtypes = [C.c_void_p, C.c_int32, fp]
    lib.icpk_intensity_pyramid_host.argtypes = [pp, u16, fp, C.c_int32, C.c_int32, C.c_int32, fp]
    lib.icpk_tsdf_raycast_color_gradients.argtypes = [C.c_void_p, C.c_float, C.c_int32, C.c_int32]
    lib.icpk_tsdf_get_raycast_color_gradients.argtypes = [C.c_void_p, fp, fp, fp]
    lib.icpk_tsdf_get_raycast_color_gradient_sums.argtypes = [C.c_void_p, i64]
    lib.icpk_raycast_color_gradients_host.argtypes = [C.POINTER(fp), C.c_int32, C.c_int32, C.c_float, C.c_int32, C.c_int64,
                                                      C.c_int32, i64, fp]
    lib.icpk_projective_reduce_colored.argtypes = [C.c_void_p, jp, kp, dp, dp, i64]
    lib.icpk_align_projective_colored.argtypes = [C.c_void_p, jp, kp, dp, dp, C.POINTER(ProjectiveResult)]
    lib.icpk_projective_pixels_colored.argtypes = [jp, dp, u16, C.c_int32, C.c_int32, C.POINTER(fp), C.c_int32, C.c_int32,
                                                   C.c_float, C.c_float, dp, C.c_int64, C.c_int32, ip, fp, dp, fp, fp,
                                                   C.POINTER(fp), kp]
    ep = C.POINTER(FernParams)
    u32 = C.POINTER(C.c_uint32)
    lib.icpk_default_fern_params.argtypes = [ep]
    lib.icpk_default_fern_params.restype = None
    lib.icpk_fern_create.argtypes = [C.c_void_p, ep, C.c_int32, C.c_int32]
    for name in ("icpk_fern_reset", "icpk_fern_destroy", "icpk_fern_count"):
        getattr(lib, name).argtypes = [C.c_void_p]
    lib.icpk_fern_encode.argtypes = [C.c_void_p, u32, ip]
    lib.icpk_fern_query.argtypes = [C.c_void_p, C.c_int32, ip, ip, ip]
    lib.icpk_fern_add.argtypes = [C.c_void_p, dp, ip]
    lib.icpk_fern_process.argtypes = [C.c_void_p, dp, C.c_int32, ip, ip, ip, ip, ip]
    lib.icpk_fern_add_code.argtypes = [C.c_void_p, u32, dp, ip]
    lib.icpk_fern_get_keyframe.argtypes = [C.c_void_p, C.c_int32, u32, dp]
    lib.icpk_fern_table.argtypes = [ep, C.c_int32, C.c_int32, ip]
    lib.icpk_fern_encode_host.argtypes = [ep, u16, C.c_int32, C.c_int32, u32, ip]
    lib.icpk_fern_dissimilarity_host.argtypes = [u32, u32, C.c_int32]
    lib.icpk_frame_view_build.argtypes = [C.c_void_p, C.c_float, C.c_float, dp, ip, ip]
    lib.icpk_frame_view_levels.argtypes = [C.c_void_p]
    lib.icpk_frame_view_shape.argtypes = [C.c_void_p, C.c_int32, ip, ip]
    lib.icpk_frame_view_get.argtypes = [C.c_void_p, C.c_int32, C.POINTER(fp)]
    lib.icpk_frame_view_release.argtypes = [C.c_void_p]
    lib.icpk_frame_view_color_gradients.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_int32, C.c_int32]
    lib.icpk_frame_view_get_color_gradients.argtypes = [C.c_void_p, C.c_int32, fp, fp, fp]
    lib.icpk_projective_set_view.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.icpk_frame_view_pixels.argtypes = [C.c_float, C.c_float, C.c_int32, dp, u16, fp, C.c_int32, C.c_int32, C.c_int64,
                                           C.c_int32, fp, ip]
    sp = C.POINTER(SdfParams)
    lib.icpk_default_sdf_params.argtypes = [sp]
    lib.icpk_default_sdf_params.restype = None
    lib.icpk_sdf_associate.argtypes = [C.c_void_p, sp, dp, ip, fp]
    lib.icpk_sdf_reduce.argtypes = [C.c_void_p, sp, dp, dp, i64]
    lib.icpk_align_sdf.argtypes = [C.c_void_p, sp, dp, dp, C.POINTER(ProjectiveResult)]
    lib.icpk_get_sdf_trace.argtypes = [C.c_void_p, C.POINTER(ProjectiveIter), C.c_int32]
    lib.icpk_sdf_pixels.argtypes = [sp, C.POINTER(TsdfParams), dp, u16, C.c_int32, C.c_int32, fp, u16, C.c_int64, C.c_int32,
                                    ip, fp, dp]
    xp = C.POINTER(EsdfParams)
    lib.icpk_default_esdf_params.argtypes = [xp]
    lib.icpk_default_esdf_params.restype = None
    lib.icpk_esdf_compute.argtypes = [C.c_void_p, xp, i64]
    lib.icpk_esdf_get.argtypes = [C.c_void_p, ip, u8, fp]
    lib.icpk_esdf_get_box.argtypes = [C.c_void_p, ip, ip, ip, u8, fp]
    lib.icpk_esdf_query.argtypes = [C.c_void_p, fp, fp, fp, C.c_int32, fp, fp, fp, fp, u8]
    lib.icpk_esdf_release.argtypes = [C.c_void_p]
    lib.icpk_esdf_host.argtypes = [C.POINTER(TsdfParams), xp, fp, u16, ip, u8, fp, i64]
    lib.icpk_esdf_query_host.argtypes = [C.POINTER(TsdfParams), xp, ip, u8, fp, fp, fp, C.c_int32, fp, fp, fp, fp, u8]
    bp, u32 = C.POINTER(BriefMatchParams), C.POINTER(C.c_uint32)
    lib.icpk_default_brief_match_params.argtypes = [bp]
    lib.icpk_default_brief_match_params.restype = None
    lib.icpk_describe_keypoints.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.icpk_describe_points.argtypes = [C.c_void_p, C.c_int32, u8, C.c_int32, C.c_int32, C.c_int32, fp, C.c_int32, C.c_int32]
    lib.icpk_get_descriptors.argtypes = [C.c_void_p, C.c_int32, fp, u32, u8, u8, ip]
    lib.icpk_set_descriptors.argtypes = [C.c_void_p, C.c_int32, fp, u32, u8, u8, C.c_int32]
    lib.icpk_described_to_cloud.argtypes = [C.c_void_p, C.c_int32, u16, C.c_int32, C.c_int32, C.c_float, C.c_float, fp, fp, ip]
    lib.icpk_get_descriptor_cloud_map.argtypes = [C.c_void_p, C.c_int32, ip, ip]
    lib.icpk_match_descriptors.argtypes = [C.c_void_p, bp, ip]
    lib.icpk_get_descriptor_matches.argtypes = [C.c_void_p, ip, ip, ip, ip, ip]
    lib.icpk_brief_pattern.argtypes = [C.POINTER(C.c_int8)]
    lib.icpk_brief_pattern.restype = None
    lib.icpk_brief_boundaries.argtypes = [ip]
    lib.icpk_brief_boundaries.restype = None
    lib.icpk_brief_bin.argtypes = [C.c_int32, C.c_int32]
    lib.icpk_brief_describe_host.argtypes = [u8, C.c_int32, C.c_int32, C.c_int32, fp, C.c_int32, C.c_int32, u32, u8, u8]
    lib.icpk_brief_match_host.argtypes = [u32, u8, C.c_int32, u32, u8, C.c_int32, bp, ip, ip, ip, ip, ip]
    cp = C.POINTER(ClusterParams)
    lib.icpk_cluster_dbscan.argtypes = [C.c_void_p, C.c_int32, cp, C.c_int32, ip, ip, ip]
    lib.icpk_get_clusters.argtypes = [C.c_void_p, ip, ip, ip, u8, ip, ip, ip, ip, ip]
    lib.icpk_cluster_host.argtypes = [fp, C.c_int32, cp, ip, ip, ip, ip, u8, ip, ip, ip, ip, ip]
    pp, dp = C.POINTER(PlaneParams), C.POINTER(C.c_double)
    lib.icpk_default_plane_params.argtypes = [pp]
    lib.icpk_default_plane_params.restype = None
    lib.icpk_segment_planes.argtypes = [C.c_void_p, C.c_int32, pp, C.c_int32, ip, ip, ip]
    lib.icpk_get_planes.argtypes = [C.c_void_p, ip, ip, ip, ip, dp, ip, dp]
    lib.icpk_segment_planes_host.argtypes = [fp, C.c_int32, pp, C.c_int32, ip, ip, ip, ip, ip, dp, ip, dp]
    lib.icpk_plane_fit_host.argtypes = [dp, C.c_int32, fp, dp, dp]
    _lib = lib
    return lib


def comm_unique_id():
    """ncclGetUniqueId through the C ABI: 128 opaque bytes rank 0 ships to the other ranks."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = load().icpk_comm_unique_id(buf)
    if rc != OK:
        raise IcpkError(rc, "icpk_comm_unique_id failed (librccl.so.1 not loadable?)")
    return buf.raw


def comm_partition(n_items, world, rank):
    s, c = C.c_int32(0), C.c_int32(0)
    load().icpk_comm_partition(n_items, world, rank, C.byref(s), C.byref(c))
    return s.value, c.value


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def default_params(**kw):
    p = Params()
    load().icpk_default_params(C.byref(p))
    for k, v in kw.items():
        if k in ("last_rotation", "last_translation"):
            arr = _f(v).reshape(-1)
            getattr(p, k)[:] = [float(x) for x in arr]
        else:
            setattr(p, k, v)
    return p


# ---- host helpers (no device) ------------------------------------------------
def backproject_keypoints(depth, kp_xy, fx=468.60, cx=318.27):
    """pointcloud.cpp:60-98 (host only): (points (3, m) float32, kept (m,) indices into kp_xy)."""
    depth = np.ascontiguousarray(depth, np.uint16)
    kp = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
    out = np.zeros((max(len(kp), 1), 3), np.float32)
    kept = np.zeros(max(len(kp), 1), np.int32)
    m = load().icpk_backproject_keypoints(depth.ctypes.data_as(C.POINTER(C.c_uint16)), depth.shape[0], depth.shape[1], _fp(kp),
                                          len(kp), fx, cx, _fp(out), kept.ctypes.data_as(C.POINTER(C.c_int32)))
    if m < 0:
        raise IcpkError(m, "icpk_backproject_keypoints")
    return np.ascontiguousarray(out[:m].T), kept[:m].copy()


def map_voxel(p):
    """map.cpp:55-85 getVoxelCoordinates on the host: (3,) point -> (3,) int32 voxel."""
    p = _f(p).reshape(3)
    v = np.zeros(3, np.int32)
    load().icpk_map_voxel(_fp(p), v.ctypes.data_as(C.POINTER(C.c_int32)))
    return v


def intensity_from_bgr(bgr):
    """(..., 3) uint8 BGR -> (n,) float32 intensities (b + g + r) / 765 in [0, 1], as the colour calls take them."""
    px = np.ascontiguousarray(bgr, np.uint8).reshape(-1, 3)
    out = np.zeros(len(px), np.float32)
    load().icpk_intensity_from_bgr(px.ctypes.data_as(C.POINTER(C.c_uint8)), len(px), _fp(out))
    return out


def make_rotation_matrix(x, y, z):
    out = np.zeros(9, np.float32)
    load().icpk_make_rotation_matrix(x, y, z, _fp(out))
    return out.reshape(3, 3)


def matrix_to_quaternion(m):
    m = _f(m).reshape(9)
    q = np.zeros(4, np.float32)
    load().icpk_matrix_to_quaternion(_fp(m), _fp(q))
    return q


def quaternion_to_euler(q):
    q = _f(q).reshape(4)
    e = np.zeros(3, np.float32)
    load().icpk_quaternion_to_euler(_fp(q), _fp(e))
    return e


def distance3(a, b):
    """icp.cpp:595-602 distance(cv::Point3f, cv::Point3f) on the host."""
    a = _f(a).reshape(3)
    b = _f(b).reshape(3)
    return np.float32(load().icpk_distance3(_fp(a), _fp(b)))


def solve_reference(M):
    M = _f(M).reshape(9)
    R = np.zeros(9, np.float32)
    load().icpk_solve_reference(_fp(M), _fp(R))
    return R.reshape(3, 3)


def solve_point_to_plane(sums):
    dp = C.POINTER(C.c_double)
    sums = np.ascontiguousarray(sums, np.float64)
    R = np.zeros(9)
    t = np.zeros(3)
    rc = load().icpk_solve_point_to_plane(sums.ctypes.data_as(dp), R.ctypes.data_as(dp), t.ctypes.data_as(dp))
    return R.reshape(3, 3), t, rc


def solve_kabsch(n, sa, sb, sab):
    dp = C.POINTER(C.c_double)
    sa = np.ascontiguousarray(sa, np.float64)
    sb = np.ascontiguousarray(sb, np.float64)
    sab = np.ascontiguousarray(sab, np.float64).reshape(9)
    R = np.zeros(9)
    t = np.zeros(3)
    load().icpk_solve_kabsch(int(n), sa.ctypes.data_as(dp), sb.ctypes.data_as(dp), sab.ctypes.data_as(dp),
                             R.ctypes.data_as(dp), t.ctypes.data_as(dp))
    return R.reshape(3, 3), t


def score_metrics(sums, inliers, n_source):
    """icpk_score_metrics (host only): (fitness, inlier_rmse, mean_dist) as float32 from one pose's NSCORE sums."""
    dp = C.POINTER(C.c_double)
    sums = np.ascontiguousarray(sums, np.float64).reshape(NSCORE)
    f, r, m = C.c_float(0), C.c_float(0), C.c_float(0)
    load().icpk_score_metrics(sums.ctypes.data_as(dp), int(inliers), int(n_source), C.byref(f), C.byref(r), C.byref(m))
    return np.float32(f.value), np.float32(r.value), np.float32(m.value)


def information_matrix(sums, inliers):
    """icpk_information_matrix (host only): the (6, 6) float64 sum G^T G, G = [-[q]x | I], from one pose's NSCORE sums."""
    dp = C.POINTER(C.c_double)
    sums = np.ascontiguousarray(sums, np.float64).reshape(NSCORE)
    info = np.zeros(36, np.float64)
    load().icpk_information_matrix(sums.ctypes.data_as(dp), int(inliers), info.ctypes.data_as(dp))
    return info.reshape(6, 6)


def default_pg_params(**kw):
    """icpk_default_pg_params with the given fields replaced."""
    p = PgParams()
    load().icpk_default_pg_params(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"icpk_pg_params has no field {k}")
        setattr(p, k, v)
    return p


def pg_edges(edges):
    """A sequence of (source, target, T (4, 4), info (6, 6), uncertain) as an array of icpk_pg_edge."""
    arr = (PgEdge * max(len(edges), 1))()
    v = np.frombuffer(arr, dtype=np.dtype([("source", "<i4"), ("target", "<i4"), ("uncertain", "<i4"), ("reserved", "<i4"),
                                           ("T", "<f8", 16), ("info", "<f8", 36)]))
    for k, (s, t, T, info, unc) in enumerate(edges):
        v[k] = (int(s), int(t), int(bool(unc)), 0, np.asarray(T, np.float64).reshape(16),
                np.asarray(info, np.float64).reshape(36))
    return arr


def pose_graph_check(poses, edges, params=None, n_nodes=None, n_edges=None):
    """icpk_pose_graph_check (host only): the status icpk_pose_graph_optimize / _evaluate would refuse the graph with
    (OK or E_ARG).  poses (n, 4, 4) float64 or None, edges as pg_edges takes them or None."""
    dp = C.POINTER(C.c_double)
    P = None if poses is None else np.ascontiguousarray(poses, np.float64)
    n = int(n_nodes) if n_nodes is not None else (0 if P is None else P.size // 16)
    m = int(n_edges) if n_edges is not None else (0 if edges is None else len(edges))
    return load().icpk_pose_graph_check(n, None if P is None else P.ctypes.data_as(dp), m,
                                        None if edges is None else pg_edges(edges),
                                        None if params is None else C.byref(params))


def tsdf_params(dims=None, voxel=None, origin=None, trunc=None, max_weight=None, depth_scale=None, flags=None):
    """icpk_default_tsdf_params with the given fields replaced."""
    p = TsdfParams()
    load().icpk_default_tsdf_params(C.byref(p))
    if dims is not None:
        p.dims[:] = [int(v) for v in dims]
    if origin is not None:
        p.origin[:] = [float(v) for v in origin]
    for k, v in (("voxel", voxel), ("trunc", trunc), ("max_weight", max_weight), ("depth_scale", depth_scale),
                 ("flags", flags)):
        if v is not None:
            setattr(p, k, v)
    return p


def tsdf_invert_pose(pose):
    """icpk_tsdf_invert_pose (host only): the camera-to-world pose (4, 4) float64 inverted in double and rounded to
    float once, as icpk_tsdf_integrate takes it.  Returns (R (3, 3), t (3,)) float32."""
    P = np.ascontiguousarray(pose, np.float64).reshape(16)
    R, t = np.zeros(9, np.float32), np.zeros(3, np.float32)
    rc = load().icpk_tsdf_invert_pose(P.ctypes.data_as(C.POINTER(C.c_double)), _fp(R), _fp(t))
    if rc < 0:
        raise IcpkError(rc, "icpk_tsdf_invert_pose: the pose is not finite")
    return R.reshape(3, 3), t


def tsdf_voxel_update(params, R, t, depth, tsdf, weight, intensity=None, intensity_value=None, fx=468.60, cx=318.27,
                      first=0, count=None):
    """icpk_tsdf_voxel_update (host only): the per-voxel rule for `count` voxels from linear index `first` (default:
    all that tsdf holds).  tsdf float32, weight uint16 and intensity_value float32 arrays of count entries are updated
    in place.  Returns the number of voxels written."""
    depth = np.ascontiguousarray(depth, np.uint16)
    rows, cols = depth.shape
    R, t = _f(R).reshape(9), _f(t).reshape(3)
    img = None if intensity is None else _f(intensity).reshape(-1)
    for a, dt in ((tsdf, np.float32), (weight, np.uint16), (intensity_value, np.float32)):
        if a is not None and (a.dtype != dt or not a.flags.c_contiguous):
            raise ValueError("the voxel state arrays must be contiguous float32 / uint16 / float32")
    count = tsdf.size if count is None else int(count)
    u16 = C.POINTER(C.c_uint16)
    rc = load().icpk_tsdf_voxel_update(C.byref(params), _fp(R), _fp(t), depth.ctypes.data_as(u16),
                                       None if img is None else _fp(img), rows, cols, fx, cx, int(first), count,
                                       _fp(tsdf), weight.ctypes.data_as(u16),
                                       None if intensity_value is None else _fp(intensity_value))
    if rc < 0:
        raise IcpkError(rc, "icpk_tsdf_voxel_update")
    return rc


def tsdf_raycast_params(shape=None, fx=None, cx=None, z_near=None, z_far=None, step=None, min_weight=None):
    """icpk_default_tsdf_raycast_params with the given fields replaced; shape = (rows, cols)."""
    p = TsdfRaycastParams()
    load().icpk_default_tsdf_raycast_params(C.byref(p))
    if shape is not None:
        p.rows, p.cols = int(shape[0]), int(shape[1])
    for k, v in (("fx", fx), ("cx", cx), ("z_near", z_near), ("z_far", z_far), ("step", step), ("min_weight", min_weight)):
        if v is not None:
            setattr(p, k, v)
    return p


def tsdf_raycast_pixels(params, ray, pose, tsdf, weight, intensity=None, first=0, count=None):
    """icpk_tsdf_raycast_pixels (host only): the ray rule for `count` pixels from row-major pixel `first` (default: all
    from there on) over the host planes tsdf float32, weight uint16 (and intensity float32 on a TSDF_COLOR volume).
    params: TsdfParams, ray: TsdfRaycastParams.  Returns (maps (8, count) float32: x, y, z, nx, ny, nz, depth, intensity;
    the number of listed hits)."""
    f, w = _f(tsdf).reshape(-1), np.ascontiguousarray(weight, np.uint16).reshape(-1)
    ci = None if intensity is None else _f(intensity).reshape(-1)
    n = params.dims[0] * params.dims[1] * params.dims[2]
    if f.size != n or w.size != n or (ci is not None and ci.size != n):
        raise ValueError("the planes must hold one entry per voxel")
    count = ray.rows * ray.cols - int(first) if count is None else int(count)
    out = np.zeros((8, max(count, 0)), np.float32)
    P = np.ascontiguousarray(pose, np.float64).reshape(16)
    rc = load().icpk_tsdf_raycast_pixels(C.byref(params), C.byref(ray), P.ctypes.data_as(C.POINTER(C.c_double)), _fp(f),
                                         w.ctypes.data_as(C.POINTER(C.c_uint16)), None if ci is None else _fp(ci),
                                         int(first), count, _fp(out))
    if rc < 0:
        raise IcpkError(rc, "icpk_tsdf_raycast_pixels")
    return out, rc


def default_projective_params(**kw):
    """icpk_default_projective_params with the given fields replaced (level, fx, cx, max_iterations, max_dist,
    min_normal_cos, min_pairs)."""
    p = ProjectiveParams()
    load().icpk_default_projective_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _pose16(pose):
    return np.ascontiguousarray(pose, np.float64).reshape(16)


_FERN_FIELDS = ("level", "n_ferns", "seed", "d_min", "d_max", "capacity", "harvest_above", "min_valid")


def default_fern_params(**kw):
    """icpk_default_fern_params with the given fields replaced (level, n_ferns, seed, d_min, d_max, capacity,
    harvest_above, min_valid).  harvest_above and min_valid follow n_ferns (F / 5, F / 2) unless given."""
    p = FernParams()
    load().icpk_default_fern_params(C.byref(p))
    for k, v in kw.items():
        if k not in _FERN_FIELDS:
            raise TypeError(f"icpk_fern_params has no field {k!r}")
        setattr(p, k, int(v))
    if "n_ferns" in kw:
        if "harvest_above" not in kw:
            p.harvest_above = p.n_ferns // 5
        if "min_valid" not in kw:
            p.min_valid = p.n_ferns // 2
    return p


def _fern_words(params):
    """the uint32 words of a code; 1 for an n_ferns the call will refuse before it writes"""
    F = 256 if params is None else params.n_ferns
    return F // 8 if 8 <= F <= FERN_MAX_FERNS and F % 8 == 0 else 1


def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def _fern_ref(params):
    return None if params is None else C.byref(params)


def fern_table(params, rows, cols):
    """icpk_fern_table (host only): (F, 6) int32 -- each fern's row, col and four thresholds on a level of rows x cols."""
    out = np.zeros((_fern_words(params) * 8, 6), np.int32)
    rc = load().icpk_fern_table(_fern_ref(params), int(rows), int(cols), out.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc < 0:
        raise IcpkError(rc, "icpk_fern_table: parameters outside their ranges or an empty level")
    return out


def fern_encode_host(params, level):
    """icpk_fern_encode_host (host only): (code (F / 8,) uint32, V) of a (rows, cols) uint16 level."""
    level = np.ascontiguousarray(level, np.uint16)
    if level.ndim != 2:
        raise ValueError("a (rows, cols) level expected")
    code = np.zeros(_fern_words(params), np.uint32)
    V = C.c_int32(0)
    rc = load().icpk_fern_encode_host(_fern_ref(params), level.ctypes.data_as(C.POINTER(C.c_uint16)), level.shape[0],
                                      level.shape[1], _u32p(code), C.byref(V))
    if rc < 0:
        raise IcpkError(rc, "icpk_fern_encode_host: parameters outside their ranges or an empty level")
    return code, V.value


def fern_dissimilarity_host(a, b, n_ferns=None):
    """icpk_fern_dissimilarity_host (host only): the ferns whose nibbles differ between two packed codes."""
    a, b = np.ascontiguousarray(a, np.uint32).reshape(-1), np.ascontiguousarray(b, np.uint32).reshape(-1)
    n_ferns = 8 * a.size if n_ferns is None else int(n_ferns)
    if a.size != b.size or (8 <= n_ferns <= FERN_MAX_FERNS and n_ferns != 8 * a.size):
        raise ValueError("two codes of n_ferns / 8 words expected")
    rc = load().icpk_fern_dissimilarity_host(_u32p(a), _u32p(b), n_ferns)
    if rc < 0:
        raise IcpkError(rc, "icpk_fern_dissimilarity_host: n_ferns is not a multiple of 8 in 8 .. 1024")
    return rc


def projective_pixels(params, pose, level, view, view_shape, view_fx, view_cx, view_pose, first=0, count=None,
                      terms=False):
    """icpk_projective_pixels (host only): the projective rule for `count` pixels from row-major pixel `first` of the
    (rows, cols) uint16 image `level` (default: all from there on).  view: seven float32 planes x, y, z, nx, ny, nz,
    depth of view_shape.  Returns (pixel (count,) int32: the view pixel or the PROJ_* code; dist (count,) float32;
    terms (count, 28) float64 or None; the number of pairs)."""
    img = np.ascontiguousarray(level, np.uint16)
    rows_s, cols_s = img.shape
    rows_v, cols_v = int(view_shape[0]), int(view_shape[1])
    planes = [_f(view[k]).reshape(-1) for k in range(7)]
    if any(a.size != rows_v * cols_v for a in planes):
        raise ValueError("every plane of the view must hold rows x cols entries")
    count = rows_s * cols_s - int(first) if count is None else int(count)
    n = max(count, 0)
    pixel, dist = np.zeros(n, np.int32), np.zeros(n, np.float32)
    tm = np.zeros((n, 28), np.float64) if terms else None
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    rc = load().icpk_projective_pixels(C.byref(params), _pose16(pose).ctypes.data_as(dp), img.ctypes.data_as(C.POINTER(C.c_uint16)),
                                       rows_s, cols_s, (fp * 7)(*[_fp(a) for a in planes]), rows_v, cols_v, view_fx, view_cx,
                                       _pose16(view_pose).ctypes.data_as(dp), int(first), count,
                                       pixel.ctypes.data_as(C.POINTER(C.c_int32)), _fp(dist),
                                       None if tm is None else tm.ctypes.data_as(dp))
    if rc < 0:
        raise IcpkError(rc, "icpk_projective_pixels")
    return pixel, dist, tm, rc


def tsdf_mesh_host(params, tsdf, weight, intensity=None, min_weight=1, cap_vertices=None, cap_triangles=None):
    """icpk_tsdf_mesh_host (host only): the mesh rule over the host planes tsdf float32, weight uint16 (and intensity
    float32 on a TSDF_COLOR volume).  Returns dict(vertices (3, n), normals (3, n), intensity (n,), voxel_index (n,)
    int32, edge (n,) uint8, triangles (m, 3) int32, n_vertices, n_triangles, n_no_normal).  cap_vertices / cap_triangles:
    the room the arrays are given (default: what a first, counting call asks for); when the mesh does not fit, IcpkError
    is raised with the counts in its `counts` attribute."""
    f, w = _f(tsdf).reshape(-1), np.ascontiguousarray(weight, np.uint16).reshape(-1)
    ci = None if intensity is None else _f(intensity).reshape(-1)
    n = params.dims[0] * params.dims[1] * params.dims[2]
    if f.size != n or w.size != n or (ci is not None and ci.size != n):
        raise ValueError("the planes must hold one entry per voxel")
    lib = load()
    counts = np.full(3, -1, np.int64)
    planes = (_fp(f), w.ctypes.data_as(C.POINTER(C.c_uint16)), None if ci is None else _fp(ci))
    cp = counts.ctypes.data_as(C.POINTER(C.c_int64))

    def refuse(rc):
        e = IcpkError(rc, "icpk_tsdf_mesh_host")
        e.counts = tuple(int(c) for c in counts)
        raise e

    if cap_vertices is None or cap_triangles is None:
        lib.icpk_tsdf_mesh_host(C.byref(params), int(min_weight), *planes, 0, 0, *([None] * 10), cp)
        if counts[0] < 0:
            refuse(E_ARG)
        cap_vertices = int(counts[0]) if cap_vertices is None else cap_vertices
        cap_triangles = int(counts[1]) if cap_triangles is None else cap_triangles
    nv, nt = max(int(cap_vertices), 1), max(int(cap_triangles), 1)
    pts, nrm = np.zeros((3, nv), np.float32), np.zeros((3, nv), np.float32)
    inten, vox, edge = np.zeros(nv, np.float32), np.zeros(nv, np.int32), np.zeros(nv, np.uint8)
    tri = np.zeros((nt, 3), np.int32)
    i32 = C.POINTER(C.c_int32)
    rc = lib.icpk_tsdf_mesh_host(C.byref(params), int(min_weight), *planes, int(cap_vertices), int(cap_triangles),
                                 _fp(pts[0]), _fp(pts[1]), _fp(pts[2]), _fp(nrm[0]), _fp(nrm[1]), _fp(nrm[2]), _fp(inten),
                                 vox.ctypes.data_as(i32), edge.ctypes.data_as(C.POINTER(C.c_uint8)), tri.ctypes.data_as(i32), cp)
    if rc < 0:
        refuse(rc)
    n, m = int(counts[0]), int(counts[1])
    return dict(vertices=pts[:, :n], normals=nrm[:, :n], intensity=inten[:n], voxel_index=vox[:n], edge=edge[:n],
                triangles=tri[:m], n_vertices=n, n_triangles=m, n_no_normal=int(counts[2]))


def global_hypotheses(matches, src, tgt, seed, edge_similarity=0.9, h0=0, count=1):
    """icpk_global_hypotheses (host only): hypotheses h0 .. h0 + count - 1 of icpk_register_global's draw over `matches`
    ((src_index, tgt_index) int arrays) and the clouds src, tgt ((3, n) float32).  Returns (samples (count, 3) int32,
    valid (count,) bool, T (count, 4, 4) float32)."""
    ip, u8 = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    ms = np.ascontiguousarray(matches[0], np.int32).reshape(-1)
    mt = np.ascontiguousarray(matches[1], np.int32).reshape(-1)
    s = [_f(src[k]) for k in range(3)]
    t = [_f(tgt[k]) for k in range(3)]
    count = int(count)
    samples = np.zeros((max(count, 1), 3), np.int32)
    valid = np.zeros(max(count, 1), np.uint8)
    T = np.zeros((max(count, 1), 16), np.float32)
    rc = load().icpk_global_hypotheses(ms.ctypes.data_as(ip), mt.ctypes.data_as(ip), ms.size, _fp(s[0]), _fp(s[1]),
                                       _fp(s[2]), s[0].size, _fp(t[0]), _fp(t[1]), _fp(t[2]), t[0].size, int(seed),
                                       float(edge_similarity), int(h0), count, samples.ctypes.data_as(ip),
                                       valid.ctypes.data_as(u8), _fp(T))
    if rc < 0:
        raise IcpkError(rc, "icpk_global_hypotheses")
    return samples[:count], valid[:count].astype(bool), T[:count].reshape(count, 4, 4)


# -- the moving volume (K23): functions over a Context, which gains no name ------------------------------------------
def _i3(v, what):
    a = np.ascontiguousarray(v, np.int32).reshape(-1)
    if a.size != 3:
        raise ValueError(f"{what}: three integers expected")
    return a


def tsdf_shift(ctx, s):
    """icpk_tsdf_shift: the context's volume moved by s = (s_x, s_y, s_z) whole voxels -- the new voxel v holds the old
    voxel v + s, or nothing.  Drops the surface list, the ray-cast maps and the mesh (s = 0: a no-op).  No host wait."""
    s = _i3(s, "s")
    ctx._chk(ctx._lib.icpk_tsdf_shift(ctx._h, s.ctypes.data_as(C.POINTER(C.c_int32))))
    if s.any():
        ctx._tsdf_n = ctx._tsdf_ray = ctx._tsdf_mesh = None


def tsdf_extract_leaving(ctx, s, min_weight=1):
    """icpk_tsdf_extract_leaving: the surface list restricted to the crossings a shift by s would lose; it replaces the
    surface list (Context.tsdf_get_surface, tsdf_surface_to_target).  Returns (n_points, n_no_normal)."""
    s = _i3(s, "s")
    n, m = C.c_int32(-1), C.c_int32(-1)
    ctx._chk(ctx._lib.icpk_tsdf_extract_leaving(ctx._h, int(min_weight), s.ctypes.data_as(C.POINTER(C.c_int32)),
                                                C.byref(n), C.byref(m)))
    ctx._tsdf_n = n.value
    return n.value, m.value


def tsdf_get_params(ctx):
    """icpk_tsdf_get_params: (TsdfParams with the current origin, total (3,) int64: the cumulative shift)."""
    p, total = TsdfParams(), np.zeros(3, np.int64)
    ctx._chk(ctx._lib.icpk_tsdf_get_params(ctx._h, C.byref(p), total.ctypes.data_as(C.POINTER(C.c_int64))))
    return p, total


def tsdf_get_box(ctx, lo, hi, tsdf=True, weight=True, intensity=False):
    """icpk_tsdf_get_box: (tsdf, weight, intensity) of the sub-box lo <= (x, y, z) < hi as (hi_z - lo_z, hi_y - lo_y,
    hi_x - lo_x) arrays; None where not asked."""
    lo, hi = _i3(lo, "lo"), _i3(hi, "hi")
    shape = tuple(max(int(hi[a]) - int(lo[a]), 1) for a in (2, 1, 0))  # (an empty box: the call refuses it)
    f = np.empty(shape, np.float32) if tsdf else None
    w = np.empty(shape, np.uint16) if weight else None
    c = np.empty(shape, np.float32) if intensity else None
    i32 = C.POINTER(C.c_int32)
    ctx._chk(ctx._lib.icpk_tsdf_get_box(ctx._h, lo.ctypes.data_as(i32), hi.ctypes.data_as(i32),
                                        None if f is None else _fp(f),
                                        None if w is None else w.ctypes.data_as(C.POINTER(C.c_uint16)),
                                        None if c is None else _fp(c)))
    return f, w, c


# -- signed updates of the volume (K30): functions over a Context, like the moving volume's above ---------------------
TSDF_MAX_OPS = 16


def tsdf_ops(ops):
    """A list of (sign, frame, pose (4, 4) float64) as a TsdfOp array."""
    arr = (TsdfOp * max(len(ops), 1))()
    for k, (sign, frame, pose) in enumerate(ops):
        arr[k].sign, arr[k].frame = int(sign), int(frame)
        arr[k].pose[:] = np.ascontiguousarray(pose, np.float64).reshape(16).tolist()
    return arr


def _tsdf_frames(frames, intensities):
    """The images of an op-list call as ctypes pointer tables (and the arrays that keep them alive)."""
    d = [np.ascontiguousarray(f, np.uint16) for f in frames]
    if not d or d[0].ndim != 2 or any(f.shape != d[0].shape for f in d):
        raise ValueError("frames: at least one (rows, cols) depth image, all of one shape")
    u16 = C.POINTER(C.c_uint16)
    dt = (u16 * len(d))(*[f.ctypes.data_as(u16) for f in d])
    img, it = None, None
    if intensities is not None:
        img = [_f(i).reshape(-1) for i in intensities]
        if len(img) != len(d) or any(i.size != d[0].size for i in img):
            raise ValueError("one intensity image per frame, one intensity per pixel expected")
        it = (C.POINTER(C.c_float) * len(img))(*[_fp(i) for i in img])
    return d, img, dt, it


def tsdf_apply(ctx, frames, ops, intensities=None, fx=468.60, cx=318.27):
    """icpk_tsdf_apply: the signed ops -- a list of (sign, frame, pose): +1 integrates, -1 de-integrates frames[frame]
    at pose -- applied to the context's volume in order, in one pass over it.  frames: (rows, cols) uint16 images of
    one shape; intensities: as many float32 images on a TSDF_COLOR volume.  Returns the voxels every op wrote
    (n_ops,) int64."""
    d, img, dt, it = _tsdf_frames(frames, intensities)
    n = np.zeros(max(len(ops), 1), np.int64)
    ctx._chk(ctx._lib.icpk_tsdf_apply(ctx._h, len(d), dt, it, d[0].shape[0], d[0].shape[1], fx, cx, len(ops), tsdf_ops(ops),
                                      n.ctypes.data_as(C.POINTER(C.c_int64))))
    return n[:len(ops)]


def tsdf_deintegrate(ctx, depth, pose, intensity=None, fx=468.60, cx=318.27):
    """icpk_tsdf_deintegrate: one frame taken out of the volume again -- the inverse of Context.tsdf_integrate with the
    same arguments, up to rounding (exact on voxels the frame alone had written).  Returns the voxels written."""
    d = np.ascontiguousarray(depth, np.uint16)
    rows, cols = d.shape
    P = np.ascontiguousarray(pose, np.float64).reshape(16)
    img = None if intensity is None else _f(intensity).reshape(-1)
    if img is not None and img.size != rows * cols:
        raise ValueError("one intensity per pixel expected")
    n = C.c_int32(-1)
    ctx._chk(ctx._lib.icpk_tsdf_deintegrate(ctx._h, d.ctypes.data_as(C.POINTER(C.c_uint16)), None if img is None else _fp(img),
                                            rows, cols, fx, cx, P.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)))
    return n.value


def tsdf_voxel_apply(params, frames, ops, tsdf, weight, intensities=None, intensity_value=None, fx=468.60, cx=318.27,
                     first=0, count=None):
    """icpk_tsdf_voxel_apply (host only): the signed update rule for `count` voxels from linear index `first` (default:
    all that tsdf holds); tsdf float32, weight uint16 and intensity_value float32 arrays of count entries are updated in
    place.  Returns the voxels every op wrote among them (n_ops,) int64."""
    d, img, dt, it = _tsdf_frames(frames, intensities)
    for a, t in ((tsdf, np.float32), (weight, np.uint16), (intensity_value, np.float32)):
        if a is not None and (a.dtype != t or not a.flags.c_contiguous):
            raise ValueError("the voxel state arrays must be contiguous float32 / uint16 / float32")
    count = tsdf.size if count is None else int(count)
    n = np.zeros(max(len(ops), 1), np.int64)
    rc = load().icpk_tsdf_voxel_apply(C.byref(params), len(d), dt, it, d[0].shape[0], d[0].shape[1], fx, cx, len(ops),
                                      tsdf_ops(ops), int(first), count, _fp(tsdf),
                                      weight.ctypes.data_as(C.POINTER(C.c_uint16)),
                                      None if intensity_value is None else _fp(intensity_value),
                                      n.ctypes.data_as(C.POINTER(C.c_int64)))
    if rc < 0:
        raise IcpkError(rc, "icpk_tsdf_voxel_apply")
    return n[:len(ops)]


# ---- projective frame-to-model alignment (K25): functions of a context, like the moving volume's above ----------------
def _projective(params, kw):
    return params if params is not None else default_projective_params(**kw)


def projective_associate(ctx, pose, params=None, **kw):
    """icpk_projective_associate at the camera-to-world pose (4, 4) float64: (pixel (rows, cols) int32 -- the view pixel
    every pixel of the pyramid level pairs with, or its PROJ_* code --, dist (rows, cols) float32).  params:
    ProjectiveParams, or its fields as keywords."""
    p = _projective(params, kw)
    P = _pose16(pose)
    dp = C.POINTER(C.c_double)
    r, c = C.c_int32(0), C.c_int32(0)
    if ctx._lib.icpk_depth_pyramid_shape(ctx._h, int(p.level), C.byref(r), C.byref(c)) != OK:
        # (no such level: the call states its own refusal, and needs no arrays for it)
        ctx._chk(ctx._lib.icpk_projective_associate(ctx._h, C.byref(p), P.ctypes.data_as(dp), None, None))
        raise IcpkError(E_ARG, "a level the pyramid does not have")
    pixel, dist = np.zeros((r.value, c.value), np.int32), np.zeros((r.value, c.value), np.float32)
    ctx._chk(ctx._lib.icpk_projective_associate(ctx._h, C.byref(p), P.ctypes.data_as(dp),
                                                pixel.ctypes.data_as(C.POINTER(C.c_int32)), _fp(dist)))
    return pixel, dist


def projective_reduce(ctx, pose, params=None, **kw):
    """icpk_projective_reduce: (28 float64 sums, pair count) of one evaluation at the pose."""
    p = _projective(params, kw)
    P = _pose16(pose)
    sums, n = np.zeros(28, np.float64), C.c_int64(-1)
    dp = C.POINTER(C.c_double)
    ctx._chk(ctx._lib.icpk_projective_reduce(ctx._h, C.byref(p), P.ctypes.data_as(dp), sums.ctypes.data_as(dp), C.byref(n)))
    return sums, n.value


def align_projective(ctx, pose, params=None, **kw):
    """icpk_align_projective from the camera-to-world pose (4, 4) float64: (pose (4, 4) float64, ProjectiveResult).  The
    result's status is OK, W_TOO_FEW_PAIRS or W_DEGENERATE; its count and mean_dist are those of the last evaluated
    iteration, i.e. at the estimate before the last update."""
    p = _projective(params, kw)
    P = _pose16(pose)
    out, res = np.zeros(16, np.float64), ProjectiveResult()
    dp = C.POINTER(C.c_double)
    ctx._chk(ctx._lib.icpk_align_projective(ctx._h, C.byref(p), P.ctypes.data_as(dp), out.ctypes.data_as(dp), C.byref(res)))
    return out.reshape(4, 4), res


def projective_trace(ctx):
    """icpk_get_projective_trace: the evaluated iterations of the last align_projective, a list of dict(pose (3, 4)
    float64 E_k, sums (28,), count, status)."""
    buf = (ProjectiveIter * PROJECTIVE_MAX_ITERATIONS)()
    n = ctx._chk(ctx._lib.icpk_get_projective_trace(ctx._h, buf, PROJECTIVE_MAX_ITERATIONS))
    return [dict(pose=np.array(buf[k].pose, np.float64).reshape(3, 4), sums=np.array(buf[k].sums, np.float64),
                 count=int(buf[k].count), status=int(buf[k].status)) for k in range(n)]


# ---- the photometric term of the projective alignment (K26): functions of a context and three host-only ones ---------
def default_projective_color_params(**kw):
    """icpk_default_projective_color_params with the given fields replaced (lambda_geometric)."""
    c = ProjectiveColorParams()
    load().icpk_default_projective_color_params(C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _projective_color(color):
    if color is None:
        return default_projective_color_params()
    return color if isinstance(color, ProjectiveColorParams) else default_projective_color_params(**dict(color))


def set_pyramid_intensity(ctx, intensity):
    """icpk_depth_pyramid_set_intensity: the (rows, cols) float32 image in [0, 1] beside the resident depth pyramid's
    level 0; every level the depth pyramid has is built.  The next depth_front.build_pyramid drops them."""
    img = _f(intensity)
    if img.ndim != 2:
        raise ValueError("intensity must be a (rows, cols) image")
    ctx._chk(ctx._lib.icpk_depth_pyramid_set_intensity(ctx._h, _fp(img), img.shape[0], img.shape[1]))


def pyramid_intensity(ctx, level):
    """icpk_depth_pyramid_get_intensity: the level's (rows, cols) float32 intensities."""
    r, c = C.c_int32(1), C.c_int32(1)
    if ctx._lib.icpk_depth_pyramid_shape(ctx._h, int(level), C.byref(r), C.byref(c)) != OK:
        r, c = C.c_int32(1), C.c_int32(1)  # (the call states its own refusal)
    out = np.zeros((r.value, c.value), np.float32)
    ctx._chk(ctx._lib.icpk_depth_pyramid_get_intensity(ctx._h, int(level), _fp(out)))
    return out


def intensity_pyramid_host(depth, intensity, level, params=None):
    """icpk_intensity_pyramid_host (host only): level `level` of the intensity pyramid of the two (rows, cols) images."""
    d, img = np.ascontiguousarray(depth, np.uint16), _f(intensity)
    if d.ndim != 2 or d.shape != img.shape:
        raise ValueError("depth and intensity must be (rows, cols) images of one shape")
    p = params
    if p is None:
        p = PyramidParams()
        load().icpk_default_pyramid_params(C.byref(p))
    r, c = d.shape
    for _ in range(max(int(level), 0)):
        r, c = (r + 1) // 2, (c + 1) // 2
    out = np.zeros((r, c), np.float32)
    rc = load().icpk_intensity_pyramid_host(C.byref(p), d.ctypes.data_as(C.POINTER(C.c_uint16)), _fp(img), d.shape[0], d.shape[1],
                                            int(level), _fp(out))
    if rc < 0:
        raise IcpkError(rc, "icpk_intensity_pyramid_host")
    return out


def raycast_color_gradients(ctx, radius, min_neighbors=4, keep_sums=False):
    """icpk_tsdf_raycast_color_gradients: the colour gradients of the last ray cast, kept on the device.  No host wait."""
    ctx._chk(ctx._lib.icpk_tsdf_raycast_color_gradients(ctx._h, float(radius), int(min_neighbors),
                                                        COLOR_KEEP_SUMS if keep_sums else 0))


def get_raycast_color_gradients(ctx, sums=False):
    """icpk_tsdf_get_raycast_color_gradients: (3, rows, cols) float32; sums=True: also the (rows, cols, 10) int64 words of
    icpk_tsdf_get_raycast_color_gradient_sums."""
    shape = ctx._tsdf_ray
    if shape is None:
        ctx._chk(ctx._lib.icpk_tsdf_get_raycast_color_gradients(ctx._h, None, None, None))  # (ICPK_E_NOT_SET)
        raise IcpkError(E_NOT_SET, "no ray cast (tsdf_raycast)")
    g = np.zeros((3,) + tuple(shape), np.float32)
    ctx._chk(ctx._lib.icpk_tsdf_get_raycast_color_gradients(ctx._h, _fp(g[0]), _fp(g[1]), _fp(g[2])))
    if not sums:
        return g
    S = np.zeros(tuple(shape) + (10,), np.int64)
    ctx._chk(ctx._lib.icpk_tsdf_get_raycast_color_gradient_sums(ctx._h, S.ctypes.data_as(C.POINTER(C.c_int64))))
    return g, S


def raycast_color_gradients_host(view, radius, min_neighbors=4, first=0, count=None):
    """icpk_raycast_color_gradients_host (host only): view (8, rows, cols) float32.  Returns (sums (count, 10) int64,
    gradients (count, 3) float32, the number of pixels with a non-zero gradient)."""
    v = _f(view)
    if v.ndim != 3 or v.shape[0] != 8:
        raise ValueError("view must be (8, rows, cols)")
    rows, cols = v.shape[1:]
    count = rows * cols - int(first) if count is None else int(count)
    n = max(count, 0)
    S, g = np.zeros((n, 10), np.int64), np.zeros((n, 3), np.float32)
    fp = C.POINTER(C.c_float)
    rc = load().icpk_raycast_color_gradients_host((fp * 8)(*[_fp(v[k]) for k in range(8)]), rows, cols, float(radius),
                                                  int(min_neighbors), int(first), count, S.ctypes.data_as(C.POINTER(C.c_int64)),
                                                  _fp(g))
    if rc < 0:
        raise IcpkError(rc, "icpk_raycast_color_gradients_host")
    return S, g, rc


def projective_reduce_colored(ctx, pose, params=None, color=None, **kw):
    """icpk_projective_reduce_colored: (28 float64 sums, pair count) of one evaluation of the joint step at the pose.
    color: ProjectiveColorParams, a dict of its fields, or None for the defaults."""
    p, c = _projective(params, kw), _projective_color(color)
    P = _pose16(pose)
    sums, n = np.zeros(28, np.float64), C.c_int64(-1)
    dp = C.POINTER(C.c_double)
    ctx._chk(ctx._lib.icpk_projective_reduce_colored(ctx._h, C.byref(p), C.byref(c), P.ctypes.data_as(dp), sums.ctypes.data_as(dp),
                                                     C.byref(n)))
    return sums, n.value


def align_projective_colored(ctx, pose, params=None, color=None, **kw):
    """icpk_align_projective_colored: align_projective with the joint step; projective_trace reads its iterations."""
    p, c = _projective(params, kw), _projective_color(color)
    P = _pose16(pose)
    out, res = np.zeros(16, np.float64), ProjectiveResult()
    dp = C.POINTER(C.c_double)
    ctx._chk(ctx._lib.icpk_align_projective_colored(ctx._h, C.byref(p), C.byref(c), P.ctypes.data_as(dp), out.ctypes.data_as(dp),
                                                    C.byref(res)))
    return out.reshape(4, 4), res


def projective_pixels_colored(params, pose, level, view, view_shape, view_fx, view_cx, view_pose, level_intensity, gradient,
                              color=None, first=0, count=None, terms=False):
    """icpk_projective_pixels_colored (host only): projective_pixels with the coloured rule 9.  view: EIGHT planes (the
    eighth is the view's intensity); level_intensity: the level's (rows, cols) float32; gradient: (3, rows_v, cols_v)."""
    img = np.ascontiguousarray(level, np.uint16)
    rows_s, cols_s = img.shape
    rows_v, cols_v = int(view_shape[0]), int(view_shape[1])
    planes = [_f(view[k]).reshape(-1) for k in range(8)]
    grads = [_f(gradient[k]).reshape(-1) for k in range(3)]
    li = _f(level_intensity).reshape(-1)
    if any(a.size != rows_v * cols_v for a in planes + grads) or li.size != rows_s * cols_s:
        raise ValueError("every plane must hold rows x cols entries")
    count = rows_s * cols_s - int(first) if count is None else int(count)
    n = max(count, 0)
    pixel, dist = np.zeros(n, np.int32), np.zeros(n, np.float32)
    tm = np.zeros((n, 28), np.float64) if terms else None
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    c = _projective_color(color)
    rc = load().icpk_projective_pixels_colored(
        C.byref(params), _pose16(pose).ctypes.data_as(dp), img.ctypes.data_as(C.POINTER(C.c_uint16)), rows_s, cols_s,
        (fp * 7)(*[_fp(a) for a in planes[:7]]), rows_v, cols_v, view_fx, view_cx, _pose16(view_pose).ctypes.data_as(dp),
        int(first), count, pixel.ctypes.data_as(C.POINTER(C.c_int32)), _fp(dist), None if tm is None else tm.ctypes.data_as(dp),
        _fp(li), _fp(planes[7]), (fp * 3)(*[_fp(a) for a in grads]), C.byref(c))
    if rc < 0:
        raise IcpkError(rc, "icpk_projective_pixels_colored")
    return pixel, dist, tm, rc


# ---- K27: fern keyframe relocalisation.  Functions over a context: the class itself gains no method ----
def fern_create(ctx, rows, cols, params=None, **kw):
    """icpk_fern_create: a keyframe database for levels of rows x cols (it replaces the context's previous one).
    params: a FernParams, or fields of default_fern_params as keywords.  Returns the FernParams in force."""
    p = default_fern_params(**kw) if params is None else params
    ctx._chk(ctx._lib.icpk_fern_create(ctx._h, C.byref(p), int(rows), int(cols)))
    ctx._fern = FernParams.from_buffer_copy(p)
    return ctx._fern


def _fern_w(ctx):
    p = getattr(ctx, "_fern", None)
    return 1 if p is None else p.n_ferns // 8


def fern_reset(ctx):
    ctx._chk(ctx._lib.icpk_fern_reset(ctx._h))


def fern_destroy(ctx):
    ctx._chk(ctx._lib.icpk_fern_destroy(ctx._h))
    ctx._fern = None


def fern_count(ctx):
    return ctx._chk(ctx._lib.icpk_fern_count(ctx._h))


def fern_encode(ctx):
    """icpk_fern_encode: the database's level of the resident pyramid into the current code.  Returns (code
    (F / 8,) uint32, V)."""
    code, V = np.zeros(_fern_w(ctx), np.uint32), C.c_int32(0)
    ctx._chk(ctx._lib.icpk_fern_encode(ctx._h, _u32p(code), C.byref(V)))
    return code, V.value


def _fern_lists(n, idx, diss):
    return idx[:n.value].copy(), diss[:n.value].copy()


def fern_query(ctx, k=3):
    """icpk_fern_query: the min(k, n) nearest keyframes of the current code, (index, diss) int32 arrays in ascending
    (diss, index) order."""
    idx, diss, n = np.zeros(FERN_MAX_K, np.int32), np.zeros(FERN_MAX_K, np.int32), C.c_int32(0)
    ip = C.POINTER(C.c_int32)
    ctx._chk(ctx._lib.icpk_fern_query(ctx._h, int(k), idx.ctypes.data_as(ip), diss.ctypes.data_as(ip), C.byref(n)))
    return _fern_lists(n, idx, diss)


def fern_add(ctx, pose):
    """icpk_fern_add: the current code becomes a keyframe with this (4, 4) pose.  Returns its index."""
    i = C.c_int32(-1)
    ctx._chk(ctx._lib.icpk_fern_add(ctx._h, _pose16(pose).ctypes.data_as(C.POINTER(C.c_double)), C.byref(i)))
    return i.value


def fern_process(ctx, pose=None, k=3):
    """icpk_fern_process: encode, search and -- with a pose, when the harvest rule says so -- append.  Returns
    dict(index, diss (the search BEFORE the append), valid, added (the new keyframe's index or -1))."""
    idx, diss, n = np.zeros(FERN_MAX_K, np.int32), np.zeros(FERN_MAX_K, np.int32), C.c_int32(0)
    V, added = C.c_int32(0), C.c_int32(-1)
    ip = C.POINTER(C.c_int32)
    pp = None if pose is None else _pose16(pose)
    ctx._chk(ctx._lib.icpk_fern_process(ctx._h, None if pp is None else pp.ctypes.data_as(C.POINTER(C.c_double)), int(k),
                                          idx.ctypes.data_as(ip), diss.ctypes.data_as(ip), C.byref(n), C.byref(V),
                                          C.byref(added)))
    index, diss = _fern_lists(n, idx, diss)
    return dict(index=index, diss=diss, valid=V.value, added=added.value)


def fern_add_code(ctx, code, pose):
    """icpk_fern_add_code: a host code (F / 8,) uint32 becomes a keyframe.  Returns its index."""
    code = np.ascontiguousarray(code, np.uint32).reshape(-1)
    if getattr(ctx, "_fern", None) is not None and code.size != _fern_w(ctx):
        raise ValueError("a code of n_ferns / 8 words expected")
    i = C.c_int32(-1)
    ctx._chk(ctx._lib.icpk_fern_add_code(ctx._h, _u32p(code), _pose16(pose).ctypes.data_as(C.POINTER(C.c_double)),
                                           C.byref(i)))
    return i.value


def fern_keyframe(ctx, index):
    """icpk_fern_get_keyframe: (code (F / 8,) uint32, pose (4, 4) float64) of one keyframe."""
    code, pose = np.zeros(_fern_w(ctx), np.uint32), np.zeros(16, np.float64)
    ctx._chk(ctx._lib.icpk_fern_get_keyframe(ctx._h, int(index), _u32p(code), pose.ctypes.data_as(C.POINTER(C.c_double))))
    return code, pose.reshape(4, 4)


# ---- the frame view (K28): functions of a context, like the projective calls above, and a host-only one -----------------
def frame_view_pixels(depth, pose, fx=468.60, cx=318.27, level=0, intensity=None, first=0, count=None):
    """icpk_frame_view_pixels (host only): THE FRAME VIEW RULE for `count` pixels from row-major pixel `first` of the
    (rows, cols) uint16 image `depth` -- the level's own image; `level` only scales fx, cx -- at the camera-to-world
    `pose`.  intensity: the level's (rows, cols) float32, or None.  Returns (planes (8, count) float32: x, y, z, nx, ny,
    nz, depth, intensity; n_valid; n_no_normal)."""
    img = np.ascontiguousarray(depth, np.uint16)
    if img.ndim != 2:
        raise ValueError("depth: a (rows, cols) image expected")
    inten = None if intensity is None else _f(intensity).reshape(img.shape)
    count = img.size - int(first) if count is None else int(count)
    out, none = np.zeros((8, max(count, 1)), np.float32), C.c_int32(-1)
    P = None if pose is None else _pose16(pose)
    rc = load().icpk_frame_view_pixels(float(fx), float(cx), int(level), None if P is None else P.ctypes.data_as(C.POINTER(C.c_double)),
                                       img.ctypes.data_as(C.POINTER(C.c_uint16)), None if inten is None else _fp(inten),
                                       img.shape[0], img.shape[1], int(first), count, _fp(out), C.byref(none))
    if rc < 0:
        raise IcpkError(rc, "icpk_frame_view_pixels")
    return out[:, :count], rc, none.value


def frame_view_build(ctx, pose, fx=468.60, cx=318.27, counts=True):
    """icpk_frame_view_build: every level of the resident pyramid as eight planes in world coordinates at the
    camera-to-world `pose`, kept by the context until the next build or frame_view_release.  Returns (n_valid,
    n_no_normal), one int per level; counts=False: None, and the call does not wait."""
    P = None if pose is None else _pose16(pose)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    nv, nn = np.full(PYRAMID_MAX_LEVELS, -1, np.int32), np.full(PYRAMID_MAX_LEVELS, -1, np.int32)
    ctx._chk(ctx._lib.icpk_frame_view_build(ctx._h, float(fx), float(cx), None if P is None else P.ctypes.data_as(dp),
                                              nv.ctypes.data_as(ip) if counts else None,
                                              nn.ctypes.data_as(ip) if counts else None))
    if not counts:
        return None
    L = frame_view_levels(ctx)
    return [int(x) for x in nv[:L]], [int(x) for x in nn[:L]]


def frame_view_levels(ctx):
    """icpk_frame_view_levels: the levels of the snapshot (0 without one)."""
    return ctx._chk(ctx._lib.icpk_frame_view_levels(ctx._h))


def frame_view_shape(ctx, level):
    """icpk_frame_view_shape: (rows, cols) of a level of the snapshot."""
    r, c = C.c_int32(0), C.c_int32(0)
    ctx._chk(ctx._lib.icpk_frame_view_shape(ctx._h, int(level), C.byref(r), C.byref(c)))
    return r.value, c.value


def frame_view(ctx, level):
    """icpk_frame_view_get: the (8, rows, cols) float32 planes x, y, z, nx, ny, nz, depth, intensity of a level."""
    rows, cols = frame_view_shape(ctx, level)
    out = np.zeros((8, rows, cols), np.float32)
    ctx._chk(ctx._lib.icpk_frame_view_get(ctx._h, int(level), (C.POINTER(C.c_float) * 8)(*[_fp(out[k]) for k in range(8)])))
    return out


def frame_view_release(ctx):
    """icpk_frame_view_release: drops the snapshot and its memory."""
    ctx._chk(ctx._lib.icpk_frame_view_release(ctx._h))


def frame_view_color_gradients(ctx, level, radius, min_neighbors=4):
    """icpk_frame_view_color_gradients: THE VIEW GRADIENT RULE over a level of the snapshot, kept beside it.  No wait."""
    ctx._chk(ctx._lib.icpk_frame_view_color_gradients(ctx._h, int(level), float(radius), int(min_neighbors), 0))


def frame_view_get_color_gradients(ctx, level):
    """icpk_frame_view_get_color_gradients: (3, rows, cols) float32."""
    rows, cols = frame_view_shape(ctx, level)
    g = np.zeros((3, rows, cols), np.float32)
    ctx._chk(ctx._lib.icpk_frame_view_get_color_gradients(ctx._h, int(level), _fp(g[0]), _fp(g[1]), _fp(g[2])))
    return g


def projective_set_view(ctx, which, view_level=0):
    """icpk_projective_set_view: VIEW_RAYCAST (the default) or VIEW_FRAME with the snapshot's level the projective
    calls (align_projective and its neighbours) then read."""
    ctx._chk(ctx._lib.icpk_projective_set_view(ctx._h, int(which), int(view_level)))


# ---- depth frames tracked directly against the TSDF (K29): functions of a context and one host-only one ---------------
def default_sdf_params(**kw):
    """icpk_default_sdf_params with the given fields replaced (level, fx, cx, max_iterations, max_abs_tsdf, min_weight,
    min_normal_cos, min_pairs)."""
    p = SdfParams()
    load().icpk_default_sdf_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _sdf(params, kw):
    return params if params is not None else default_sdf_params(**kw)


def sdf_associate(ctx, pose, params=None, **kw):
    """icpk_sdf_associate at the camera-to-world pose (4, 4) float64: (cell (rows, cols) int32 -- the linear index of the
    lowest corner of the cell every pixel of the pyramid level lands in, or its SDF_* code --, value (rows, cols) float32:
    the signed distance D there, 0 for a rejected pixel).  params: SdfParams, or its fields as keywords."""
    p = _sdf(params, kw)
    P = _pose16(pose)
    dp = C.POINTER(C.c_double)
    r, c = C.c_int32(0), C.c_int32(0)
    if ctx._lib.icpk_depth_pyramid_shape(ctx._h, int(p.level), C.byref(r), C.byref(c)) != OK:
        # (no such level: the call states its own refusal, and needs no arrays for it)
        ctx._chk(ctx._lib.icpk_sdf_associate(ctx._h, C.byref(p), P.ctypes.data_as(dp), None, None))
        raise IcpkError(E_ARG, "a level the pyramid does not have")
    cell, value = np.zeros((r.value, c.value), np.int32), np.zeros((r.value, c.value), np.float32)
    ctx._chk(ctx._lib.icpk_sdf_associate(ctx._h, C.byref(p), P.ctypes.data_as(dp), cell.ctypes.data_as(C.POINTER(C.c_int32)),
                                         _fp(value)))
    return cell, value


def sdf_reduce(ctx, pose, params=None, **kw):
    """icpk_sdf_reduce: (28 float64 sums, accepted pixels) of one evaluation at the pose."""
    p = _sdf(params, kw)
    P = _pose16(pose)
    sums, n = np.zeros(28, np.float64), C.c_int64(-1)
    dp = C.POINTER(C.c_double)
    ctx._chk(ctx._lib.icpk_sdf_reduce(ctx._h, C.byref(p), P.ctypes.data_as(dp), sums.ctypes.data_as(dp), C.byref(n)))
    return sums, n.value


def align_sdf(ctx, pose, params=None, **kw):
    """icpk_align_sdf from the camera-to-world pose (4, 4) float64: (pose (4, 4) float64, ProjectiveResult).  The result's
    status is OK, W_TOO_FEW_PAIRS or W_DEGENERATE; its count and mean_dist (the mean |D|) are those of the last evaluated
    iteration, i.e. at the estimate before the last update."""
    p = _sdf(params, kw)
    P = _pose16(pose)
    out, res = np.zeros(16, np.float64), ProjectiveResult()
    dp = C.POINTER(C.c_double)
    ctx._chk(ctx._lib.icpk_align_sdf(ctx._h, C.byref(p), P.ctypes.data_as(dp), out.ctypes.data_as(dp), C.byref(res)))
    return out.reshape(4, 4), res


def sdf_trace(ctx):
    """icpk_get_sdf_trace: the evaluated iterations of the last align_sdf, a list of dict(pose (3, 4) float64 E_k, sums
    (28,), count, status)."""
    buf = (ProjectiveIter * PROJECTIVE_MAX_ITERATIONS)()
    n = ctx._chk(ctx._lib.icpk_get_sdf_trace(ctx._h, buf, PROJECTIVE_MAX_ITERATIONS))
    return [dict(pose=np.array(buf[k].pose, np.float64).reshape(3, 4), sums=np.array(buf[k].sums, np.float64),
                 count=int(buf[k].count), status=int(buf[k].status)) for k in range(n)]


def sdf_pixels(params, volume, pose, level, tsdf, weight, first=0, count=None, terms=False):
    """icpk_sdf_pixels (host only): the SDF tracking rule for `count` pixels from row-major pixel `first` of the (rows,
    cols) uint16 image `level` (default: all from there on) over the host planes tsdf float32, weight uint16 of `volume`,
    a TsdfParams whose origin is the one to use.  Returns (cell (count,) int32: the cell or the SDF_* code; value
    (count,) float32; terms (count, 28) float64 or None; the number of accepted pixels)."""
    img = np.ascontiguousarray(level, np.uint16)
    rows_s, cols_s = img.shape
    f, w = _f(tsdf).reshape(-1), np.ascontiguousarray(weight, np.uint16).reshape(-1)
    n = volume.dims[0] * volume.dims[1] * volume.dims[2]
    if f.size != n or w.size != n:
        raise ValueError("the planes must hold one entry per voxel")
    count = rows_s * cols_s - int(first) if count is None else int(count)
    m = max(count, 0)
    cell, value = np.zeros(m, np.int32), np.zeros(m, np.float32)
    tm = np.zeros((m, 28), np.float64) if terms else None
    dp, u16 = C.POINTER(C.c_double), C.POINTER(C.c_uint16)
    rc = load().icpk_sdf_pixels(C.byref(params), C.byref(volume), _pose16(pose).ctypes.data_as(dp), img.ctypes.data_as(u16),
                                rows_s, cols_s, _fp(f), w.ctypes.data_as(u16), int(first), count,
                                cell.ctypes.data_as(C.POINTER(C.c_int32)), _fp(value),
                                None if tm is None else tm.ctypes.data_as(dp))
    if rc < 0:
        raise IcpkError(rc, "icpk_sdf_pixels")
    return cell, value, tm, rc


# -- the Euclidean distance map of the volume (K31): the host-only entry points, then the device calls -------------
def esdf_params(max_distance=None, min_weight=None, flags=None):
    """icpk_default_esdf_params, overridden by what is given."""
    p = EsdfParams()
    load().icpk_default_esdf_params(C.byref(p))
    if max_distance is not None:
        p.max_distance = max_distance
    if min_weight is not None:
        p.min_weight = min_weight
    if flags is not None:
        p.flags = flags
    return p


def _esdf(params, kw):
    return params if params is not None else esdf_params(**kw)


def _query_points(points):
    """world points as (3, n) float32: three contiguous planes, as every cloud here is passed"""
    pts = _f(points)
    if pts.ndim != 2 or pts.shape[0] != 3:
        raise ValueError("points: (3, n) expected")
    return pts


def brief_match_params(max_hamming=48, ratio=None, mutual=True, to_clouds=False):
    """icpk_brief_match_params: ratio None (no ratio test) or (num, den)."""
    p = BriefMatchParams()
    load().icpk_default_brief_match_params(C.byref(p))
    p.max_hamming = int(max_hamming)
    p.ratio_num, p.ratio_den = (0, 1) if ratio is None else (int(ratio[0]), int(ratio[1]))
    p.flags = (BRIEF_MUTUAL if mutual else 0) | (BRIEF_TO_CLOUDS if to_clouds else 0)
    return p


def brief_pattern():
    """icpk_brief_pattern: the committed (32, 256, 4) int8 table of THE BRIEF RULE, (ax, ay, bx, by) per bin and test."""
    out = np.zeros((32, 256, 4), np.int8)
    load().icpk_brief_pattern(out.ctypes.data_as(C.POINTER(C.c_int8)))
    return out


def brief_boundaries():
    """icpk_brief_boundaries: the (8, 2) int32 boundary directions (x, y) of the first quadrant."""
    out = np.zeros((8, 2), np.int32)
    load().icpk_brief_boundaries(out.ctypes.data_as(C.POINTER(C.c_int32)))
    return out


def brief_bin(m10, m01):
    """icpk_brief_bin: the orientation bin of a pair of int32 moments."""
    return load().icpk_brief_bin(int(m10), int(m01))


def _image_arg(img):
    img = np.ascontiguousarray(img, np.uint8)
    if img.ndim == 3 and img.shape[2] == 3:
        return img, 3
    if img.ndim == 2:
        return img, 1
    raise ValueError("(rows, cols, 3) BGR or (rows, cols) grey image expected")


def brief_describe_host(img, kp_xy, upright=False):
    """icpk_brief_describe_host (host only): (words (n, 8) uint32, bin (n,) uint8, valid (n,) uint8)."""
    img, ch = _image_arg(img)
    kp = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
    n = len(kp)
    words, b, v = np.zeros((max(n, 1), 8), np.uint32), np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
    u8 = C.POINTER(C.c_uint8)
    rc = load().icpk_brief_describe_host(img.ctypes.data_as(u8), img.shape[0], img.shape[1], ch, _fp(kp), n,
                                         BRIEF_UPRIGHT if upright else 0, words.ctypes.data_as(C.POINTER(C.c_uint32)),
                                         b.ctypes.data_as(u8), v.ctypes.data_as(u8))
    if rc != OK:
        raise IcpkError(rc, "icpk_brief_describe_host")
    return words[:n], b[:n], v[:n]


def brief_match_host(words_s, valid_s, words_t, valid_t, params=None, **kw):
    """icpk_brief_match_host (host only): (src_kp, tgt_kp, H, H2) int32 arrays of the kept pairs, source order."""
    p = params if params is not None else brief_match_params(**kw)
    ws = np.ascontiguousarray(words_s, np.uint32).reshape(-1, 8)
    wt = np.ascontiguousarray(words_t, np.uint32).reshape(-1, 8)
    vs, vt = np.ascontiguousarray(valid_s, np.uint8), np.ascontiguousarray(valid_t, np.uint8)
    out = [np.zeros(max(len(ws), 1), np.int32) for _ in range(4)]
    m = C.c_int32(0)
    ip, u8, u32 = C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    rc = load().icpk_brief_match_host(ws.ctypes.data_as(u32), vs.ctypes.data_as(u8), len(ws), wt.ctypes.data_as(u32),
                                      vt.ctypes.data_as(u8), len(wt), C.byref(p), *[o.ctypes.data_as(ip) for o in out], C.byref(m))
    if rc != OK:
        raise IcpkError(rc, "icpk_brief_match_host")
    return tuple(o[:m.value].copy() for o in out)


def esdf_host(volume, tsdf, weight, params=None, **kw):
    """icpk_esdf_host (host only): THE DISTANCE RULE over host planes of the TsdfParams `volume` (its dims and voxel).
    Returns (sq int32, cls uint8, dist float32, each (dz, dy, dx), counts (4,) int64: unknown, free, occupied, far)."""
    p = _esdf(params, kw)
    n = volume.dims[0] * volume.dims[1] * volume.dims[2]
    f, w = _f(tsdf).reshape(-1), np.ascontiguousarray(weight, np.uint16).reshape(-1)
    if f.size != n or w.size != n:
        raise ValueError("the planes must hold one entry per voxel")
    shape = (volume.dims[2], volume.dims[1], volume.dims[0])
    sq, cls, dist = np.empty(shape, np.int32), np.empty(shape, np.uint8), np.empty(shape, np.float32)
    counts = np.zeros(4, np.int64)
    rc = load().icpk_esdf_host(C.byref(volume), C.byref(p), _fp(f), w.ctypes.data_as(C.POINTER(C.c_uint16)),
                               sq.ctypes.data_as(C.POINTER(C.c_int32)), cls.ctypes.data_as(C.POINTER(C.c_uint8)), _fp(dist),
                               counts.ctypes.data_as(C.POINTER(C.c_int64)))
    if rc != OK:
        raise IcpkError(rc, "icpk_esdf_host")
    return sq, cls, dist, counts


def esdf_query_host(volume, sq, cls, points, params=None, **kw):
    """icpk_esdf_query_host (host only): THE QUERY RULE for the world points (3, n) over host sq and cls planes of the
    TsdfParams `volume` (dims, voxel and the origin to use).  Returns dict(dist (n,), grad (3, n), status (n,) uint8)."""
    p = _esdf(params, kw)
    pts = _query_points(points)
    n = pts.shape[1]
    nvox = volume.dims[0] * volume.dims[1] * volume.dims[2]
    q, c = np.ascontiguousarray(sq, np.int32).reshape(-1), np.ascontiguousarray(cls, np.uint8).reshape(-1)
    if q.size != nvox or c.size != nvox:
        raise ValueError("the planes must hold one entry per voxel")
    dist, grad, status = np.zeros(n, np.float32), np.zeros((3, n), np.float32), np.zeros(n, np.uint8)
    rc = load().icpk_esdf_query_host(C.byref(volume), C.byref(p), q.ctypes.data_as(C.POINTER(C.c_int32)),
                                     c.ctypes.data_as(C.POINTER(C.c_uint8)), _fp(pts[0]), _fp(pts[1]), _fp(pts[2]), n, _fp(dist),
                                     _fp(grad[0]), _fp(grad[1]), _fp(grad[2]), status.ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc != OK:
        raise IcpkError(rc, "icpk_esdf_query_host")
    return dict(dist=dist, grad=grad, status=status)


# ... and the device calls: functions over a Context, like the moving volume's and the signed updates' above
def esdf_compute(ctx, params=None, counts=True, **kw):
    """icpk_esdf_compute: the distance map of the volume as it stands; it stays on the device, a snapshot.  params:
    EsdfParams, or max_distance / min_weight / flags as keywords.  Returns counts (4,) int64 -- unknown, free,
    occupied, far --, or None with counts=False (no host wait)."""
    p = _esdf(params, kw)
    out = np.zeros(4, np.int64)
    ctx._chk(ctx._lib.icpk_esdf_compute(ctx._h, C.byref(p), out.ctypes.data_as(C.POINTER(C.c_int64)) if counts else None))
    return out if counts else None


def esdf_get(ctx, sq=True, cls=True, dist=True):
    """icpk_esdf_get: (sq int32, cls uint8, dist float32) of shape (dz, dy, dx); None where not asked."""
    p = ctx._tsdf
    if p is None:
        ctx._chk(ctx._lib.icpk_esdf_get(ctx._h, None, None, None))  # (ICPK_E_NOT_SET)
    shape = (p.dims[2], p.dims[1], p.dims[0])
    q = np.empty(shape, np.int32) if sq else None
    c = np.empty(shape, np.uint8) if cls else None
    d = np.empty(shape, np.float32) if dist else None
    ctx._chk(ctx._lib.icpk_esdf_get(ctx._h, None if q is None else q.ctypes.data_as(C.POINTER(C.c_int32)),
                                    None if c is None else c.ctypes.data_as(C.POINTER(C.c_uint8)),
                                    None if d is None else _fp(d)))
    return q, c, d


def esdf_get_box(ctx, lo, hi, sq=True, cls=True, dist=True):
    """icpk_esdf_get_box: the same of the sub-box lo <= (x, y, z) < hi, as (hi_z - lo_z, hi_y - lo_y, hi_x - lo_x)
    arrays."""
    lo, hi = _i3(lo, "lo"), _i3(hi, "hi")
    shape = tuple(max(int(hi[a]) - int(lo[a]), 1) for a in (2, 1, 0))  # (an empty box: the call refuses it)
    q = np.empty(shape, np.int32) if sq else None
    c = np.empty(shape, np.uint8) if cls else None
    d = np.empty(shape, np.float32) if dist else None
    i32 = C.POINTER(C.c_int32)
    ctx._chk(ctx._lib.icpk_esdf_get_box(ctx._h, lo.ctypes.data_as(i32), hi.ctypes.data_as(i32),
                                        None if q is None else q.ctypes.data_as(i32),
                                        None if c is None else c.ctypes.data_as(C.POINTER(C.c_uint8)),
                                        None if d is None else _fp(d)))
    return q, c, d


def esdf_query(ctx, points):
    """icpk_esdf_query: THE QUERY RULE for the world points (3, n).  Returns dict(dist (n,), grad (3, n), status
    (n,) uint8: ESDF_Q_OUTSIDE, or ESDF_Q_FAR | ESDF_Q_UNKNOWN of the cell's corners)."""
    pts = _query_points(points)
    n = pts.shape[1]
    dist, grad, status = np.zeros(n, np.float32), np.zeros((3, n), np.float32), np.zeros(n, np.uint8)
    ctx._chk(ctx._lib.icpk_esdf_query(ctx._h, _fp(pts[0]), _fp(pts[1]), _fp(pts[2]), n, _fp(dist), _fp(grad[0]),
                                      _fp(grad[1]), _fp(grad[2]), status.ctypes.data_as(C.POINTER(C.c_uint8))))
    return dict(dist=dist, grad=grad, status=status)


def esdf_release(ctx):
    ctx._chk(ctx._lib.icpk_esdf_release(ctx._h))


class Context:
    """One GPU + one HIP stream (icpk_ctx)."""

    def __init__(self, device=0):
        self._lib = load()
        h = C.c_void_p()
        rc = self._lib.icpk_create(C.byref(h), int(device))
        if rc != OK:
            raise IcpkError(rc, "icpk_create failed (no usable HIP device: there is no CPU fallback)")
        self._h = h
        self._log_ref = None
        self._pinned = {}  # register_host_buffer: address -> the array, alive while the library may read it
        self._tsdf = None    # the TsdfParams of the volume the context holds (tsdf_create) ...
        self._tsdf_n = None  # ... and the length of its surface list (tsdf_extract_surface)
        self._tsdf_ray = None  # ... and the (rows, cols) of its last ray cast (tsdf_raycast)
        self._tsdf_mesh = None  # ... and the three counts of its last mesh (tsdf_extract_mesh)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.icpk_destroy(self._h)
            self._h = None
            self._pinned.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc < 0:
            raise IcpkError(rc, self._lib.icpk_last_error(self._h).decode())
        return rc

    @property
    def stream(self):
        return self._lib.icpk_stream(self._h)

    # -- clouds ---------------------------------------------------------------
    def set_target(self, pts):
        x, y, z = (_f(pts[k]) for k in range(3))
        self._chk(self._lib.icpk_set_target(self._h, _fp(x), _fp(y), _fp(z), x.size))

    def set_source(self, pts):
        x, y, z = (_f(pts[k]) for k in range(3))
        self._chk(self._lib.icpk_set_source(self._h, _fp(x), _fp(y), _fp(z), x.size))

    def set_target_device(self, px, py, pz, n):
        self._chk(self._lib.icpk_set_target_device(self._h, px, py, pz, n))

    def set_source_device(self, px, py, pz, n):
        self._chk(self._lib.icpk_set_source_device(self._h, px, py, pz, n))

    def reset_source(self):
        self._chk(self._lib.icpk_reset_source(self._h))

    def commit_source(self):
        self._chk(self._lib.icpk_commit_source(self._h))

    def get_source(self):
        n = self._lib.icpk_source_size(self._h)
        out = np.empty((3, n), np.float32)
        self._chk(self._lib.icpk_get_source(self._h, _fp(out[0]), _fp(out[1]), _fp(out[2])))
        return out

    def get_target(self):
        n = self._lib.icpk_target_size(self._h)
        out = np.empty((3, n), np.float32)
        self._chk(self._lib.icpk_get_target(self._h, _fp(out[0]), _fp(out[1]), _fp(out[2])))
        return out

    @property
    def source_size(self):
        return self._lib.icpk_source_size(self._h)

    @property
    def target_size(self):
        return self._lib.icpk_target_size(self._h)

    # -- steps ------------------------------------------------------------------
    def nn(self, nn_mode=NN_EXACT, fetch=True):
        n = self.source_size
        if not fetch:
            self._chk(self._lib.icpk_nn(self._h, nn_mode, None, None))
            return None
        idx = np.empty(n, np.int32)
        dist = np.empty(n, np.float32)
        self._chk(self._lib.icpk_nn(self._h, nn_mode, idx.ctypes.data_as(C.POINTER(C.c_int32)), _fp(dist)))
        return idx, dist

    def get_associations(self):
        n = self.source_size
        idx = np.empty(n, np.int32)
        dist = np.empty(n, np.float32)
        self._chk(self._lib.icpk_get_associations(self._h, idx.ctypes.data_as(C.POINTER(C.c_int32)), _fp(dist)))
        return idx, dist

    def reduce(self, max_dist=0.75):
        sums = np.zeros(NSUM, np.float64)
        cnt = C.c_int64(0)
        self._chk(self._lib.icpk_reduce(self._h, max_dist, sums.ctypes.data_as(C.POINTER(C.c_double)), C.byref(cnt)))
        return sums, cnt.value

    def transform_source(self, R, t):
        R = _f(R).reshape(9)
        t = _f(t).reshape(3)
        self._chk(self._lib.icpk_transform_source(self._h, _fp(R), _fp(t)))

    def transform_target(self, R, t):
        R = _f(R).reshape(9)
        t = _f(t).reshape(3)
        self._chk(self._lib.icpk_transform_target(self._h, _fp(R), _fp(t)))

    def get_trace(self, max_iterations=64):
        return self._trace(lambda *a: self._lib.icpk_get_trace(self._h, *a), max_iterations)

    def get_frames_trace(self, job, max_iterations=64):
        """get_trace of job `job` of the last align_frames_batch call."""
        return self._trace(lambda *a: self._lib.icpk_get_frames_trace(self._h, int(job), *a), max_iterations)

    def _trace(self, call, max_iterations):
        n = C.c_int32(0)
        R = np.zeros((max_iterations, 9), np.float32)
        t = np.zeros((max_iterations, 3), np.float32)
        pairs = np.zeros(max_iterations, np.int32)
        mse = np.zeros(max_iterations, np.float32)
        self._chk(call(C.byref(n), _fp(R), _fp(t), pairs.ctypes.data_as(C.POINTER(C.c_int32)), _fp(mse)))
        k = n.value
        return [dict(R=R[i].reshape(3, 3).copy(), t=t[i].copy(), n_pairs=int(pairs[i]), mse=np.float32(mse[i]))
                for i in range(k)]

    def pair_distance(self, a, b, point3=False):
        """point3: the cv::Point3f overload (icp.cpp:595-602) instead of the loop's distance."""
        a = _f(a)
        b = _f(b)
        n = a.shape[1]
        out = np.empty(n, np.float32)
        fn = self._lib.icpk_pair_distance3 if point3 else self._lib.icpk_pair_distance
        self._chk(fn(self._h, _fp(a), _fp(b), _fp(out), n))
        return out

    def register_host_buffer(self, arr):
        """Pins a C-contiguous numpy array for the device (icpk_register_host_buffer): depth images that lie inside it
        are read by icpk_backproject_pair where they are.  The Context holds the array until unregister_host_buffer /
        close."""
        if not arr.flags["C_CONTIGUOUS"]:
            raise ValueError("a C-contiguous array expected")
        self._chk(self._lib.icpk_register_host_buffer(self._h, arr.ctypes.data, arr.nbytes))
        self._pinned[arr.ctypes.data] = arr

    def unregister_host_buffer(self, arr):
        self._chk(self._lib.icpk_unregister_host_buffer(self._h, arr.ctypes.data))
        self._pinned.pop(arr.ctypes.data, None)

    def set_subsample(self, factor=40, seed=0):
        """pointcloud.cpp:27-30 with a reproducible choice: every back-projection keeps one valid pixel in `factor`
        (0 / 1: all); see include/icpk.h.  oracle.subsample_keep gives the same mask."""
        self._chk(self._lib.icpk_set_subsample(self._h, int(factor), int(seed)))

    def backproject(self, depth, which=0, fx=468.60, cx=318.27, offset=None):
        depth = np.ascontiguousarray(depth, np.uint16)
        rows, cols = depth.shape
        off = None if offset is None else _f(offset)
        n = self._chk(self._lib.icpk_backproject(self._h, depth.ctypes.data_as(C.POINTER(C.c_uint16)), rows, cols,
                                                 fx, cx, None if off is None else _fp(off), which))
        return n

    def filter_depth_image(self, depth, max_d=25000, min_d=1000, morph=True, anchor=(-1, -1)):
        """SLAM.cpp:553-574 on the device; anchor = (x, y) of dilate/erode, -1 = element centre."""
        depth = np.ascontiguousarray(depth, np.uint16)
        out = np.empty_like(depth)
        rows, cols = depth.shape
        u16 = C.POINTER(C.c_uint16)
        self._chk(self._lib.icpk_filter_depth_image(self._h, depth.ctypes.data_as(u16), out.ctypes.data_as(u16), rows, cols,
                                                    int(max_d), int(min_d), int(bool(morph)), int(anchor[0]), int(anchor[1])))
        return out

    def backproject_filtered(self, depth, which=0, normals_mode=-1, fx=468.60, cx=318.27, offset=None, max_d=25000,
                             min_d=1000, morph=True, anchor=(-1, -1)):
        depth = np.ascontiguousarray(depth, np.uint16)
        rows, cols = depth.shape
        off = None if offset is None else _f(offset)
        return self._chk(self._lib.icpk_backproject_filtered(
            self._h, depth.ctypes.data_as(C.POINTER(C.c_uint16)), rows, cols, fx, cx, None if off is None else _fp(off),
            which, normals_mode, int(max_d), int(min_d), int(bool(morph)), int(anchor[0]), int(anchor[1])))

    def backproject_pair(self, depth_source, depth_target, R=None, t=None, fx=468.60, cx=318.27, offset=None, filter=False,
                         max_d=25000, min_d=1000, morph=True, anchor=(-1, -1)):
        """icp.cpp:38-71 in one call: both frames back-projected (filtered first if filter), posed by (R, t),
        the posed source committed.  Returns (n_source, n_target)."""
        ds = np.ascontiguousarray(depth_source, np.uint16)
        # depth_target None: the frame this context received as depth_source last time, still on the device (SLAM.cpp:305)
        dt = None if depth_target is None else np.ascontiguousarray(depth_target, np.uint16)
        if ds.ndim != 2 or (dt is not None and ds.shape != dt.shape):
            raise ValueError("two depth images of the same rows x cols shape expected")
        rows, cols = ds.shape
        off = None if offset is None else _f(offset)
        Rm = None if R is None else _f(R)
        tv = None if t is None else _f(t)
        ns, nt = C.c_int32(-1), C.c_int32(-1)
        u16 = C.POINTER(C.c_uint16)
        self._chk(self._lib.icpk_backproject_pair(
            self._h, ds.ctypes.data_as(u16), None if dt is None else dt.ctypes.data_as(u16), rows, cols, fx, cx, None if off is None else _fp(off),
            None if Rm is None else _fp(Rm), None if tv is None else _fp(tv), int(bool(filter)), int(max_d), int(min_d),
            int(bool(morph)), int(anchor[0]), int(anchor[1]), C.byref(ns), C.byref(nt)))
        return ns.value, nt.value

    def align_frames_batch(self, jobs, params=None, fx=468.60, cx=318.27, offset=None, filter=False, max_d=25000,
                           min_d=1000, morph=True, anchor=(-1, -1), **kw):
        """backproject_pair + align for many depth streams in lock step (icpk_align_frames_batch).  jobs: list of dicts
        with stream, source (rows x cols uint16), target (same shape, or None: the stream's resident frame), R, t (the
        camera pose), last_rotation, last_translation.  Returns (T (n, 4, 4), stats list, rc); a job that could not
        run has its status in its stats."""
        p = params if params is not None else default_params(**kw)
        n = len(jobs)
        arr = (FrameJob * max(n, 1))()
        keep = []
        shape = None
        u16 = C.POINTER(C.c_uint16)
        for k, j in enumerate(jobs):
            ds = np.ascontiguousarray(j["source"], np.uint16)
            dt = None if j.get("target") is None else np.ascontiguousarray(j["target"], np.uint16)
            shape = shape or ds.shape
            if ds.ndim != 2 or ds.shape != shape or (dt is not None and dt.shape != shape):
                raise ValueError("depth images of one rows x cols shape expected")
            keep.append((ds, dt))
            arr[k].stream = int(j["stream"])
            arr[k].depth_source = ds.ctypes.data_as(u16)
            arr[k].depth_target = None if dt is None else dt.ctypes.data_as(u16)
            for name, default in (("R", np.eye(3)), ("t", np.zeros(3)), ("last_rotation", np.eye(3)),
                                  ("last_translation", np.zeros(3))):
                v = j.get(name)
                getattr(arr[k], name)[:] = [float(x) for x in _f(default if v is None else v).reshape(-1)]
        rows, cols = shape if shape else (1, 1)
        off = None if offset is None else _f(offset)
        T = np.zeros((max(n, 1), 16), np.float32)
        st = (Stats * max(n, 1))()
        rc = self._lib.icpk_align_frames_batch(
            self._h, n, arr, rows, cols, fx, cx, None if off is None else _fp(off), int(bool(filter)), int(max_d),
            int(min_d), int(bool(morph)), int(anchor[0]), int(anchor[1]), C.byref(p), _fp(T), st)
        return T[:n].reshape(n, 4, 4), list(st)[:n], rc

    def release_frame_streams(self):
        self._chk(self._lib.icpk_release_frame_streams(self._h))

    def associate_keypoints(self, max_dist=MAX_NN_KEYPOINT_DISTANCE, nn_mode=NN_GRID, rejected=None, capacity=None):
        """icp.cpp:488-515 on the context's clouds.  rejected: the caller's running list of rejected
        query indices (None = empty).  Returns (status, assoc_q, assoc_t, assoc_d, rejected) --
        with status W_EMPTY_MAP the other entries are None / the unchanged list."""
        n = self.source_size
        prev = np.asarray([] if rejected is None else rejected, np.int32)
        cap = prev.size + max(n, 1) if capacity is None else int(capacity)
        aq = np.full(max(n, 1), -1, np.int32)
        at = np.full(max(n, 1), -1, np.int32)
        ad = np.full(max(n, 1), np.nan, np.float32)
        rj = np.full(max(cap, 1), -1, np.int32)
        rj[:prev.size] = prev
        na, nr = C.c_int32(-1), C.c_int32(prev.size)
        ip = C.POINTER(C.c_int32)
        rc = self._chk(self._lib.icpk_associate_keypoints(self._h, nn_mode, max_dist, aq.ctypes.data_as(ip), at.ctypes.data_as(ip),
                                                          _fp(ad), C.byref(na), rj.ctypes.data_as(ip), cap, C.byref(nr)))
        if rc == W_EMPTY_MAP:
            assert na.value == -1 and nr.value == prev.size  # untouched
            return rc, None, None, None, prev
        return rc, aq[:na.value].copy(), at[:na.value].copy(), ad[:na.value].copy(), rj[:nr.value].copy()

    # -- point-to-plane extension ------------------------------------------------
    def backproject_with_normals(self, depth, normals_mode=NORMALS_CROSS, fx=468.60, cx=318.27, offset=None):
        depth = np.ascontiguousarray(depth, np.uint16)
        rows, cols = depth.shape
        off = None if offset is None else _f(offset)
        return self._chk(self._lib.icpk_backproject_with_normals(
            self._h, depth.ctypes.data_as(C.POINTER(C.c_uint16)), rows, cols, fx, cx,
            None if off is None else _fp(off), normals_mode))

    def set_target_normals(self, nrm):
        x, y, z = (_f(nrm[k]) for k in range(3))
        self._chk(self._lib.icpk_set_target_normals(self._h, _fp(x), _fp(y), _fp(z), x.size))

    def get_target_normals(self):
        out = np.empty((3, self.target_size), np.float32)
        self._chk(self._lib.icpk_get_target_normals(self._h, _fp(out[0]), _fp(out[1]), _fp(out[2])))
        return out

    def reduce_p2l(self, max_dist=0.75):
        sums = np.zeros(NP2L, np.float64)
        cnt = C.c_int64(0)
        self._chk(self._lib.icpk_reduce_p2l(self._h, max_dist, sums.ctypes.data_as(C.POINTER(C.c_double)), C.byref(cnt)))
        return sums, cnt.value

    # -- robust alignment (icpk_set_robust) -----------------------------------------
    def set_robust(self, kernel=ROBUST_NONE, scale=1.0, scale_mode=SCALE_FIXED, trim=1.0):
        """Weights and trimming of every later alignment (include/icpk.h); set_robust(None) turns it off."""
        if kernel is None:
            return self._chk(self._lib.icpk_set_robust(self._h, None))
        r = Robust(kernel, scale_mode, scale, trim)
        return self._chk(self._lib.icpk_set_robust(self._h, C.byref(r)))

    def get_robust_trace(self, max_iterations=64):
        """Per iteration of the last robust alignment: dict(kept, cut, c, wsum)."""
        n = C.c_int32(0)
        kept = np.zeros(max_iterations, np.int32)
        cut = np.zeros(max_iterations, np.float32)
        c = np.zeros(max_iterations, np.float64)
        w = np.zeros(max_iterations, np.float64)
        dp = C.POINTER(C.c_double)
        self._chk(self._lib.icpk_get_robust_trace(self._h, C.byref(n), kept.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  _fp(cut), c.ctypes.data_as(dp), w.ctypes.data_as(dp)))
        return [dict(kept=int(kept[i]), cut=np.float32(cut[i]), c=float(c[i]), wsum=float(w[i])) for i in range(n.value)]

    def reduce_weighted(self, max_dist=0.75, solve=SOLVE_KABSCH):
        """One robust reduction over the last sweep's associations: (sums, accepted, kept, cut, median, c)."""
        sums = np.zeros(NP2L_W if solve == SOLVE_POINT_TO_PLANE else NSUM_W, np.float64)
        acc, kept = C.c_int64(0), C.c_int64(0)
        cut, med = C.c_float(0), C.c_float(0)
        c = C.c_double(0)
        self._chk(self._lib.icpk_reduce_weighted(self._h, max_dist, solve, sums.ctypes.data_as(C.POINTER(C.c_double)),
                                                 C.byref(acc), C.byref(kept), C.byref(cut), C.byref(med), C.byref(c)))
        return sums, acc.value, kept.value, np.float32(cut.value), np.float32(med.value), c.value

    # -- voxel-grid downsampling (icpk_voxel_downsample) ------------------------------
    def voxel_downsample(self, which=0, leaf=0.05, mode=VOXEL_CENTROID):
        """One point per occupied cube of edge `leaf` (include/icpk.h) in place of the working source (which = 0) or
        the target (1).  Returns (n_out, n_dropped)."""
        n_out, n_drop = C.c_int32(0), C.c_int32(0)
        self._chk(self._lib.icpk_voxel_downsample(self._h, int(which), float(leaf), int(mode), C.byref(n_out),
                                                  C.byref(n_drop)))
        return n_out.value, n_drop.value

    def get_voxel_groups(self):
        """The grouping of the last voxel_downsample: dict(n_in, n_out, first_index (n_out,), count (n_out,),
        out_of_point (n_in,): -1 for a dropped point)."""
        n_in, n_out = C.c_int32(0), C.c_int32(0)
        self._chk(self._lib.icpk_get_voxel_groups(self._h, C.byref(n_in), C.byref(n_out), None, None, None))
        first = np.empty(n_out.value, np.int32)
        count = np.empty(n_out.value, np.int32)
        oop = np.empty(n_in.value, np.int32)
        ip = C.POINTER(C.c_int32)
        self._chk(self._lib.icpk_get_voxel_groups(self._h, None, None, first.ctypes.data_as(ip), count.ctypes.data_as(ip),
                                                  oop.ctypes.data_as(ip)))
        return dict(n_in=n_in.value, n_out=n_out.value, first_index=first, count=count, out_of_point=oop)

    # -- target normals from the target's geometry (icpk_estimate_target_normals) -------
    def estimate_target_normals(self, radius, min_neighbors=5, viewpoint=None, keep_moments=False):
        """Per target point the normal of the plane fitted to its neighbours within `radius`, oriented towards
        `viewpoint` ((3,) or None), installed as the target normals (include/icpk.h).  Stream-ordered: no host wait."""
        v = None if viewpoint is None else _f(viewpoint).reshape(3)
        self._keep_normals_moments = bool(keep_moments)
        self._chk(self._lib.icpk_estimate_target_normals(self._h, float(radius), int(min_neighbors),
                                                         None if v is None else _fp(v),
                                                         NORMALS_KEEP_MOMENTS if keep_moments else 0))

    def get_normal_stats(self):
        """What the last estimate_target_normals found: dict(n, n_valid, count (n,) int32, curvature (n,) float32, and
        moments (n, 10) int64 -- m, S_x S_y S_z, S_xx S_xy S_xz S_yy S_yz S_zz -- if they were kept)."""
        n, nv = C.c_int32(0), C.c_int32(0)
        self._chk(self._lib.icpk_get_normal_stats(self._h, C.byref(n), C.byref(nv), None, None, None))
        count = np.empty(n.value, np.int32)
        curv = np.empty(n.value, np.float32)
        mom = np.empty((n.value, 10), np.int64) if getattr(self, "_keep_normals_moments", False) else None
        self._chk(self._lib.icpk_get_normal_stats(self._h, None, None, count.ctypes.data_as(C.POINTER(C.c_int32)), _fp(curv),
                                                  None if mom is None else mom.ctypes.data_as(C.POINTER(C.c_int64))))
        out = dict(n=n.value, n_valid=nv.value, count=count, curvature=curv)
        if mom is not None:
            out["moments"] = mom
        return out

    # -- outlier removal (icpk_remove_outliers) ----------------------------------------
    def remove_outliers(self, which=0, kind=FILTER_STATISTICAL, k=16, std_ratio=2.0, radius=0.05, min_neighbors=5,
                        stats_only=False):
        """Removes stray points from the working source (which = 0) or the target (1): the statistical filter on the
        mean distance to the k nearest neighbours, or the radius filter on the neighbour count (include/icpk.h).
        stats_only: the cloud stays as it is, only outlier_stats() changes.  Returns (n_out, n_dropped)."""
        f = OutlierFilter(int(kind), int(k), float(std_ratio), float(radius), int(min_neighbors))
        n_out, n_drop = C.c_int32(0), C.c_int32(0)
        self._chk(self._lib.icpk_remove_outliers(self._h, int(which), C.byref(f), FILTER_STATS_ONLY if stats_only else 0,
                                                 C.byref(n_out), C.byref(n_drop)))
        self._filter_kind = int(kind)
        return n_out.value, n_drop.value

    def outlier_stats(self):
        """What the last remove_outliers found: dict(n_in, n_out, value (n_in,) float64 -- the mean k-NN distance or the
        neighbour count --, kth (n_in,) float32 (statistical filter only, else None), out_index (n_in,) int32: -1 for a
        removed or dropped point, summary (4,) float64: N, mu, sigma, T / N, 0, 0, min_neighbors)."""
        n_in, n_out = C.c_int32(0), C.c_int32(0)
        summary = np.zeros(4, np.float64)
        dp = C.POINTER(C.c_double)
        self._chk(self._lib.icpk_get_outlier_stats(self._h, C.byref(n_in), C.byref(n_out), None, None, None,
                                                   summary.ctypes.data_as(dp)))
        value = np.zeros(n_in.value, np.float64)
        kth = np.zeros(n_in.value, np.float32)
        oidx = np.empty(n_in.value, np.int32)
        self._chk(self._lib.icpk_get_outlier_stats(self._h, None, None, value.ctypes.data_as(dp), _fp(kth),
                                                   oidx.ctypes.data_as(C.POINTER(C.c_int32)), None))
        statistical = getattr(self, "_filter_kind", FILTER_STATISTICAL) == FILTER_STATISTICAL
        return dict(n_in=n_in.value, n_out=n_out.value, value=value, kth=kth if statistical else None, out_index=oidx,
                    summary=summary)

    # -- plane-to-plane flavour (SOLVE_PLANE_TO_PLANE; include/icpk.h) ------------------
    def estimate_source_normals(self, radius, min_neighbors=5, viewpoint=None):
        """estimate_target_normals' rule applied to the uploaded source; the result stays with the source until it is
        replaced.  Stream-ordered: no host wait."""
        v = None if viewpoint is None else _f(viewpoint).reshape(3)
        self._chk(self._lib.icpk_estimate_source_normals(self._h, float(radius), int(min_neighbors),
                                                         None if v is None else _fp(v), 0))

    def set_source_normals(self, nrm):
        x, y, z = (_f(nrm[k]) for k in range(3))
        self._chk(self._lib.icpk_set_source_normals(self._h, _fp(x), _fp(y), _fp(z), x.size))

    def get_source_normals(self):
        out = np.empty((3, self.source_size), np.float32)
        self._chk(self._lib.icpk_get_source_normals(self._h, _fp(out[0]), _fp(out[1]), _fp(out[2])))
        return out

    def set_plane_to_plane(self, epsilon=1e-3):
        """epsilon of the surface model C(n) = I - (1 - epsilon) n n^T, finite and in (0, 1]."""
        return self._chk(self._lib.icpk_set_plane_to_plane(self._h, float(epsilon)))

    def reduce_plane_to_plane(self, max_dist=0.75, R_acc=None):
        """The 28 sums of the plane-to-plane step over the last sweep's associations and the accepted count; R_acc:
        the rotation accumulated so far ((3, 3), default the identity)."""
        sums = np.zeros(NP2L, np.float64)
        cnt = C.c_int64(0)
        R = None if R_acc is None else _f(np.asarray(R_acc, np.float32).reshape(9))
        self._chk(self._lib.icpk_reduce_plane_to_plane(self._h, max_dist, None if R is None else _fp(R),
                                                       sums.ctypes.data_as(C.POINTER(C.c_double)), C.byref(cnt)))
        return sums, cnt.value

    # -- colored ICP (icpk_set_colored; include/icpk.h) ---------------------------------
    def set_target_colors(self, intensity):
        """One intensity in [0, 1] per target point ((n,) float32)."""
        v = _f(intensity).reshape(-1)
        self._chk(self._lib.icpk_set_target_colors(self._h, _fp(v), v.size))

    def set_source_colors(self, intensity):
        """One intensity in [0, 1] per point of the uploaded source, in its order; they stay with it until it is
        replaced."""
        v = _f(intensity).reshape(-1)
        self._chk(self._lib.icpk_set_source_colors(self._h, _fp(v), v.size))

    def get_target_colors(self):
        out = np.empty(self.target_size, np.float32)
        self._chk(self._lib.icpk_get_target_colors(self._h, _fp(out)))
        return out

    def get_source_colors(self):
        out = np.empty(self.source_size, np.float32)
        self._chk(self._lib.icpk_get_source_colors(self._h, _fp(out)))
        return out

    def estimate_target_color_gradients(self, radius, min_neighbors=4, keep_sums=False):
        """Per target point the gradient of the intensity over its tangent plane, fitted to the neighbours within
        `radius` (needs target normals and colours).  min_neighbors must be at least 1 (E_ARG otherwise); a point with
        fewer neighbours gets the zero gradient.  Stream-ordered: no host wait."""
        self._chk(self._lib.icpk_estimate_target_color_gradients(self._h, float(radius), int(min_neighbors),
                                                                 COLOR_KEEP_SUMS if keep_sums else 0))

    def get_target_color_gradients(self):
        out = np.empty((3, self.target_size), np.float32)
        self._chk(self._lib.icpk_get_target_color_gradients(self._h, _fp(out[0]), _fp(out[1]), _fp(out[2])))
        return out

    def color_gradient_sums(self):
        """(n, 10) int64 -- m, S_00 S_01 S_02 S_11 S_12 S_22, T_0 T_1 T_2 -- of the last estimate (keep_sums=True)."""
        out = np.empty((self.target_size, 10), np.int64)
        self._chk(self._lib.icpk_get_color_gradient_sums(self._h, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out

    def set_colored(self, on=True, lambda_geometric=0.968):
        """While on, SOLVE_POINT_TO_PLANE alignments run the joint geometric + photometric step; lambda_geometric in
        [0, 1] weighs the geometric part."""
        return self._chk(self._lib.icpk_set_colored(self._h, 1 if on else 0, float(lambda_geometric)))

    def reduce_colored(self, max_dist=0.75):
        """The 28 sums of the joint step over the last sweep's associations and the accepted count."""
        sums = np.zeros(NP2L, np.float64)
        cnt = C.c_int64(0)
        self._chk(self._lib.icpk_reduce_colored(self._h, max_dist, sums.ctypes.data_as(C.POINTER(C.c_double)),
                                                C.byref(cnt)))
        return sums, cnt.value

    # -- pose scoring (icpk_score_poses) -----------------------------------------------
    def score_poses(self, T=None, max_dist=0.75, keep_assoc=False):
        """Scores candidate poses of the uploaded source against the target (include/icpk.h): T (n, 4, 4) or (4, 4)
        float32 row-major, or None for the working source as it stands (after align: the alignment just computed).
        The context's state is not touched.  Returns dict(sums (n, 11) float64, inliers (n,) int64, fitness,
        inlier_rmse, mean_dist (n,) float32, information (n, 6, 6) float64)."""
        if T is None:
            n, Tp = 1, None
        else:
            Tf = _f(T).reshape(-1, 16)
            n, Tp = Tf.shape[0], _fp(Tf)
        sums = np.zeros((max(n, 1), NSCORE), np.float64)
        inl = np.zeros(max(n, 1), np.int64)
        self._chk(self._lib.icpk_score_poses(self._h, n, Tp, float(max_dist), SCORE_KEEP_ASSOC if keep_assoc else 0,
                                             sums.ctypes.data_as(C.POINTER(C.c_double)),
                                             inl.ctypes.data_as(C.POINTER(C.c_int64))))
        ns = self.source_size
        met = np.array([score_metrics(sums[k], inl[k], ns) for k in range(n)], np.float32).reshape(n, 3)
        info = np.stack([information_matrix(sums[k], inl[k]) for k in range(n)]) if n else np.zeros((0, 6, 6))
        return dict(sums=sums[:n], inliers=inl[:n], fitness=met[:, 0].copy(), inlier_rmse=met[:, 1].copy(),
                    mean_dist=met[:, 2].copy(), information=info)

    def score_associations(self, pose=0):
        """(index (ns,) int32, distance (ns,) float32) of pose `pose` of the last score_poses(keep_assoc=True): -1 and
        +inf for a point without a partner within max_dist."""
        n = self.source_size
        idx = np.empty(n, np.int32)
        dist = np.empty(n, np.float32)
        self._chk(self._lib.icpk_get_score_associations(self._h, int(pose), idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                                        _fp(dist)))
        return idx, dist

    # -- global registration (icpk_compute_fpfh / icpk_match_features / icpk_register_global) ----
    def compute_fpfh(self, which, radius, keep_spfh=False):
        """FPFH descriptors of the uploaded source (which = 0, needs source normals) or the target (which = 1, needs
        target normals) over the neighbours within `radius` (include/icpk.h, K16).  Stream-ordered: no host wait."""
        return self._chk(self._lib.icpk_compute_fpfh(self._h, int(which), float(radius), FPFH_KEEP_SPFH if keep_spfh else 0))

    def get_fpfh(self, which):
        """(desc (n, 33) float32 in the caller's point order, valid (n,) bool)"""
        n = self.source_size if which == 0 else self.target_size
        desc = np.zeros((max(n, 1), FPFH_BINS), np.float32)
        valid = np.zeros(max(n, 1), np.uint8)
        m = C.c_int32(0)
        self._chk(self._lib.icpk_get_fpfh(self._h, int(which), _fp(desc), valid.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(m)))
        return desc[:m.value], valid[:m.value].astype(bool)

    def get_spfh(self, which):
        """(counts (n, 33) int32, m (n,) int32) of the last compute_fpfh(which, keep_spfh=True)"""
        n = self.source_size if which == 0 else self.target_size
        counts = np.zeros((max(n, 1), FPFH_BINS), np.int32)
        m = np.zeros(max(n, 1), np.int32)
        ip = C.POINTER(C.c_int32)
        self._chk(self._lib.icpk_get_spfh(self._h, int(which), counts.ctypes.data_as(ip), m.ctypes.data_as(ip)))
        return counts[:n], m[:n]

    def match_features(self, mutual=False):
        """Pairs every valid source descriptor with its nearest valid target descriptor (ties: the lowest index);
        mutual: only pairs that are each other's best.  Returns (src_index, tgt_index int32, D float32), source order;
        the pairs stay on the device for register_global."""
        self._chk(self._lib.icpk_match_features(self._h, MATCH_MUTUAL if mutual else 0))
        n = max(self.source_size, 1)
        si, ti, D = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        m = C.c_int32(0)
        ip = C.POINTER(C.c_int32)
        self._chk(self._lib.icpk_get_feature_matches(self._h, si.ctypes.data_as(ip), ti.ctypes.data_as(ip), _fp(D), C.byref(m)))
        return si[:m.value].copy(), ti[:m.value].copy(), D[:m.value].copy()

    def register_global(self, n_hypotheses=4096, seed=0, max_dist=0.75, edge_similarity=0.9):
        """Seeded RANSAC over the matches of match_features, ranked by score_poses' path (include/icpk.h, K16).
        Returns (dict(T (4, 4) float32, hypothesis, inliers, sums (11,) float64, n_valid, n_matches), rc); rc is
        W_TOO_FEW_PAIRS (T the identity) with fewer than 3 matches or no valid hypothesis."""
        p = GlobalParams()
        self._lib.icpk_default_global_params(C.byref(p))
        p.n_hypotheses, p.seed, p.max_dist, p.edge_similarity = int(n_hypotheses), int(seed), float(max_dist), float(edge_similarity)
        r = GlobalResult()
        rc = self._chk(self._lib.icpk_register_global(self._h, C.byref(p), C.byref(r)))
        return dict(T=np.array(r.T, np.float32).reshape(4, 4), hypothesis=r.hypothesis, inliers=int(r.inliers),
                    sums=np.array(r.sums, np.float64), n_valid=r.n_valid, n_matches=r.n_matches), rc

    # -- loop ---------------------------------------------------------------------
    def pose_graph_optimize(self, poses, edges, params=None, **kw):
        """icpk_pose_graph_optimize (K18).  poses (n, 4, 4) float64, edges a sequence of (source, target, T, info,
        uncertain); params a PgParams or its fields as keywords.  Returns (poses (n, 4, 4), result PgResult, weights
        (m,), chi2 (m,), pruned (m,) bool, status OK or W_NOT_CONVERGED)."""
        dp = C.POINTER(C.c_double)
        p = params if params is not None else default_pg_params(**kw)
        P = np.array(poses, np.float64, order="C").reshape(-1, 4, 4)
        m = len(edges)
        res = PgResult()
        w, chi2, pruned = np.zeros(max(m, 1)), np.zeros(max(m, 1)), np.zeros(max(m, 1), np.uint8)
        rc = self._chk(self._lib.icpk_pose_graph_optimize(self._h, P.shape[0], P.ctypes.data_as(dp), m, pg_edges(edges),
                                                          C.byref(p), C.byref(res), w.ctypes.data_as(dp),
                                                          chi2.ctypes.data_as(dp),
                                                          pruned.ctypes.data_as(C.POINTER(C.c_uint8))))
        return P, res, w[:m], chi2[:m], pruned[:m].astype(bool), rc

    def pose_graph_evaluate(self, poses, edges, mu=0.0):
        """icpk_pose_graph_evaluate: (chi2 (m,), weights (m,), cost, gradient (n, 6)) at the given poses; nothing moves."""
        dp = C.POINTER(C.c_double)
        P = np.ascontiguousarray(poses, np.float64).reshape(-1, 4, 4)
        m = len(edges)
        chi2, w, g = np.zeros(max(m, 1)), np.zeros(max(m, 1)), np.zeros((P.shape[0], 6))
        cost = C.c_double(0)
        self._chk(self._lib.icpk_pose_graph_evaluate(self._h, P.shape[0], P.ctypes.data_as(dp), m, pg_edges(edges),
                                                     float(mu), chi2.ctypes.data_as(dp), w.ctypes.data_as(dp),
                                                     C.byref(cost), g.ctypes.data_as(dp)))
        return chi2[:m], w[:m], cost.value, g

    def get_pose_graph_trace(self):
        """Per LM iteration of the last pose_graph_optimize: dict(cost, lam, pcg_iterations, accepted)."""
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        n = C.c_int32(0)
        self._chk(self._lib.icpk_get_pose_graph_trace(self._h, C.byref(n), None, None, None, None))
        k = max(n.value, 1)
        cost, lam, pcg, acc = np.zeros(k), np.zeros(k), np.zeros(k, np.int32), np.zeros(k, np.int32)
        self._chk(self._lib.icpk_get_pose_graph_trace(self._h, C.byref(n), cost.ctypes.data_as(dp), lam.ctypes.data_as(dp),
                                                      pcg.ctypes.data_as(ip), acc.ctypes.data_as(ip)))
        return [dict(cost=float(cost[i]), lam=float(lam[i]), pcg_iterations=int(pcg[i]), accepted=bool(acc[i]))
                for i in range(n.value)]

    # -- TSDF volume (K19) ---------------------------------------------------------
    def tsdf_create(self, params=None, **kw):
        """icpk_tsdf_create: the context's TSDF volume (replaces the one it held).  params: TsdfParams, or the fields
        of tsdf_params as keywords.  Returns the TsdfParams in force."""
        p = params if params is not None else tsdf_params(**kw)
        self._chk(self._lib.icpk_tsdf_create(self._h, C.byref(p)))
        self._tsdf, self._tsdf_n, self._tsdf_ray, self._tsdf_mesh = p, None, None, None
        return p

    def tsdf_reset(self):
        self._chk(self._lib.icpk_tsdf_reset(self._h))
        self._tsdf_n = self._tsdf_ray = self._tsdf_mesh = None

    def tsdf_release(self):
        self._chk(self._lib.icpk_tsdf_release(self._h))
        self._tsdf, self._tsdf_n, self._tsdf_ray, self._tsdf_mesh = None, None, None, None

    def tsdf_integrate(self, depth, pose, intensity=None, fx=468.60, cx=318.27, shape=None, count=True):
        """icpk_tsdf_integrate: one frame into the volume.  depth (rows, cols) uint16, or None: the frame
        backproject_pair left resident (shape = (rows, cols) then).  pose (4, 4) float64, camera-to-world.  intensity
        (rows, cols) float32 on a TSDF_COLOR volume.  Returns the number of voxels written (None with count=False)."""
        d = None if depth is None else np.ascontiguousarray(depth, np.uint16)
        rows, cols = d.shape if d is not None else shape
        P = np.ascontiguousarray(pose, np.float64).reshape(16)
        img = None if intensity is None else _f(intensity).reshape(-1)
        if img is not None and img.size != rows * cols:
            raise ValueError("one intensity per pixel expected")
        n = C.c_int32(-1)
        self._chk(self._lib.icpk_tsdf_integrate(self._h, None if d is None else d.ctypes.data_as(C.POINTER(C.c_uint16)),
                                                None if img is None else _fp(img), rows, cols, fx, cx,
                                                P.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n) if count else None))
        return n.value if count else None

    def tsdf_get(self, tsdf=True, weight=True, intensity=False):
        """icpk_tsdf_get: (tsdf float32, weight uint16, intensity float32) of shape (dz, dy, dx); None where not asked."""
        p = self._tsdf
        if p is None:
            self._chk(self._lib.icpk_tsdf_get(self._h, None, None, None))  # (ICPK_E_NOT_SET)
        shape = (p.dims[2], p.dims[1], p.dims[0])
        f = np.empty(shape, np.float32) if tsdf else None
        w = np.empty(shape, np.uint16) if weight else None
        c = np.empty(shape, np.float32) if intensity else None
        self._chk(self._lib.icpk_tsdf_get(self._h, None if f is None else _fp(f),
                                          None if w is None else w.ctypes.data_as(C.POINTER(C.c_uint16)),
                                          None if c is None else _fp(c)))
        return f, w, c

    def tsdf_set(self, tsdf, weight, intensity=None):
        """icpk_tsdf_set: the planes from arrays of one entry per voxel ((dz, dy, dx), or flat): tsdf float32 in
        [-1, 1], weight uint16, intensity float32 in [0, 1] on a TSDF_COLOR volume.  Drops the surface list, the ray-cast
        maps and the mesh."""
        p = self._tsdf
        if p is None:
            self._chk(self._lib.icpk_tsdf_set(self._h, None, None, None))  # (ICPK_E_NOT_SET)
        n = p.dims[0] * p.dims[1] * p.dims[2]
        f, w = _f(tsdf).reshape(-1), np.ascontiguousarray(weight, np.uint16).reshape(-1)
        c = None if intensity is None else _f(intensity).reshape(-1)
        if f.size != n or w.size != n or (c is not None and c.size != n):
            raise ValueError("the planes must hold one entry per voxel")
        self._chk(self._lib.icpk_tsdf_set(self._h, _fp(f), w.ctypes.data_as(C.POINTER(C.c_uint16)),
                                          None if c is None else _fp(c)))
        self._tsdf_n = self._tsdf_ray = self._tsdf_mesh = None

    def tsdf_extract_mesh(self, min_weight=1):
        """icpk_tsdf_extract_mesh: (n_vertices, n_triangles, n_no_normal); the mesh stays on the device."""
        nv, nt, nn = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
        self._chk(self._lib.icpk_tsdf_extract_mesh(self._h, int(min_weight), C.byref(nv), C.byref(nt), C.byref(nn)))
        self._tsdf_mesh = (nv.value, nt.value, nn.value)
        return self._tsdf_mesh

    def tsdf_get_mesh(self):
        """icpk_tsdf_get_mesh: dict(vertices (3, n), normals (3, n), intensity (n,), voxel_index (n,) int32, edge (n,)
        uint8, triangles (m, 3) int32, n_vertices, n_triangles, n_no_normal) of the last mesh extraction."""
        if self._tsdf_mesh is None:
            self._chk(self._lib.icpk_tsdf_get_mesh(self._h, *([None] * 10)))  # (ICPK_E_NOT_SET)
            raise IcpkError(E_NOT_SET, "no mesh (tsdf_extract_mesh)")
        n, m, nn = self._tsdf_mesh
        pts, nrm = np.zeros((3, max(n, 1)), np.float32), np.zeros((3, max(n, 1)), np.float32)
        inten, vox, edge = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint8)
        tri = np.zeros((max(m, 1), 3), np.int32)
        i32 = C.POINTER(C.c_int32)
        self._chk(self._lib.icpk_tsdf_get_mesh(self._h, _fp(pts[0]), _fp(pts[1]), _fp(pts[2]), _fp(nrm[0]), _fp(nrm[1]),
                                               _fp(nrm[2]), _fp(inten), vox.ctypes.data_as(i32),
                                               edge.ctypes.data_as(C.POINTER(C.c_uint8)), tri.ctypes.data_as(i32)))
        return dict(vertices=pts[:, :n], normals=nrm[:, :n], intensity=inten[:n], voxel_index=vox[:n], edge=edge[:n],
                    triangles=tri[:m], n_vertices=n, n_triangles=m, n_no_normal=nn)

    def tsdf_extract_surface(self, min_weight=1):
        """icpk_tsdf_extract_surface: (n_points, n_no_normal); the list stays on the device."""
        n, m = C.c_int32(-1), C.c_int32(-1)
        self._chk(self._lib.icpk_tsdf_extract_surface(self._h, int(min_weight), C.byref(n), C.byref(m)))
        self._tsdf_n = n.value
        return n.value, m.value

    def tsdf_get_surface(self):
        """icpk_tsdf_get_surface: dict(points (3, n), normals (3, n), intensity (n,), voxel (n,) int32, axis (n,) uint8)
        of the last extraction."""
        n = self._tsdf_n
        if n is None:
            self._chk(self._lib.icpk_tsdf_get_surface(self._h, *([None] * 9)))  # (ICPK_E_NOT_SET)
            n = 0
        m = max(n, 1)
        pts, nrm = np.zeros((3, m), np.float32), np.zeros((3, m), np.float32)
        inten, vox, axis = np.zeros(m, np.float32), np.zeros(m, np.int32), np.zeros(m, np.uint8)
        self._chk(self._lib.icpk_tsdf_get_surface(self._h, _fp(pts[0]), _fp(pts[1]), _fp(pts[2]), _fp(nrm[0]), _fp(nrm[1]),
                                                  _fp(nrm[2]), _fp(inten), vox.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  axis.ctypes.data_as(C.POINTER(C.c_uint8))))
        return dict(points=pts[:, :n], normals=nrm[:, :n], intensity=inten[:n], voxel=vox[:n], axis=axis[:n])

    def tsdf_surface_to_target(self):
        self._chk(self._lib.icpk_tsdf_surface_to_target(self._h))

    # -- ray cast of the TSDF volume (K20) -------------------------------------------
    def tsdf_raycast(self, pose, params=None, count=True, **kw):
        """icpk_tsdf_raycast: the volume seen from the camera-to-world pose (4, 4) float64, as maps that stay on the
        device.  params: TsdfRaycastParams, or the fields of tsdf_raycast_params as keywords.  Returns (n_hits,
        n_no_normal), or None with count=False (the call does not wait then)."""
        p = params if params is not None else tsdf_raycast_params(**kw)
        P = np.ascontiguousarray(pose, np.float64).reshape(16)
        n, m = C.c_int32(-1), C.c_int32(-1)
        self._chk(self._lib.icpk_tsdf_raycast(self._h, C.byref(p), P.ctypes.data_as(C.POINTER(C.c_double)),
                                              C.byref(n) if count else None, C.byref(m) if count else None))
        self._tsdf_ray = (p.rows, p.cols)
        return (n.value, m.value) if count else None

    def tsdf_get_raycast(self):
        """icpk_tsdf_get_raycast: dict(points (3, rows, cols), normals (3, rows, cols), depth (rows, cols), intensity
        (rows, cols)) of the last ray cast; a pixel without a hit holds 0 everywhere.  Without TSDF_COLOR the
        intensity is not asked for and comes back 0."""
        if self._tsdf_ray is None:
            self._chk(self._lib.icpk_tsdf_get_raycast(self._h, *([None] * 8)))  # (ICPK_E_NOT_SET)
            raise IcpkError(E_NOT_SET, "no ray cast (tsdf_raycast)")
        rows, cols = self._tsdf_ray
        maps = np.zeros((8, rows, cols), np.float32)
        color = self._tsdf is not None and (self._tsdf.flags & TSDF_COLOR)
        self._chk(self._lib.icpk_tsdf_get_raycast(self._h, *[_fp(maps[k]) for k in range(7)], _fp(maps[7]) if color else None))
        return dict(points=maps[0:3], normals=maps[3:6], depth=maps[6], intensity=maps[7])

    def tsdf_raycast_to_target(self):
        self._chk(self._lib.icpk_tsdf_raycast_to_target(self._h))

    def align(self, params=None, **kw):
        p = params if params is not None else default_params(**kw)
        T = np.zeros(16, np.float32)
        st = Stats()
        rc = self._chk(self._lib.icpk_align(self._h, C.byref(p), _fp(T), C.byref(st)))
        return T.reshape(4, 4), st, rc

    # -- voxel certainty map (map.hpp / map.cpp) --------------------------------
    def map_reset(self):
        self._chk(self._lib.icpk_map_reset(self._h))

    def map_release(self):
        self._chk(self._lib.icpk_map_release(self._h))

    def map_update(self, rule, delta, from_=MAP_FROM_SOURCE, indices=None):
        """rule ICPK_MAP_ADD_* over the context's source / target (indices: list applied in order, None: all)."""
        if indices is None:
            return self._chk(self._lib.icpk_map_update(self._h, rule, from_, None, 0, delta))
        idx = np.ascontiguousarray(indices, np.int32).reshape(-1)
        return self._chk(self._lib.icpk_map_update(self._h, rule, from_, idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                                   idx.size, delta))

    def map_update_points(self, rule, pts, delta):
        x, y, z = (_f(pts[k]) for k in range(3))
        return self._chk(self._lib.icpk_map_update_points(self._h, rule, _fp(x), _fp(y), _fp(z), x.size, delta))

    def map_set_points(self, from_=MAP_FROM_TARGET):
        self._chk(self._lib.icpk_map_set_points(self._h, from_))

    def map_size(self, lst):
        return self._chk(self._lib.icpk_map_size(self._h, lst))

    def map_get_list(self, lst):
        n = self.map_size(lst)
        out = np.empty((3, n), np.float32)
        self._chk(self._lib.icpk_map_get_list(self._h, lst, _fp(out[0]), _fp(out[1]), _fp(out[2])))
        return out

    def map_get_certainty(self):
        """the whole grid, (300, 300, 300) uint8 indexed [x, y, z]"""
        out = np.empty(MAP_CELLS, np.uint8)
        self._chk(self._lib.icpk_map_get_certainty(self._h, out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out.reshape(MAP_HEIGHT, MAP_HEIGHT, MAP_HEIGHT)

    def map_query(self, pts):
        """per point: (certainty uint8, occupied uint8, slot list int32, slot index int32); -1, -1 = empty slot"""
        x, y, z = (_f(pts[k]) for k in range(3))
        n = x.size
        cert = np.zeros(n, np.uint8)
        occ = np.zeros(n, np.uint8)
        sl = np.zeros(n, np.int32)
        si = np.zeros(n, np.int32)
        u8 = C.POINTER(C.c_uint8)
        ip = C.POINTER(C.c_int32)
        self._chk(self._lib.icpk_map_query(self._h, _fp(x), _fp(y), _fp(z), n, cert.ctypes.data_as(u8),
                                           occ.ctypes.data_as(u8), sl.ctypes.data_as(ip), si.ctypes.data_as(ip)))
        return cert, occ, sl, si

    def map_list_to_target(self, lst):
        self._chk(self._lib.icpk_map_list_to_target(self._h, lst))

    def align_to_map(self, params=None, delta=MAP_DELTA_CONFIDENCE, **kw):
        """icp.cpp:98-271 against the map: the context's source vs the map's key points (the context's target is
        replaced), then the rejected key points of every sweep through ADD_UNASSOCIATED.  Returns (T, stats, rc)."""
        p = params if params is not None else default_params(**kw)
        T = np.zeros(16, np.float32)
        st = Stats()
        rc = self._chk(self._lib.icpk_align_to_map(self._h, C.byref(p), delta, _fp(T), C.byref(st)))
        return T.reshape(4, 4), st, rc

    def map_nearest(self, pts):
        """getNearestMappedPoint (icp.cpp:371-473, K9) per point: (dist float32, list int32, index int32); list is
        MAP_KEYPOINTS / MAP_POINTS, MAP_NN_EMPTY (the zero point of an empty voxel won) or MAP_NN_NONE (dist 0.75)."""
        x, y, z = (_f(pts[k]) for k in range(3))
        n = x.size
        d = np.zeros(n, np.float32)
        lst = np.zeros(n, np.int32)
        idx = np.zeros(n, np.int32)
        ip = C.POINTER(C.c_int32)
        self._chk(self._lib.icpk_map_nearest(self._h, _fp(x), _fp(y), _fp(z), n, _fp(d), lst.ctypes.data_as(ip),
                                             idx.ctypes.data_as(ip)))
        return d, lst, idx

    def map_lookup_to_target(self):
        """the target becomes [key points | points | (0, 0, 0)]: what NN_MAP sweeps index"""
        self._chk(self._lib.icpk_map_lookup_to_target(self._h))

    def align_to_map_dense(self, params=None, delta=MAP_DELTA_CONFIDENCE, **kw):
        """icp.cpp:155-257 with the mapped association: the context's source vs the map's lookup target (the context's
        target is replaced), then (delta > 0) the last sweep's accepted points through ADD_ASSOCIATED.
        Returns (T, stats, rc)."""
        p = params if params is not None else default_params(**kw)
        T = np.zeros(16, np.float32)
        st = Stats()
        rc = self._chk(self._lib.icpk_align_to_map_dense(self._h, C.byref(p), delta, _fp(T), C.byref(st)))
        return T.reshape(4, 4), st, rc

    # -- FAST key points (SLAM.cpp:255-256) and their back-projection (pointcloud.cpp:60-98) ------------------------
    def bgr_to_gray(self, bgr):
        """cv::cvtColor(CV_BGR2GRAY) on the device: (rows, cols, 3) uint8 BGR -> (rows, cols) uint8"""
        bgr = np.ascontiguousarray(bgr, np.uint8)
        if bgr.ndim != 3 or bgr.shape[2] != 3:
            raise ValueError("(rows, cols, 3) BGR image expected")
        out = np.empty(bgr.shape[:2], np.uint8)
        u8 = C.POINTER(C.c_uint8)
        self._chk(self._lib.icpk_bgr_to_gray(self._h, bgr.ctypes.data_as(u8), bgr.shape[0], bgr.shape[1],
                                             out.ctypes.data_as(u8)))
        return out

    def detect_fast(self, img, threshold=60, nonmax=True, type=FAST_TYPE_7_12, capacity=None):
        """cv::FAST on a (rows, cols, 3) BGR or (rows, cols) grey uint8 image.  The key points also stay on the device
        (input of detected_to_cloud).  Returns (kp_xy (n, 2) float32, response (n,) float32), at most `capacity`
        entries (None: all of them)."""
        img = np.ascontiguousarray(img, np.uint8)
        if img.ndim == 3 and img.shape[2] == 3:
            ch = 3
        elif img.ndim == 2:
            ch = 1
        else:
            raise ValueError("(rows, cols, 3) BGR or (rows, cols) grey image expected")
        rows, cols = img.shape[:2]
        u8, ip = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
        n = C.c_int32(0)
        if capacity is None:  # count first, then fetch exactly that many (the list is on the device either way)
            self._chk(self._lib.icpk_detect_fast(self._h, img.ctypes.data_as(u8), rows, cols, ch, int(threshold),
                                                 int(bool(nonmax)), int(type), 0, None, None, C.byref(n)))
            capacity = n.value
        kp = np.zeros((max(int(capacity), 1), 2), np.float32)
        resp = np.zeros(max(int(capacity), 1), np.float32)
        self._chk(self._lib.icpk_detect_fast(self._h, img.ctypes.data_as(u8), rows, cols, ch, int(threshold),
                                             int(bool(nonmax)), int(type), int(capacity), _fp(kp), _fp(resp), C.byref(n)))
        m = min(n.value, int(capacity))
        self.detected_count = n.value
        return kp[:m].copy(), resp[:m].copy()

    def detected_to_cloud(self, depth, R=None, t=None, which=0, fx=468.60, cx=318.27):
        """the detected key points back-projected from `depth` (pointcloud.cpp:60-98), posed by p <- fl32(fl32(R p) + t)
        (None: identity / zero) and made the context's source (which 0) or target (1).  Returns the point count."""
        depth = np.ascontiguousarray(depth, np.uint16)
        Rm = _f(np.eye(3) if R is None else R).reshape(9)
        tv = _f(np.zeros(3) if t is None else t).reshape(3)
        n = C.c_int32(0)
        self._chk(self._lib.icpk_detected_to_cloud(self._h, depth.ctypes.data_as(C.POINTER(C.c_uint16)), depth.shape[0],
                                                   depth.shape[1], fx, cx, _fp(Rm), _fp(tv), int(which), C.byref(n)))
        return n.value

    def align_query_sharded(self, params=None, **kw):
        """One pair, queries sharded over the communicator's ranks (collective call): this context's source is the
        rank's slice, the target is the same everywhere; one in-stream all-reduce of 20 doubles per iteration, no host
        round trip.  Returns (T, stats, rc), identical on every rank."""
        p = params if params is not None else default_params(**kw)
        T = np.zeros(16, np.float32)
        st = Stats()
        rc = self._chk(self._lib.icpk_align_query_sharded(self._h, C.byref(p), _fp(T), C.byref(st)))
        return T.reshape(4, 4), st, rc

    def align_batch(self, pairs, params=None, associations=False, **kw):
        """pairs: list of (source (3,Ns), target (3,Nt)) host arrays.  Returns (T (n,4,4), stats list,
        rc) and, with associations=True, additionally a list of (idx, dist) per pair."""
        p = params if params is not None else default_params(**kw)
        n = len(pairs)
        arr = (Pair * max(n, 1))()
        keep = []
        assoc = []
        for b, (s, t) in enumerate(pairs):
            sx, sy, sz = (_f(s[k]) for k in range(3))
            tx, ty, tz = (_f(t[k]) for k in range(3))
            keep.append((sx, sy, sz, tx, ty, tz))
            arr[b].sx, arr[b].sy, arr[b].sz, arr[b].ns = _fp(sx), _fp(sy), _fp(sz), sx.size
            arr[b].tx, arr[b].ty, arr[b].tz, arr[b].nt = _fp(tx), _fp(ty), _fp(tz), tx.size
            if associations:
                idx = np.full(sx.size, -1, np.int32)
                dist = np.full(sx.size, np.nan, np.float32)
                assoc.append((idx, dist))
                arr[b].idx_out = idx.ctypes.data_as(C.POINTER(C.c_int32))
                arr[b].dist_out = _fp(dist)
        T = np.zeros((max(n, 1), 16), np.float32)
        st = (Stats * max(n, 1))()
        rc = self._lib.icpk_align_batch(self._h, n, arr, C.byref(p), _fp(T), st)
        out = (T[:n].reshape(n, 4, 4), list(st)[:n], rc)
        return out + (assoc,) if associations else out

    def align_batch_device(self, pairs, params=None, **kw):
        """pairs: list of (src_ptr, ns, tgt_ptr, nt): device addresses of (3, N) float32 xyz-SoA
        blocks (plane stride = N floats) resident on this context's device."""
        p = params if params is not None else default_params(**kw)
        n = len(pairs)
        arr = (Pair * max(n, 1))()
        fpt = C.POINTER(C.c_float)
        for b, (sp, ns, tp, nt) in enumerate(pairs):
            arr[b].sx, arr[b].sy, arr[b].sz = (C.cast(C.c_void_p(sp + 4 * ns * k), fpt) for k in range(3))
            arr[b].tx, arr[b].ty, arr[b].tz = (C.cast(C.c_void_p(tp + 4 * nt * k), fpt) for k in range(3))
            arr[b].ns, arr[b].nt = ns, nt
        T = np.zeros((max(n, 1), 16), np.float32)
        st = (Stats * max(n, 1))()
        rc = self._lib.icpk_align_batch_device(self._h, n, arr, C.byref(p), _fp(T), st)
        return T[:n].reshape(n, 4, 4), list(st)[:n], rc

    # -- RCCL collectives behind the C ABI (icpk_comm.cpp) -------------------------------
    def comm_init(self, unique_id, rank, world):
        buf = C.create_string_buffer(bytes(unique_id), COMM_ID_BYTES)
        self._chk(self._lib.icpk_comm_init_rccl(self._h, buf, rank, world))

    def comm_destroy(self):
        self._chk(self._lib.icpk_comm_destroy(self._h))

    @property
    def comm_rank(self):
        return self._lib.icpk_comm_rank(self._h)

    @property
    def comm_world(self):
        return self._lib.icpk_comm_world(self._h)

    def comm_broadcast_target(self, root=0):
        self._chk(self._lib.icpk_comm_broadcast_target(self._h, root))

    def comm_gather_results(self, T_local, stats_local, n_total):
        """T_local (b, 4, 4) float32 and the list of Stats of this rank's block -> (T (n_total, 4, 4),
        S (n_total, 4) float64 = iterations, status, pairs, mse), identical on every rank.  (The integers cross the
        collective as int32 bit patterns: exact for any cloud size.)"""
        T_local = np.ascontiguousarray(T_local, np.float32).reshape(-1, 16)
        b = T_local.shape[0]
        st = (Stats * max(b, 1))()
        for k in range(b):
            if isinstance(stats_local[k], Stats):
                st[k] = stats_local[k]
            else:  # a row [iterations, status, pairs, mse] (batch.stats_rows)
                it, status, pairs, mse = stats_local[k]
                st[k].iterations, st[k].status, st[k].final_pairs, st[k].final_mse = int(it), int(status), int(pairs), float(mse)
        T = np.zeros((max(n_total, 1), 16), np.float32)
        S = np.zeros((max(n_total, 1), 4), np.float32)
        self._chk(self._lib.icpk_comm_gather_results(self._h, _fp(T_local) if b else None, st, b, n_total, _fp(T), _fp(S)))
        out = np.empty((n_total, 4), np.float64)
        out[:, :3] = S[:n_total, :3].view(np.int32)
        out[:, 3] = S[:n_total, 3]
        return T[:n_total].reshape(n_total, 4, 4), out

    def comm_allreduce_sums(self, sums, count):
        sums = np.ascontiguousarray(sums, np.float64).copy()
        cnt = C.c_int64(int(count))
        self._chk(self._lib.icpk_comm_allreduce_sums(self._h, sums.ctypes.data_as(C.POINTER(C.c_double)), sums.size,
                                                     C.byref(cnt)))
        return sums, cnt.value

    def comm_barrier(self):
        self._chk(self._lib.icpk_comm_barrier(self._h))

    def set_log_callback(self, fn):
        """fn(key, quantity, usec) -- same shape as logDeltaTime (SLAM.hpp:30)."""
        if fn is None:
            self._log_ref = LOG_FN()
        else:
            self._log_ref = LOG_FN(lambda k, q, us, _u: fn(k, q, us))
        self._chk(self._lib.icpk_set_log_callback(self._h, self._log_ref, None))
