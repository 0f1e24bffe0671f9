"""Python (ctypes) binding of the C ABI in include/gridvision_hip.h.

This is host-side plumbing for tests and bench.py; all compute happens in
libgridvision_hip.so (hand-written gfx950 kernels).  There is NO CPU fallback:
if the library is missing or no GPU is present, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build as _build
from .synth import BBOX_DTYPE, LSHAPE_DTYPE

GV_OK = 0
NODE_DTYPE = np.dtype([("x", np.float32), ("y", np.float32), ("z", np.float32), ("id", np.int32)])   # CellNode
STATUS = {0: "GV_OK", 1: "GV_ERR_BAD_ARG", 2: "GV_ERR_HIP", 3: "GV_ERR_RCCL", 4: "GV_ERR_NO_DEVICE",
          5: "GV_ERR_STATE", 6: "GV_ERR_TF"}

FRAME_BIN = 1 << 0
FRAME_RAYMARCH = 1 << 1
FRAME_BBOX_TEST = 1 << 2
FRAME_KEEP_CELL_IDX = 1 << 3
FRAME_KEEP_COUNTS = 1 << 4
FRAME_VISION_ORIENT = 1 << 5

TICK_VISION_ORIENT = 1 << 0
TICK_LIDAR_BIN = 1 << 1
TICK_LIDAR_RAYMARCH = 1 << 2
TICK_KEEP_DETS = 1 << 3     # [EXTENSION] X15: the tick leaves its detection list on the device
TICK_DETS = 128             # records of that list

INFLATE_KEEP_DIST2 = 1 << 0
INFLATE_OCCUPANCY_SCALE = 1 << 1

TRAJ_KEEP_POSE_COST = 1 << 0
TRAJ_DEVICE_POSES = 1 << 1
TRAJ_SCORE_DTYPE = np.dtype([("max_cost", np.int32), ("first_collision", np.int32), ("cost_sum", np.uint32),
                             ("n_off_map", np.int32)])   # gv_traj_score

NAV_BLOCKED = 0xFFFFFFFF
NAV_UNREACHABLE = 0xFFFFFFFE
NAV_SCORE_DTYPE = np.dtype([("sum", np.uint64), ("last", np.uint32), ("best", np.uint32), ("best_pose", np.int32),
                            ("n_bad", np.int32)])   # gv_nav_score

MOTION_DIFF = 0
MOTION_OMNI = 1
ROLLOUT_DEVICE_CONTROLS = 1 << 0
ROLLOUT_CONSTANT = 1 << 1
CONTROL_KEEP_TOTALS = 1 << 0
CONTROL_RESULT_DTYPE = np.dtype([("best", np.int32), ("n_valid", np.int32), ("best_total", np.uint64)])   # gv_control_result
MPPI_SHIFT = 1 << 0

DYN_MAX_OBJECTS = 128
DYN_SCORE_DTYPE = np.dtype([("max_cost", np.int32), ("first_collision", np.int32), ("cost_sum", np.uint32),
                            ("nearest_object", np.int32), ("min_dist2", np.float64)])   # gv_dyn_score
MOVING_OBJECT_DTYPE = np.dtype([("pose", LSHAPE_DTYPE), ("vx", np.float64), ("vy", np.float64)])   # gv_moving_object

TRACK_SLOTS = 128
TRACK_DEVICE_DETS = 1 << 0
TRACK_FEED_DYNAMIC = 1 << 1
TRACK_TICK_DETS = 1 << 2    # [EXTENSION] X15: the detections are the last tick's list
TRACK_DTYPE = np.dtype([("id", np.uint32), ("slot", np.int32), ("hits", np.int32), ("misses", np.int32), ("age", np.int32),
                        ("det", np.int32)] + [(n, np.float64) for n in ("x", "y", "vx", "vy", "qx", "qy", "qz", "qw", "length",
                                                                         "width", "p00", "p01", "p11")])   # gv_track
TRACK_INFO_DTYPE = np.dtype([(n, np.int32) for n in ("n_tracks", "n_confirmed", "n_exported", "n_matched", "n_born", "n_deleted",
                                                     "n_dropped", "n_invalid")] +
                            [("next_id", np.uint32), ("reserved", np.uint32)])   # gv_track_info
assert TRACK_DTYPE.itemsize == 128 and TRACK_INFO_DTYPE.itemsize == 40

# [EXTENSION] X16 scan-to-costmap matching (include/gridvision_hip_match.h)
MATCH_USE_BAND = 1 << 0      # MatchConfig.flags
MATCH_KEEP_SCORES = 1 << 0   # a call's flags
MATCH_MAX_HALF = 32
MATCH_RESULT_DTYPE = np.dtype([("best_t", np.int32), ("best_j", np.int32), ("best_i", np.int32), ("valid", np.int32),
                               ("n_used", np.uint32), ("best_score", np.uint32), ("guess_score", np.uint32),
                               ("reserved", np.uint32), ("x", np.float64), ("y", np.float64), ("yaw", np.float64),
                               ("reserved2", np.uint64)])   # gv_match_result
assert MATCH_RESULT_DTYPE.itemsize == 64
# every symbol include/gridvision_hip_match.h declares (a header of its own: ABI_SYMBOLS stays gridvision_hip.h's)
MATCH_SYMBOLS = ["gv_set_match_config", "gv_match_scan_async", "gv_match_scan", "gv_match_scan_host", "gv_match_rotations",
                 "gv_match_motion"]

# [EXTENSION] X17 path extraction from the distance field (include/gridvision_hip_path.h)
PATH_DIAGONAL = 1 << 0       # a call's flags
PATH_REACHED, PATH_TRUNCATED, PATH_OFF_MAP, PATH_BLOCKED, PATH_UNREACHABLE, PATH_STUCK = range(6)   # gv_nav_path_info.status
PATH_MAX_STARTS = 256
PATH_MAX_CAP = 65536
PATH_MAX_CELLS = 1 << 20     # S * cap
NAV_PATH_INFO_DTYPE = np.dtype([("status", np.int32), ("n_cells", np.int32), ("start_value", np.uint32), ("end_value", np.uint32),
                                ("start_entry", np.int32), ("end_entry", np.int32), ("n_diagonal", np.int32),
                                ("reserved", np.uint32)])   # gv_nav_path_info
assert NAV_PATH_INFO_DTYPE.itemsize == 32
# every symbol include/gridvision_hip_path.h declares
PATH_SYMBOLS = ["gv_nav_path_async", "gv_nav_path", "gv_nav_path_host", "gv_get_nav_path", "gv_device_nav_path",
                "gv_nav_field_from_path"]

# [EXTENSION] X18 wide-window matching by branch and bound (include/gridvision_hip_search.h)
SEARCH_USE_BAND = 1 << 0     # SearchConfig.flags
SEARCH_MAX_HALF = 128
SEARCH_STATS_DTYPE = np.dtype([("n_blocks", np.uint32), ("n_survivors", np.uint32), ("n_scored", np.uint32),
                               ("seed_block", np.uint32), ("lower_score", np.uint32), ("bound_max", np.uint32),
                               ("bound_sum", np.uint64)])   # gv_search_stats
assert SEARCH_STATS_DTYPE.itemsize == 32
# every symbol include/gridvision_hip_search.h declares
SEARCH_SYMBOLS = ["gv_set_search_config", "gv_match_search_async", "gv_match_search", "gv_match_search_host"]

# [EXTENSION] X19 frontier clusters (include/gridvision_hip_frontier.h; a second C namespace, gvx_: the gv_ set is frozen)
FRONTIER_USE_FIELD = 1 << 0  # a call's flags
FRONTIER_NONE = 0xFFFFFFFF   # labels[e] of a cell that is no frontier cell
FRONTIER_MAX_CAP = 4096
FRONTIER_DTYPE = np.dtype([("label", np.int32), ("n_cells", np.int32), ("min_x", np.int32), ("max_x", np.int32),
                           ("min_y", np.int32), ("max_y", np.int32), ("sum_x", np.uint64), ("sum_y", np.uint64),
                           ("centre_entry", np.int32), ("field_entry", np.int32), ("field_min", np.uint32),
                           ("goal_entry", np.int32), ("goal_x", np.float32), ("goal_y", np.float32)])   # gvx_frontier
FRONTIER_INFO_DTYPE = np.dtype([(n, np.int32) for n in ("n_frontier_cells", "n_components", "n_clusters", "n_written", "best",
                                                        "largest")] + [("flags", np.uint32), ("reserved", np.uint32)])   # gvx_frontier_info
assert FRONTIER_DTYPE.itemsize == 64 and FRONTIER_INFO_DTYPE.itemsize == 32
# every symbol include/gridvision_hip_frontier.h declares
FRONTIER_SYMBOLS = ["gvx_set_frontier_config", "gvx_frontier_async", "gvx_frontier", "gvx_frontier_host", "gvx_get_frontier_labels",
                    "gvx_device_frontier", "gvx_nav_field_from_frontier"]

# [EXTENSION] X20 information gain of exploration goals (include/gridvision_hip_gain.h; a header added after ABI 4 owns its
# prefix: gvx2_)
GAIN_USE_FIELD = 1 << 0        # a call's flags
GAIN_DEVICE_ENTRIES = 1 << 1
GAIN_INVALID = 1 << 0          # status bits of a record
GAIN_UNREACHABLE = 1 << 1
GAIN_BELOW_MIN = 1 << 2
GAIN_MAX_N = 4096
GAIN_MAX_RADIUS = 255
GAIN_NO_OPAQUE = 0xFFFFFFFF    # nearest_opaque_d2 when no ray ended on an opaque cell
GAIN_DTYPE = np.dtype([("entry", np.int32), ("status", np.uint32), ("n_unknown", np.int32), ("n_free", np.int32),
                       ("n_opaque", np.int32), ("rays_opaque", np.int32), ("rays_off_map", np.int32), ("rays_range", np.int32),
                       ("nearest_opaque_d2", np.uint32), ("dist", np.uint32), ("score", np.int64)])   # gvx2_gain_record
GAIN_INFO_DTYPE = np.dtype([("n_candidates", np.int32), ("n_ranked", np.int32), ("best", np.int32), ("best_entry", np.int32),
                            ("best_score", np.int64), ("flags", np.uint32), ("radius", np.int32)])   # gvx2_gain_info
assert GAIN_DTYPE.itemsize == 48 and GAIN_INFO_DTYPE.itemsize == 32
# every symbol include/gridvision_hip_gain.h declares
GAIN_SYMBOLS = ["gvx2_set_gain_config", "gvx2_gain_async", "gvx2_gain", "gvx2_frontier_gain_async", "gvx2_frontier_gain",
                "gvx2_gain_host", "gvx2_device_gain", "gvx2_nav_field_from_gain"]

# [EXTENSION] X21 shortcuts and waypoints of the resident paths (include/gridvision_hip_shortcut.h; its prefix: gvx3_)
SHORTCUT_NO_CORNER = 1 << 0    # a call's flags
SHORTCUT_OK, SHORTCUT_TRUNCATED, SHORTCUT_EMPTY = range(3)   # gvx3_shortcut_info.status
SHORTCUT_MAX_WINDOW = 4096
SHORTCUT_MAX_SPACING = 65535
SHORTCUT_MAX_WCAP = 65536
SHORTCUT_MAX_CELLS = 1 << 20   # S * wcap
SHORTCUT_INFO_DTYPE = np.dtype([("status", np.int32), ("n_waypoints", np.int32), ("n_anchors", np.int32), ("n_src", np.int32),
                                ("n_steps", np.int32), ("n_diag_steps", np.int32), ("max_cost_seen", np.int32),
                                ("end_entry", np.int32)])   # gvx3_shortcut_info
assert SHORTCUT_INFO_DTYPE.itemsize == 32
# every symbol include/gridvision_hip_shortcut.h declares
SHORTCUT_SYMBOLS = ["gvx3_set_shortcut_config", "gvx3_shortcut_async", "gvx3_shortcut", "gvx3_shortcut_host", "gvx3_get_shortcut",
                    "gvx3_device_shortcut", "gvx3_nav_field_from_shortcut"]

# gv_test_wave_op (csrc/gv_test_hooks.h), GV_TEST_WAVE_ dropped, in the enum's order; and the hook's two sentinels
WAVE_OPS = ["SCAN_ADD", "SCAN_MAX", "SCAN_MIN", "REDUCE_ADD", "REDUCE_MAX", "REDUCE_MIN",
            "SHIFT_DOWN_1", "SHIFT_DOWN_2", "SHIFT_DOWN_4", "SHIFT_DOWN_8", "GROUP_SUM_8", "GROUP_SUM_16", "MIN_KEY",
            "SUM_I32", "SUM_U32", "MAX_I32", "MAX_U32", "MAX64", "SUM64", "SHFL_XOR64", "BUTTERFLY", "TREE_SHFL",
            "DPP_F64_SHL_1", "DPP_F64_SHL_2", "DPP_F64_SHL_4", "DPP_F64_SHL_8", "RANK_LEADER",
            "BCAST_U64", "BCAST_I32", "BCAST_F64", "APPEND", "APPEND_ALL"]
WAVE_INACTIVE = 0xA5A5A5A5A5A5A5A5
WAVE_SKIPPED = 0x5A5A5A5A5A5A5A5A
WAVE_ALL_LANES = 0xFFFFFFFFFFFFFFFF

STAGES = ("detections", "points", "ray_ends", "ray_march", "finalize")

# every symbol include/gridvision_hip.h declares
ABI_SYMBOLS = [
    "gv_create", "gv_destroy", "gv_last_error", "gv_abi_version", "gv_grid_geometry", "gv_reset",
    "gv_set_transforms", "gv_cloud_upload_xyz", "gv_cloud_upload_pointcloud2",
    "gv_transform_lidar_to_camera", "gv_extract_cloud_per_bbox", "gv_compute_depth_for_bboxes",
    "gv_convert_pixels_to_3d", "gv_compute_bbox_pose", "gv_segment_ground_plane",
    "gv_compute_bbox_pose_ground_removed", "gv_vision_post_process",
    "gv_transform_lshape_objects", "gv_extract_bboxes", "gv_filter_bboxes", "gv_get_intrinsics",
    "gv_update_map", "gv_update_map_poses", "gv_update_map_points", "gv_to_occupancy_grid",
    "gv_get_log_odds", "gv_get_occupancy", "gv_set_log_odds", "gv_frame_set_detections",
    "gv_frame_enqueue", "gv_synchronize", "gv_process_frame", "gv_get_hits", "gv_get_miss",
    "gv_get_cell_idx", "gv_get_bbox_id", "gv_get_ray_stats", "gv_stream", "gv_time_frames",
    "gv_time_frame_stages", "gv_comm_unique_id", "gv_comm_init", "gv_comm_destroy",
    "gv_process_frame_sharded", "gv_comm_band",
    "gv_cloud_upload_xyz_async", "gv_cloud_upload_pointcloud2_async", "gv_cloud_upload_wait", "gv_host_alloc",
    "gv_host_free", "gv_frame_set_detections_async", "gv_frame_fence",
    "gv_to_occupancy_grid_async", "gv_frame_enqueue_sharded", "gv_time_frame_sharded_stages", "gv_shard_band_rows",
    "gv_shard_slice_words", "gv_device_layers", "gv_tick_enqueue", "gv_tick_wait", "gv_tick",
    "gv_comm_info", "gv_publish_grid_async", "gv_grid_move", "gv_set_height_band",
    "gv_inflation_cost_table", "gv_set_inflation", "gv_inflate", "gv_get_costmap", "gv_get_obstacle_dist2",
    "gv_publish_costmap_async",
    "gv_set_footprint", "gv_score_trajectories_async", "gv_score_trajectories", "gv_footprint_cells",
    "gv_nav_step_table", "gv_set_nav_config", "gv_nav_field", "gv_get_nav_field", "gv_device_nav_field",
    "gv_score_nav_async", "gv_score_nav",
    "gv_set_motion_model", "gv_rollout_async", "gv_rollout", "gv_device_rollout", "gv_get_rollout", "gv_rollout_poses",
    "gv_control_step_async", "gv_control_step", "gv_control_select",
    "gv_set_mppi", "gv_mppi_set_nominal", "gv_get_mppi_nominal", "gv_mppi_sample_async", "gv_mppi_sample",
    "gv_device_controls", "gv_get_controls", "gv_mppi_update_async", "gv_mppi_update", "gv_mppi_cycle_async",
    "gv_mppi_cycle", "gv_mppi_words", "gv_mppi_sample_controls", "gv_mppi_average",
    "gv_set_mppi_limits", "gv_mppi_constrain", "gv_get_mppi_control_costs", "gv_mppi_control_costs", "gv_mppi_average_cc",
    "gv_dyn_cost_table", "gv_set_dyn_config", "gv_set_moving_objects", "gv_score_dynamic_async", "gv_score_dynamic",
    "gv_dyn_score_poses", "gv_control_select_dyn",
    "gv_set_track_config", "gv_set_tracks", "gv_get_tracks", "gv_track_update_async", "gv_track_update", "gv_track_step",
]


class CamParams(C.Structure):
    _fields_ = [("network_h", C.c_int32), ("network_w", C.c_int32), ("orig_h", C.c_int32),
                ("orig_w", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float)]


class Transform(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("qx", "qy", "qz", "qw", "tx", "ty", "tz")]


class GridInfo(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("resolution", C.c_double),
                ("origin_x", C.c_double), ("origin_y", C.c_double)]


class GridMoveInfo(C.Structure):
    """gv_grid_move_info: what one gv_grid_move did"""
    _fields_ = [("applied", C.c_int32), ("cos_yaw", C.c_double), ("sin_yaw", C.c_double), ("tx", C.c_double),
                ("ty", C.c_double), ("res_yaw", C.c_double), ("res_x", C.c_double), ("res_y", C.c_double)]


class HeightBand(C.Structure):
    """gv_height_band: obstacle height band of the lidar map update"""
    _fields_ = [("z_ground", C.c_float), ("z_max", C.c_float), ("ground_clears", C.c_int32)]


class Inflation(C.Structure):
    """gv_inflation: radii in metres, the scaling factor in 1/m, lethal iff int8 >= lethal_threshold, INFLATE_* flags"""
    _fields_ = [("inscribed_radius", C.c_double), ("inflation_radius", C.c_double), ("cost_scaling_factor", C.c_double),
                ("lethal_threshold", C.c_int32), ("flags", C.c_int32)]


class Footprint(C.Structure):
    """gv_footprint: n_vertices 0 (centre cell only) or 3..16, vertices in metres in the robot frame (x forward), a pose
    collides at cost >= collision_cost, a pose that leaves the map costs off_map_cost"""
    _fields_ = [("n_vertices", C.c_int32), ("vx", C.c_double * 16), ("vy", C.c_double * 16),
                ("collision_cost", C.c_int32), ("off_map_cost", C.c_int32), ("flags", C.c_uint32)]

    @classmethod
    def of(cls, vertices, collision_cost=253, off_map_cost=255, flags=0):
        """vertices: a sequence of (x, y), empty for the circular robot"""
        f = cls()
        f.n_vertices = len(vertices)
        for i, (x, y) in enumerate(list(vertices)[:16]):
            f.vx[i], f.vy[i] = float(x), float(y)
        f.collision_cost, f.off_map_cost, f.flags = int(collision_cost), int(off_map_cost), int(flags)
        return f


class NavConfig(C.Structure):
    """gv_nav_config: a cell of cost >= obstacle_cost is blocked, entering a traversable cell of cost v costs
    1 + cost_weight * v"""
    _fields_ = [("obstacle_cost", C.c_int32), ("cost_weight", C.c_int32), ("flags", C.c_uint32)]


class NavInfo(C.Structure):
    """gv_nav_info: what one gv_nav_field did"""
    _fields_ = [("n_seeds_used", C.c_int32), ("rounds", C.c_int32)]


class MotionModel(C.Structure):
    """gv_motion_model: MOTION_DIFF (controls v, w) or MOTION_OMNI (vx, vy, w), the step dt in seconds"""
    _fields_ = [("model", C.c_int32), ("dt", C.c_double), ("flags", C.c_uint32)]

    @property
    def n_controls(self):
        return 3 if self.model == MOTION_OMNI else 2


class CriticWeights(C.Structure):
    """gv_critic_weights: integer weights 0..65535 of the X7 record (cost_sum, max_cost) and of the X9 record (last,
    sum, best); any nav weight non-zero makes the control step sample the distance field"""
    _fields_ = [("w_cost_sum", C.c_uint32), ("w_max_cost", C.c_uint32), ("w_nav_last", C.c_uint32),
                ("w_nav_sum", C.c_uint32), ("w_nav_best", C.c_uint32), ("flags", C.c_uint32)]


class MppiConfig(C.Structure):
    """gv_mppi_config: per-channel noise sigma and clamp [u_min, u_max], the softmax temperature lambda in units of a
    total"""
    _fields_ = [("sigma", C.c_double * 3), ("u_min", C.c_float * 3), ("u_max", C.c_float * 3), ("lambda_", C.c_double),
                ("flags", C.c_uint32)]

    @classmethod
    def of(cls, sigma, u_min=None, u_max=None, lambda_=1.0, flags=0):
        """sigma, u_min, u_max: up to three values each (missing clamps are -inf / +inf, missing sigmas 0)"""
        c = cls()
        sigma = list(sigma)
        lo = list(u_min) if u_min is not None else [-np.inf] * len(sigma)
        hi = list(u_max) if u_max is not None else [np.inf] * len(sigma)
        for i in range(3):
            c.sigma[i] = float(sigma[i]) if i < len(sigma) else 0.0
            c.u_min[i] = float(lo[i]) if i < len(lo) else -np.inf
            c.u_max[i] = float(hi[i]) if i < len(hi) else np.inf
        c.lambda_, c.flags = float(lambda_), int(flags)
        return c


class MppiLimits(C.Structure):
    """gv_mppi_limits: per-channel rate limits per second (inf: none), the control in force before step 0 (NaN: free), the
    minimum turning radius in metres (0: off) and the control-cost weight gamma (0: off)"""
    _fields_ = [("rate_up", C.c_double * 3), ("rate_down", C.c_double * 3), ("u_prev", C.c_float * 3),
                ("min_turn_radius", C.c_double), ("gamma", C.c_double), ("flags", C.c_uint32)]

    @classmethod
    def of(cls, rate_up=(), rate_down=(), u_prev=(), min_turn_radius=0.0, gamma=0.0, flags=0):
        """rate_up, rate_down, u_prev: up to three values each (missing rates are +inf, missing u_prev NaN); of() alone
        is the neutral struct that changes nothing"""
        m = cls()
        up, dn, prev = list(rate_up), list(rate_down), list(u_prev)
        for i in range(3):
            m.rate_up[i] = float(up[i]) if i < len(up) else np.inf
            m.rate_down[i] = float(dn[i]) if i < len(dn) else np.inf
            m.u_prev[i] = float(prev[i]) if i < len(prev) else np.nan
        m.min_turn_radius, m.gamma, m.flags = float(min_turn_radius), float(gamma), int(flags)
        return m


class DynConfig(C.Structure):
    """gv_dyn_config: the robot as n_circles circles of one radius at off_x on its x axis, the cost table's radii,
    scaling factor and distance quantum, the time t0 + p * dt of pose p, the collision cost and the two weights of the
    control step"""
    _fields_ = [("n_circles", C.c_int32), ("off_x", C.c_double * 8), ("radius", C.c_double), ("influence_radius", C.c_double),
                ("cost_scaling_factor", C.c_double), ("quantum", C.c_double), ("t0", C.c_double), ("dt", C.c_double),
                ("collision_cost", C.c_int32), ("w_sum", C.c_uint32), ("w_max", C.c_uint32), ("flags", C.c_uint32)]

    @classmethod
    def of(cls, off_x=(0.0,), radius=0.5, influence_radius=None, cost_scaling_factor=3.0, quantum=0.05, t0=0.0, dt=0.1,
           collision_cost=253, w_sum=1, w_max=0, flags=0):
        c = cls()
        c.n_circles = len(off_x)
        for i, v in enumerate(list(off_x)[:8]):
            c.off_x[i] = float(v)
        c.radius = float(radius)
        c.influence_radius = float(radius if influence_radius is None else influence_radius)
        c.cost_scaling_factor, c.quantum, c.t0, c.dt = float(cost_scaling_factor), float(quantum), float(t0), float(dt)
        c.collision_cost, c.w_sum, c.w_max, c.flags = int(collision_cost), int(w_sum), int(w_max), int(flags)
        return c


class TrackConfig(C.Structure):
    """gv_track_config: the association gate, the filter's three sigmas, the speed below which a track is exported as
    standing, the hits that confirm a track and the consecutive misses it survives"""
    _fields_ = [("gate", C.c_double), ("sigma_accel", C.c_double), ("sigma_meas", C.c_double), ("sigma_v0", C.c_double),
                ("min_speed", C.c_double), ("confirm_hits", C.c_int32), ("max_misses", C.c_int32), ("flags", C.c_uint32)]

    @classmethod
    def of(cls, gate=2.0, sigma_accel=1.0, sigma_meas=0.2, sigma_v0=5.0, min_speed=0.0, confirm_hits=2, max_misses=3, flags=0):
        return cls(float(gate), float(sigma_accel), float(sigma_meas), float(sigma_v0), float(min_speed), int(confirm_hits),
                   int(max_misses), int(flags))


class MatchConfig(C.Structure):
    """gv_match_config: the window's half-widths in cells (wx, wy) and yaw steps (wt), the yaw step, every stride-th
    point of the cloud, the used points a valid match needs, MATCH_USE_BAND"""
    _fields_ = [("wx", C.c_int32), ("wy", C.c_int32), ("wt", C.c_int32), ("stride", C.c_int32), ("yaw_step", C.c_double),
                ("min_points", C.c_int32), ("flags", C.c_uint32)]

    @classmethod
    def of(cls, wx=8, wy=8, wt=4, yaw_step=0.01, stride=1, min_points=1, use_band=False, flags=0):
        return cls(int(wx), int(wy), int(wt), int(stride), float(yaw_step), int(min_points),
                   int(flags) | (MATCH_USE_BAND if use_band else 0))

    @property
    def shape(self):
        """(NT, NY, NX) of the score volume"""
        return 2 * self.wt + 1, 2 * self.wy + 1, 2 * self.wx + 1


class SearchConfig(C.Structure):
    """gv_search_config: MatchConfig's fields with half-widths up to SEARCH_MAX_HALF, and block_log2 (blocks of S x S
    shifts, S = 1 << block_log2, 1..4)"""
    _fields_ = [("wx", C.c_int32), ("wy", C.c_int32), ("wt", C.c_int32), ("stride", C.c_int32), ("yaw_step", C.c_double),
                ("min_points", C.c_int32), ("flags", C.c_uint32), ("block_log2", C.c_int32), ("reserved", C.c_int32)]

    @classmethod
    def of(cls, wx=64, wy=64, wt=4, yaw_step=0.01, stride=1, min_points=1, use_band=False, flags=0, block_log2=3, reserved=0):
        return cls(int(wx), int(wy), int(wt), int(stride), float(yaw_step), int(min_points),
                   int(flags) | (SEARCH_USE_BAND if use_band else 0), int(block_log2), int(reserved))

    @property
    def shape(self):
        """(NT, NY, NX) of the window"""
        return 2 * self.wt + 1, 2 * self.wy + 1, 2 * self.wx + 1


class FrontierConfig(C.Structure):
    """gvx_frontier_config: FREE is 0..free_max, UNKNOWN unknown_min..unknown_max of the packed layer; a frontier cell's
    cost is below max_cost (256: the costmap is not read); a cluster has min_cells cells at least"""
    _fields_ = [("free_max", C.c_int32), ("unknown_min", C.c_int32), ("unknown_max", C.c_int32), ("max_cost", C.c_int32),
                ("min_cells", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]

    @classmethod
    def of(cls, free_max=25, unknown_min=40, unknown_max=60, max_cost=256, min_cells=1, flags=0):
        return cls(int(free_max), int(unknown_min), int(unknown_max), int(max_cost), int(min_cells), int(flags))


class GainConfig(C.Structure):
    """gvx2_gain_config: the classes as in FrontierConfig (everything neither FREE nor UNKNOWN is OPAQUE); rays of radius
    cells; BELOW_MIN under min_gain unknown cells; score = w_gain * n_unknown - w_dist * dist"""
    _fields_ = [("free_max", C.c_int32), ("unknown_min", C.c_int32), ("unknown_max", C.c_int32), ("radius", C.c_int32),
                ("min_gain", C.c_int32), ("w_gain", C.c_int32), ("w_dist", C.c_int32), ("reserved", C.c_uint32)]

    @classmethod
    def of(cls, free_max=25, unknown_min=40, unknown_max=60, radius=32, min_gain=0, w_gain=1, w_dist=0, reserved=0):
        return cls(int(free_max), int(unknown_min), int(unknown_max), int(radius), int(min_gain), int(w_gain), int(w_dist), int(reserved))


class ShortcutConfig(C.Structure):
    """gvx3_shortcut_config: a cell is CLEAR iff its cost <= max_cost; a shortcut reaches at most window path cells ahead;
    waypoints every spacing cells of a segment's line (0: anchors only)"""
    _fields_ = [("max_cost", C.c_int32), ("window", C.c_int32), ("spacing", C.c_int32), ("reserved", C.c_uint32 * 5)]

    @classmethod
    def of(cls, max_cost=252, window=64, spacing=0):
        return cls(int(max_cost), int(window), int(spacing))


class MatchGuess(C.Structure):
    """gv_match_guess: the pose of the current base frame in the grid's frame"""
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("yaw", C.c_double)]


def _guess(guess):
    return guess if isinstance(guess, MatchGuess) else MatchGuess(*[float(v) for v in guess])


def moving_objects(rows):
    """a MOVING_OBJECT_DTYPE array from rows of (px, py, yaw, length, width, vx, vy): the quaternion is that of the yaw
    about z"""
    rows = np.asarray(rows, np.float64).reshape(-1, 7)
    o = np.zeros(len(rows), MOVING_OBJECT_DTYPE)
    o["pose"]["px"], o["pose"]["py"] = rows[:, 0], rows[:, 1]
    o["pose"]["qz"], o["pose"]["qw"] = np.sin(0.5 * rows[:, 2]), np.cos(0.5 * rows[:, 2])
    o["pose"]["length"], o["pose"]["width"] = rows[:, 3], rows[:, 4]
    o["vx"], o["vy"] = rows[:, 5], rows[:, 6]
    return o


class FrameDesc(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("bboxes", C.c_void_p), ("n_bboxes", C.c_int32),
                ("poses", C.c_void_p), ("n_poses", C.c_int32), ("orient", C.c_void_p),
                ("conf", C.c_void_p), ("dims", C.c_void_p)]


class TickDesc(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("bboxes", C.c_void_p), ("n_bboxes", C.c_int32), ("orient", C.c_void_p),
                ("conf", C.c_void_p), ("dims", C.c_void_p), ("n_net", C.c_int32), ("k_near", C.c_int32),
                ("grid_out", C.c_void_p)]


class TickResult(C.Structure):
    _fields_ = [("n_static", C.c_int32), ("n_dynamic", C.c_int32), ("static_bboxes", C.c_void_p), ("depths", C.c_void_p),
                ("base_points_xyz", C.c_void_p), ("poses", C.c_void_p), ("n_poses", C.c_int32), ("pca_empty", C.c_int32)]


class RansacStateOut(C.Structure):
    """gv_test_ransac_state_t (csrc/gv_test_hooks.h)"""
    _fields_ = [("plane", C.c_float * 4), ("refined", C.c_float * 4), ("m", C.c_uint64), ("n_inliers", C.c_uint64),
                ("best_count", C.c_uint32), ("pad", C.c_uint32)]


class PinnedI8:
    """int8 array in page-locked host memory: the packed grid's landing place (gv_tick grid_out, gv_to_occupancy_grid_async)"""

    def __init__(self, n):
        self._lib = load()
        self._p = C.c_void_p()
        rc = self._lib.gv_host_alloc(C.byref(self._p), C.c_size_t(max(int(n), 1)))
        if rc:
            raise GVError(rc, "gv_host_alloc")
        self.array = np.ctypeslib.as_array(C.cast(self._p, C.POINTER(C.c_int8)), shape=(int(n),))

    def close(self):
        if self._p:
            self.array = None
            self._lib.gv_host_free(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GVError(RuntimeError):
    def __init__(self, code, where, detail=""):
        super().__init__(f"{where}: {STATUS.get(code, code)} {detail}".strip())
        self.code = code


_LIB = None


def lib_path() -> str:
    return _build.LIB


def load(build_if_missing: bool = True):
    """Load libgridvision_hip.so (builds it with hipcc when stale/missing)."""
    global _LIB
    if _LIB is None:
        path = _build.build() if build_if_missing else _build.LIB
        alt = os.environ.get("GV_LIB_AB")   # A/B measurements only: another build of the same library
        if alt:
            path = alt
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: build it with hipcc (python -m gvamd.build)")
        _LIB = C.CDLL(path)
        _LIB.gv_last_error.restype = C.c_char_p
        _LIB.gv_stream.restype = C.c_void_p
    return _LIB


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _boxes(bboxes):
    return np.ascontiguousarray(bboxes, dtype=BBOX_DTYPE)


def _pose_outputs(b):
    """(poses, valid) for the boxes b: one entry at least, so that an empty call still hands the library a pointer"""
    return np.zeros(max(len(b), 1), dtype=LSHAPE_DTYPE), np.zeros(max(len(b), 1), np.uint8)


def _pose_batch(poses, device_ptr, K=None, P=None):
    """(src, K, P, flags) of a (K, P, 3) pose batch for the scoring calls.  The asynchronous calls give K and P and their
    array is used where it is (it stays the caller's until completion); otherwise K and P come from the shape and host
    poses are read from a contiguous float32 copy, which the returned pointer keeps alive.  device_ptr: the floats are
    read from that device address and only the shape of `poses` is used."""
    if K is None:
        shape = np.shape(poses)
        assert len(shape) == 3 and shape[2] == 3, "poses is (K, P, 3)"
        K, P = int(shape[0]), int(shape[1])
        poses = _f32(poses) if device_ptr is None else None
    if device_ptr is not None:
        return C.c_void_p(device_ptr), K, P, TRAJ_DEVICE_POSES
    return _ptr(poses), K, P, 0


def make_tf(v):
    return Transform(*[float(t) for t in v]) if v is not None else None


def extract_bboxes(boxes, scores, conf_thr, iou_thr, orig_w, orig_h, resize):
    """object_detection::extract_bboxes on precomputed detector outputs (host side)."""
    boxes, scores = _f32(boxes), _f32(scores)
    n, c = scores.shape
    out = np.zeros(max(n, 1), dtype=BBOX_DTYPE)
    m = C.c_int32(0)
    rc = load().gv_extract_bboxes(_ptr(boxes), _ptr(scores), C.c_int32(n), C.c_int32(c), C.c_double(conf_thr),
                                  C.c_double(iou_thr), C.c_int32(orig_w), C.c_int32(orig_h), C.c_int32(resize),
                                  _ptr(out), C.byref(m))
    if rc:
        raise GVError(rc, "gv_extract_bboxes")
    return out[:m.value].copy()


def filter_bboxes(bboxes):
    b = np.ascontiguousarray(bboxes, dtype=BBOX_DTYPE)
    st = np.zeros(max(len(b), 1), dtype=BBOX_DTYPE)
    dy = np.zeros(max(len(b), 1), dtype=BBOX_DTYPE)
    ns, nd = C.c_int32(0), C.c_int32(0)
    rc = load().gv_filter_bboxes(_ptr(b), C.c_int32(len(b)), _ptr(st), C.byref(ns), _ptr(dy), C.byref(nd))
    if rc:
        raise GVError(rc, "gv_filter_bboxes")
    return st[:ns.value].copy(), dy[:nd.value].copy()


def shard_band_rows(rank, world, ny):
    """rows [y0, y1) rank `rank` of `world` finalises (the product's own band function; needs no GPU)"""
    y0, y1 = C.c_int32(), C.c_int32()
    rc = load().gv_shard_band_rows(C.c_int32(rank), C.c_int32(world), C.c_int32(ny), C.byref(y0), C.byref(y1))
    if rc:
        raise GVError(rc, "gv_shard_band_rows")
    return y0.value, y1.value


def tick_dets_host(cam, valid, tf_bc, empty=False):
    """test hook (csrc/gv_test_hooks.h): the detection list k_tick_dets makes of the camera-frame poses `cam`
    (LSHAPE_DTYPE) and their valid flags under base<-camera tf_bc (a Transform or its seven values), from the same text
    compiled for the host: (the 128 records, n, n_total) (host only; needs no GPU)"""
    cam = np.ascontiguousarray(cam, LSHAPE_DTYPE).reshape(-1)
    valid = np.ascontiguousarray(valid, np.uint8).reshape(-1)
    assert len(cam) == len(valid)
    tf = tf_bc if isinstance(tf_bc, Transform) else make_tf(tf_bc)
    out, n, nt = np.zeros(TICK_DETS, LSHAPE_DTYPE), C.c_int32(-1), C.c_int32(-1)
    rc = load().gv_test_tick_dets_host(_ptr(cam) if len(cam) else None, _ptr(valid) if len(cam) else None, C.c_int32(len(cam)),
                                       C.c_int32(1 if empty else 0), C.byref(tf), _ptr(out), C.byref(n), C.byref(nt))
    if rc:
        raise GVError(rc, "gv_test_tick_dets_host")
    return out, n.value, nt.value


def shard_plan(nx, ny, world):
    """test hook (csrc/gv_test_hooks.h): the sharded frame's plan for an nx x ny grid and `world` ranks, as a dict of
    slice, chunk (words), equal_bands, cnt0 (cells) and rows = [(y0, y1)] per rank (host only; needs no GPU)"""
    sl, ch, cnt0, eq = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
    rows = np.zeros(2 * world, np.int32)
    rc = load().gv_test_shard_plan(C.c_int32(nx), C.c_int32(ny), C.c_int32(world), C.byref(sl), C.byref(ch), C.byref(eq),
                                   C.byref(cnt0), _ptr(rows))
    if rc:
        raise GVError(rc, "gv_test_shard_plan")
    return dict(slice=sl.value, chunk=ch.value, equal_bands=bool(eq.value), cnt0=cnt0.value,
                rows=[(int(rows[2 * r]), int(rows[2 * r + 1])) for r in range(world)])


class _SectorPlan(C.Structure):
    _fields_ = [("len", C.c_int32 * 8), ("imax", C.c_int32), ("log2s_oct", C.c_int32 * 8), ("rev_oct", C.c_int32 * 8),
                ("cap", C.c_int32), ("log2m", C.c_int32), ("marks_words", C.c_int32), ("oct_perm", C.c_uint32),
                ("reorder", C.c_int32), ("wg_base", C.c_uint32 * 9), ("n_helpers", C.c_int32), ("flat_k", C.c_int32),
                ("march_limit", C.c_uint32), ("flat_direct", C.c_uint32), ("ch", C.c_int32), ("lds_bytes", C.c_int64),
                ("total_workgroups", C.c_uint32), ("stat_slots", C.c_int64), ("violations", C.c_uint32)]


# host::SectorPlan's violation bits (csrc/gv_host_math.hpp), in the order of its enum
SECTOR_VIOLATIONS = ("wide_column", "sector_count", "workgroups", "log2m", "cap", "marks_words", "lds")
SECTOR_WG_FIELDS = ("octant", "sector", "helper", "part", "nparts", "stat_slot", "idle")


def sector_plan(nx, ny, cx, cy, n, workgroups=True):
    """test hook (csrc/gv_test_hooks.h): the sector ray stage's plan for an nx x ny grid, origin cell (cx, cy) and a cloud
    of n points, under the knobs of the environment: a dict of the plan's fields (arrays as lists), `violations` (the bit
    mask) and `violated` (names from SECTOR_VIOLATIONS), and wg = int32 array (total_workgroups, 7) of SECTOR_WG_FIELDS
    per workgroup of the dispatch order (host only; needs no GPU)"""
    P = _SectorPlan()
    lib = load()
    rc = lib.gv_test_sector_plan(C.c_int32(nx), C.c_int32(ny), C.c_int32(cx), C.c_int32(cy), C.c_int64(n), C.byref(P), None,
                                 C.c_int64(0))
    if rc:
        raise GVError(rc, "gv_test_sector_plan")
    d = {k: (list(getattr(P, k)) if hasattr(getattr(P, k), "__len__") else int(getattr(P, k))) for k, _ in _SectorPlan._fields_}
    d["violated"] = [name for b, name in enumerate(SECTOR_VIOLATIONS) if d["violations"] >> b & 1]
    if workgroups:
        wg = np.zeros((max(d["total_workgroups"], 1), 7), np.int32)
        rc = lib.gv_test_sector_plan(C.c_int32(nx), C.c_int32(ny), C.c_int32(cx), C.c_int32(cy), C.c_int64(n), C.byref(P),
                                     _ptr(wg), C.c_int64(len(wg)))
        if rc:
            raise GVError(rc, "gv_test_sector_plan")
        d["wg"] = wg[:d["total_workgroups"]]
    return d


def inflation_cost_table(cfg, resolution):
    """the uint8 cost table (d2max + 1 entries) an Inflation gives at `resolution` (host only; needs no GPU)"""
    table = np.zeros(4096, np.uint8)
    n = C.c_int32(0)
    rc = load().gv_inflation_cost_table(C.byref(cfg), C.c_double(resolution), _ptr(table), C.c_int32(table.size), C.byref(n))
    if rc:
        raise GVError(rc, "gv_inflation_cost_table")
    return table[:n.value].copy()


def footprint_cells(grid_x, grid_y, resolution, footprint, x, y, yaw):
    """the cells one pose tests on the grid GridVisionHIP(grid_x, grid_y, resolution) holds: int32 array, the centre cell
    first, then the outline edge by edge, each iy * nx + ix; None for an off-map pose (host only; needs no GPU)"""
    lib = load()
    n = C.c_int32(0)
    cells = np.zeros(256, np.int32)
    for _ in range(2):
        rc = lib.gv_footprint_cells(C.c_uint8(grid_x), C.c_uint8(grid_y), C.c_double(resolution), C.byref(footprint),
                                    C.c_float(x), C.c_float(y), C.c_float(yaw), _ptr(cells), C.c_int32(cells.size), C.byref(n))
        if rc == 0:
            return None if n.value < 0 else cells[:n.value].copy()
        if n.value <= cells.size:
            break
        cells = np.zeros(n.value, np.int32)
    raise GVError(rc, "gv_footprint_cells")


def nav_step_table(cfg):
    """the uint32 step table (256 entries, 0 = blocked) a NavConfig gives (host only; needs no GPU)"""
    table = np.zeros(256, np.uint32)
    rc = load().gv_nav_step_table(C.byref(cfg), _ptr(table))
    if rc:
        raise GVError(rc, "gv_nav_step_table")
    return table


def _motion_model(model, dt=None):
    """a MotionModel from one, or from (model, dt)"""
    return model if isinstance(model, MotionModel) else MotionModel(int(model), float(dt), 0)


def _control_batch(model, controls, constant):
    """(float32 array, K, P or None) of a controls array: (K, P, C), or (K, C) when constant"""
    c = _f32(controls)
    want = 2 if constant else 3
    assert c.ndim == want and c.shape[-1] == model.n_controls, "controls is (K, P, C), or (K, C) when constant"
    return c, int(c.shape[0]), (None if constant else int(c.shape[1]))


def rollout_poses(model, start, controls, constant=False, P=None):
    """the float32 (K, P, 3) poses a MotionModel makes of float32 controls (K, P, C), or (K, C) held for P steps when
    constant, from start = (x, y, yaw): the library's own arithmetic with the host's sin and cos (host only; needs no
    GPU)"""
    c, K, p = _control_batch(model, controls, constant)
    P = int(P) if constant else p
    out = np.zeros((K, P, 3), np.float32)
    s = (C.c_double * 3)(*[float(v) for v in start])
    rc = load().gv_rollout_poses(C.byref(model), s, _ptr(c), C.c_int32(K), C.c_int32(P),
                                 C.c_uint32(ROLLOUT_CONSTANT if constant else 0), _ptr(out))
    if rc:
        raise GVError(rc, "gv_rollout_poses")
    return out


def control_select(weights, traj, nav=None, keep_totals=False):
    """combine and select over TRAJ_SCORE_DTYPE / NAV_SCORE_DTYPE records (nav may be None when no nav weight is set):
    the CONTROL_RESULT_DTYPE record, and with keep_totals also the uint64 totals (host only; needs no GPU)"""
    traj = np.ascontiguousarray(traj, TRAJ_SCORE_DTYPE)
    nav = np.ascontiguousarray(nav, NAV_SCORE_DTYPE) if nav is not None else None
    assert nav is None or len(nav) == len(traj)
    res = np.zeros(1, CONTROL_RESULT_DTYPE)
    totals = np.zeros(max(len(traj), 1), np.uint64) if keep_totals else None
    rc = load().gv_control_select(C.byref(weights), _ptr(traj), _ptr(nav), C.c_int32(len(traj)), _ptr(res), _ptr(totals))
    if rc:
        raise GVError(rc, "gv_control_select")
    return (res[0], totals[:len(traj)]) if keep_totals else res[0]


def _objects(objs):
    return np.ascontiguousarray(objs if objs is not None else [], MOVING_OBJECT_DTYPE).reshape(-1)


def dyn_cost_table(cfg):
    """the uint8 cost table (T entries) a DynConfig gives (host only; needs no GPU)"""
    table = np.zeros(4096, np.uint8)
    n = C.c_int32(0)
    rc = load().gv_dyn_cost_table(C.byref(cfg), _ptr(table), C.c_int32(table.size), C.byref(n))
    if rc:
        raise GVError(rc, "gv_dyn_cost_table")
    return table[:n.value].copy()


def dyn_score_poses(cfg, objs, poses, keep_pose_cost=False):
    """the DYN_SCORE_DTYPE records of float32 (K, P, 3) poses against MOVING_OBJECT_DTYPE objects under a DynConfig, and
    with keep_pose_cost also the uint8 (K, P) pose costs: the library's own arithmetic with the host's sin and cos (host
    only; needs no GPU)"""
    src, K, P, _ = _pose_batch(poses, None)
    o = _objects(objs)
    scores = np.zeros(max(K, 1), DYN_SCORE_DTYPE)
    pc = np.zeros(max(K * P, 1), np.uint8) if keep_pose_cost else None
    rc = load().gv_dyn_score_poses(C.byref(cfg), _ptr(o), C.c_int32(len(o)), src, C.c_int32(K), C.c_int32(P), _ptr(scores),
                                   _ptr(pc))
    if rc:
        raise GVError(rc, "gv_dyn_score_poses")
    return (scores[:K], pc[:K * P].reshape(K, P)) if keep_pose_cost else scores[:K]


def _detections(dets):
    return np.ascontiguousarray(dets if dets is not None else np.zeros(0, LSHAPE_DTYPE), LSHAPE_DTYPE).reshape(-1)


def _motion(motion):
    """None, a Transform, or (qx, qy, qz, qw, tx, ty, tz)"""
    if motion is None or isinstance(motion, Transform):
        return motion
    return Transform(*[float(v) for v in motion])


def track_step(cfg, tracks, next_id, dets, dt, motion=None):
    """one update of the tracker on the host (gv_track_step; needs no GPU): tracks a TRACK_DTYPE array of the live
    records in ascending slot order, dets an LSHAPE_DTYPE array.  Returns (tracks, next_id, info, objs): the new live
    records, the counter, the TRACK_INFO_DTYPE record and the exported MOVING_OBJECT_DTYPE array."""
    buf = np.zeros(TRACK_SLOTS, TRACK_DTYPE)
    tracks = np.ascontiguousarray(tracks if tracks is not None else buf[:0], TRACK_DTYPE).reshape(-1)
    assert len(tracks) <= TRACK_SLOTS
    buf[:len(tracks)] = tracks
    z = _detections(dets)
    n_t, nid, n_o = C.c_int32(len(tracks)), C.c_uint32(int(next_id)), C.c_int32(0)
    info, objs, m = np.zeros(1, TRACK_INFO_DTYPE), np.zeros(TRACK_SLOTS, MOVING_OBJECT_DTYPE), _motion(motion)
    rc = load().gv_track_step(C.byref(cfg), _ptr(buf), C.byref(n_t), C.byref(nid), _ptr(z) if len(z) else None, C.c_int32(len(z)),
                              C.c_double(dt), C.byref(m) if m is not None else None, _ptr(info), _ptr(objs), C.byref(n_o))
    if rc != GV_OK:
        raise GVError(rc, "gv_track_step")
    return buf[:n_t.value].copy(), nid.value, info[0], objs[:n_o.value].copy()


def match_rotations(cfg, guess):
    """the float32 (NT, 2) table of (cos, sin) of a MatchConfig's yaw candidates around a guess (host only)"""
    table = np.zeros((2 * MATCH_MAX_HALF + 1, 2), np.float32)
    q = _guess(guess)
    rc = load().gv_match_rotations(C.byref(cfg), C.byref(q), _ptr(table))
    if rc:
        raise GVError(rc, "gv_match_rotations")
    return table[:cfg.shape[0]].copy()


def match_motion(result):
    """the Transform (motion of grid_move and track_update) of a MATCH_RESULT_DTYPE record (host only)"""
    r = np.ascontiguousarray(result, MATCH_RESULT_DTYPE).reshape(-1)[:1]
    out = Transform()
    rc = load().gv_match_motion(_ptr(r), C.byref(out))
    if rc:
        raise GVError(rc, "gv_match_motion")
    return out


def match_scan_host(grid_x, grid_y, resolution, cost, x, y, z, base_lidar, cfg, guess, band=None, keep_scores=False):
    """gv_match_scan_host, the library's host twin of match_scan (needs no GPU): cost the uint8 costmap of G bytes in
    data order, x / y / z the lidar-frame cloud, base_lidar the seven values of base_from_lidar, band None or (z_ground,
    z_max).  Returns the MATCH_RESULT_DTYPE record, and with keep_scores also the uint32 (NT, NY, NX) volume."""
    cost = np.ascontiguousarray(cost, np.uint8).reshape(-1)
    x, y, z = _f32(x), _f32(y), _f32(z)
    tf, q = make_tf(base_lidar), _guess(guess)
    hb = HeightBand(float(band[0]), float(band[1]), 0) if band is not None else None
    res = np.zeros(1, MATCH_RESULT_DTYPE)
    vol = np.zeros(cfg.shape, np.uint32) if keep_scores else None
    rc = load().gv_match_scan_host(C.c_uint8(grid_x), C.c_uint8(grid_y), C.c_double(resolution), _ptr(cost), _ptr(x), _ptr(y),
                                   _ptr(z), C.c_size_t(len(x)), C.byref(tf), C.byref(hb) if hb is not None else None,
                                   C.byref(cfg), C.byref(q), C.c_uint32(MATCH_KEEP_SCORES if keep_scores else 0), _ptr(res),
                                   _ptr(vol))
    if rc:
        raise GVError(rc, "gv_match_scan_host")
    return (res[0], vol) if keep_scores else res[0]


def match_search_host(grid_x, grid_y, resolution, cost, x, y, z, base_lidar, cfg, guess, band=None):
    """gv_match_search_host, the library's host twin of match_search (needs no GPU), with match_scan_host's arguments and
    a SearchConfig.  Returns (the MATCH_RESULT_DTYPE record, the SEARCH_STATS_DTYPE record)."""
    cost = np.ascontiguousarray(cost, np.uint8).reshape(-1)
    x, y, z = _f32(x), _f32(y), _f32(z)
    tf, q = make_tf(base_lidar), _guess(guess)
    hb = HeightBand(float(band[0]), float(band[1]), 0) if band is not None else None
    res, stats = np.zeros(1, MATCH_RESULT_DTYPE), np.zeros(1, SEARCH_STATS_DTYPE)
    rc = load().gv_match_search_host(C.c_uint8(grid_x), C.c_uint8(grid_y), C.c_double(resolution), _ptr(cost), _ptr(x), _ptr(y),
                                     _ptr(z), C.c_size_t(len(x)), C.byref(tf), C.byref(hb) if hb is not None else None,
                                     C.byref(cfg), C.byref(q), C.c_uint32(0), _ptr(res), _ptr(stats))
    if rc:
        raise GVError(rc, "gv_match_search_host")
    return res[0], stats[0]


def _gain_entries(entries, device_ptr, n, flags):
    """(pointer, n, flags) of a gain call's candidates: a host int32 array, or a device address of n entries"""
    if device_ptr is not None:
        return C.c_void_p(device_ptr), int(n), int(flags) | GAIN_DEVICE_ENTRIES
    e = np.ascontiguousarray(entries, np.int32).reshape(-1)
    return _ptr(e), len(e), int(flags)


def _starts(starts):
    s = _f32(starts).reshape(-1, 2)
    assert len(s) >= 1, "starts is (S, 2)"
    return s


def nav_path_host(grid_x, grid_y, resolution, field, starts, cap, flags=0, keep_xy=True):
    """gv_nav_path_host, the library's host twin of nav_path (needs no GPU): field ANY uint32 array of G values in data
    order, starts (S, 2) float32 in the grid's frame.  Returns (info NAV_PATH_INFO_DTYPE (S,), entries int32 (S, cap),
    xy float32 (S, cap, 2) or None); slots past n_cells are zero."""
    field = np.ascontiguousarray(field, np.uint32).reshape(-1)
    s = _starts(starts)
    S, cap = len(s), int(cap)
    room = max(S * cap, 1) if 1 <= cap <= PATH_MAX_CAP and S * cap <= PATH_MAX_CELLS else 1
    info = np.zeros(S, NAV_PATH_INFO_DTYPE)
    entries = np.zeros(room, np.int32)
    xy = np.zeros(2 * room, np.float32) if keep_xy else None
    rc = load().gv_nav_path_host(C.c_uint8(grid_x), C.c_uint8(grid_y), C.c_double(resolution), _ptr(field), _ptr(s), C.c_int32(S),
                                 C.c_int32(cap), C.c_uint32(flags), _ptr(info), _ptr(entries), _ptr(xy))
    if rc:
        raise GVError(rc, "gv_nav_path_host")
    return info, entries.reshape(S, cap), xy.reshape(S, cap, 2) if keep_xy else None


def frontier_host(grid_x, grid_y, resolution, occ_i8, cfg, cap, flags=0, cost=None, field=None, keep_labels=True):
    """gvx_frontier_host, the library's host twin of frontier (needs no GPU): occ_i8 the packed int8 layer, cost the
    uint8 costmap (None with max_cost 256), field the uint32 distance field (None without FRONTIER_USE_FIELD), all of G
    values in data order.  Returns (info FRONTIER_INFO_DTYPE record, records FRONTIER_DTYPE (cap,), labels uint32 (G,) or
    None); records past n_written are zero."""
    occ = np.ascontiguousarray(occ_i8, np.int8).reshape(-1)
    cost = np.ascontiguousarray(cost, np.uint8).reshape(-1) if cost is not None else None
    field = np.ascontiguousarray(field, np.uint32).reshape(-1) if field is not None else None
    cap = int(cap)
    info = np.zeros(1, FRONTIER_INFO_DTYPE)
    out = np.zeros(cap if 1 <= cap <= FRONTIER_MAX_CAP else 1, FRONTIER_DTYPE)
    labels = np.zeros(len(occ), np.uint32) if keep_labels else None
    rc = load().gvx_frontier_host(C.c_uint8(grid_x), C.c_uint8(grid_y), C.c_double(resolution), _ptr(occ), _ptr(cost), _ptr(field),
                                  C.byref(cfg) if cfg is not None else None, C.c_int32(cap), C.c_uint32(flags), _ptr(info),
                                  _ptr(out), _ptr(labels))
    if rc:
        raise GVError(rc, "gvx_frontier_host")
    return info[0], out, labels


def gain_host(grid_x, grid_y, resolution, occ_i8, cfg, entries, flags=0, field=None):
    """gvx2_gain_host, the library's host twin of gain (needs no GPU): occ_i8 the packed int8 layer and field the uint32
    distance field (None without GAIN_USE_FIELD), both of G values in data order; entries int32 (n,).  Returns (info
    GAIN_INFO_DTYPE record, records GAIN_DTYPE (n,))."""
    occ = np.ascontiguousarray(occ_i8, np.int8).reshape(-1)
    field = np.ascontiguousarray(field, np.uint32).reshape(-1) if field is not None else None
    e = np.ascontiguousarray(entries, np.int32).reshape(-1)
    info = np.zeros(1, GAIN_INFO_DTYPE)
    out = np.zeros(max(len(e), 1), GAIN_DTYPE)
    rc = load().gvx2_gain_host(C.c_uint8(grid_x), C.c_uint8(grid_y), C.c_double(resolution), _ptr(occ), _ptr(field),
                               C.byref(cfg) if cfg is not None else None, C.c_int32(len(e)), _ptr(e), C.c_uint32(flags), _ptr(info),
                               _ptr(out))
    if rc:
        raise GVError(rc, "gvx2_gain_host")
    return info[0], out[:len(e)]


def shortcut_host(grid_x, grid_y, resolution, cost, cfg, src_entries, src_n, wcap, flags=0):
    """gvx3_shortcut_host, the library's host twin of shortcut (needs no GPU): cost ANY uint8 array of G values in data
    order, src_entries int32 (S, cap) and src_n int32 (S,) the paths.  Returns (info SHORTCUT_INFO_DTYPE (S,), entries int32
    (S, wcap), index int32 (S, wcap), xy float32 (S, wcap, 2)); slots past n_waypoints are zero."""
    cost = np.ascontiguousarray(cost, np.uint8).reshape(-1)
    src = np.ascontiguousarray(src_entries, np.int32)
    assert src.ndim == 2, "src_entries is (S, cap)"
    S, cap = src.shape
    n = np.ascontiguousarray(src_n, np.int32).reshape(-1)
    assert len(n) == S
    wcap = int(wcap)
    room = max(S * wcap, 1) if 1 <= wcap <= SHORTCUT_MAX_WCAP and S * wcap <= SHORTCUT_MAX_CELLS else 1
    info = np.zeros(max(S, 1), SHORTCUT_INFO_DTYPE)
    entries, index, xy = np.zeros(room, np.int32), np.zeros(room, np.int32), np.zeros(2 * room, np.float32)
    rc = load().gvx3_shortcut_host(C.c_uint8(grid_x), C.c_uint8(grid_y), C.c_double(resolution), _ptr(cost),
                                   C.byref(cfg) if cfg is not None else None, _ptr(src), _ptr(n), C.c_int32(S), C.c_int32(cap),
                                   C.c_int32(wcap), C.c_uint32(flags), _ptr(info), _ptr(entries), _ptr(index), _ptr(xy))
    if rc:
        raise GVError(rc, "gvx3_shortcut_host")
    return info[:S], entries.reshape(S, wcap), index.reshape(S, wcap), xy.reshape(S, wcap, 2)


def control_select_dyn(weights, traj, nav, dyn, cfg, keep_totals=False):
    """control_select with the DYN_SCORE_DTYPE records of a DynConfig as the third critic (cfg None: control_select)"""
    traj = np.ascontiguousarray(traj, TRAJ_SCORE_DTYPE)
    nav = np.ascontiguousarray(nav, NAV_SCORE_DTYPE) if nav is not None else None
    dyn = np.ascontiguousarray(dyn, DYN_SCORE_DTYPE) if dyn is not None else None
    assert (nav is None or len(nav) == len(traj)) and (dyn is None or len(dyn) == len(traj))
    res = np.zeros(1, CONTROL_RESULT_DTYPE)
    totals = np.zeros(max(len(traj), 1), np.uint64) if keep_totals else None
    rc = load().gv_control_select_dyn(C.byref(weights), _ptr(traj), _ptr(nav), _ptr(dyn), C.byref(cfg) if cfg is not None else None,
                                      C.c_int32(len(traj)), _ptr(res), _ptr(totals))
    if rc:
        raise GVError(rc, "gv_control_select_dyn")
    return (res[0], totals[:len(traj)]) if keep_totals else res[0]


def mppi_words(seed, iteration, k, p):
    """the four Philox4x32-10 words of pose (k, p): uint32 (4,) (host only; needs no GPU)"""
    w = np.zeros(4, np.uint32)
    rc = load().gv_mppi_words(C.c_uint64(seed), C.c_uint64(iteration), C.c_uint32(k), C.c_uint32(p), _ptr(w))
    if rc:
        raise GVError(rc, "gv_mppi_words")
    return w


def mppi_sample_controls(cfg, nominal, K, seed, iteration, shift=False):
    """the float32 (K, P, C) controls an MppiConfig samples around the float32 (P, C) nominal: the library's own arithmetic
    with the host's log, sin and cos (host only; needs no GPU)"""
    nom = _f32(nominal)
    assert nom.ndim == 2
    P, Cn = nom.shape
    out = np.zeros((K, P, Cn), np.float32)
    rc = load().gv_mppi_sample_controls(C.byref(cfg), C.c_int32(Cn), _ptr(nom), C.c_int32(K), C.c_int32(P), C.c_uint64(seed),
                                        C.c_uint64(iteration), C.c_uint32(MPPI_SHIFT if shift else 0), _ptr(out))
    if rc:
        raise GVError(rc, "gv_mppi_sample_controls")
    return out


def mppi_average(cfg, controls, totals, nominal):
    """the float32 (P, C) softmax average of float32 (K, P, C) controls over uint64 (K,) totals (UINT64_MAX: rejected),
    `nominal` when every trajectory is rejected: the sequential fp64 sums (host only; needs no GPU)"""
    u, nom = _f32(controls), _f32(nominal)
    t = np.ascontiguousarray(totals, np.uint64)
    assert u.ndim == 3 and nom.shape == u.shape[1:] and len(t) == len(u)
    out = np.zeros_like(nom)
    rc = load().gv_mppi_average(C.byref(cfg), C.c_int32(u.shape[2]), _ptr(u), _ptr(t), C.c_int32(u.shape[0]),
                                C.c_int32(u.shape[1]), _ptr(nom), _ptr(out))
    if rc:
        raise GVError(rc, "gv_mppi_average")
    return out


def mppi_constrain(limits, model, controls):
    """float32 (K, P, C) controls passed through the chain of an MppiLimits under a MotionModel (its dt and C): a new
    array, the library's own arithmetic (host only; needs no GPU)"""
    u = _f32(controls).copy()
    assert u.ndim == 3 and u.shape[2] == model.n_controls
    rc = load().gv_mppi_constrain(C.byref(limits), C.byref(model), _ptr(u), C.c_int32(u.shape[0]), C.c_int32(u.shape[1]))
    if rc:
        raise GVError(rc, "gv_mppi_constrain")
    return u


def mppi_control_costs(cfg, limits, controls, nominal, shift=False):
    """the fp64 (K,) control costs g_k of float32 (K, P, C) controls around the float32 (P, C) nominal their sampling read
    (shift: it had MPPI_SHIFT): the 64 partial sums and the tree of the header (host only; needs no GPU)"""
    u, nom = _f32(controls), _f32(nominal)
    assert u.ndim == 3 and nom.shape == u.shape[1:]
    out = np.zeros(max(u.shape[0], 1), np.float64)
    rc = load().gv_mppi_control_costs(C.byref(cfg), C.byref(limits), C.c_int32(u.shape[2]), _ptr(u), _ptr(nom),
                                      C.c_int32(u.shape[0]), C.c_int32(u.shape[1]), C.c_uint32(MPPI_SHIFT if shift else 0), _ptr(out))
    if rc:
        raise GVError(rc, "gv_mppi_control_costs")
    return out[:u.shape[0]]


def mppi_average_cc(cfg, controls, totals, control_costs, nominal):
    """mppi_average with the fp64 (K,) control costs in the exponent (None: mppi_average itself): the sequential fp64
    sums (host only; needs no GPU)"""
    u, nom = _f32(controls), _f32(nominal)
    t = np.ascontiguousarray(totals, np.uint64)
    g = np.ascontiguousarray(control_costs, np.float64) if control_costs is not None else None
    assert u.ndim == 3 and nom.shape == u.shape[1:] and len(t) == len(u) and (g is None or len(g) == len(u))
    out = np.zeros_like(nom)
    rc = load().gv_mppi_average_cc(C.byref(cfg), C.c_int32(u.shape[2]), _ptr(u), _ptr(t), _ptr(g), C.c_int32(u.shape[0]),
                                   C.c_int32(u.shape[1]), _ptr(nom), _ptr(out))
    if rc:
        raise GVError(rc, "gv_mppi_average_cc")
    return out


def shard_slice_words(words, world):
    lib = load()
    lib.gv_shard_slice_words.restype = C.c_int64
    return int(lib.gv_shard_slice_words(C.c_int64(words), C.c_int32(world)))


class PinnedF32:
    """float32 array in page-locked host memory (gv_host_alloc) for the asynchronous uploads."""

    def __init__(self, n):
        self._lib = load()
        self._p = C.c_void_p()
        rc = self._lib.gv_host_alloc(C.byref(self._p), C.c_size_t(max(int(n), 1) * 4))
        if rc:
            raise GVError(rc, "gv_host_alloc")
        self.array = np.ctypeslib.as_array(C.cast(self._p, C.POINTER(C.c_float)), shape=(int(n),))

    def close(self):
        if self._p:
            self.array = None
            self._lib.gv_host_free(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GridVisionHIP:
    """One handle = one MI355X + one stream + one resident occupancy grid."""

    def __init__(self, grid_x, grid_y, resolution, fx=320.0, fy=320.0, cx=320.0, cy=240.0,
                 image_w=640, image_h=480, network_w=224, network_h=224, device=-1):
        self._lib = load()
        self._h = C.c_void_p()
        cam = CamParams(network_h, network_w, image_h, image_w, fx, fy, cx, cy)
        rc = self._lib.gv_create(C.byref(self._h), C.c_uint8(grid_x), C.c_uint8(grid_y), C.c_double(resolution),
                                 C.byref(cam), C.c_int(device))
        if rc:
            self._h = C.c_void_p()
            raise GVError(rc, "gv_create", "(no MI355X visible: this library has no CPU path)" if rc == 4 else "")
        nx, ny = C.c_int32(), C.c_int32()
        px, py = C.c_double(), C.c_double()
        self._ck(self._lib.gv_grid_geometry(self._h, C.byref(nx), C.byref(ny), C.byref(px), C.byref(py)), "geometry")
        self.nx, self.ny, self.pos_x, self.pos_y = nx.value, ny.value, px.value, py.value
        self.G = self.nx * self.ny
        self.n = 0
        self._motion = None           # the MotionModel in force (set_motion_model)
        self._pending_controls = []   # host controls of rollout_async calls, kept alive until the stream is waited for
        self._nominal_c = 0           # controls per step of the resident MPPI nominal (mppi_set_nominal)
        self._match_cfg = None        # a copy of the MatchConfig in force (set_match_config): the volume's shape

    # ---- plumbing
    def _ck(self, rc, where):
        if rc:
            raise GVError(rc, where, (self._lib.gv_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.gv_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- setup
    def reset(self):
        self._ck(self._lib.gv_reset(self._h), "gv_reset")

    def set_transforms(self, cam_lidar=None, base_cam=None, base_lidar=None):
        a, b, c = make_tf(cam_lidar), make_tf(base_cam), make_tf(base_lidar)
        self._ck(self._lib.gv_set_transforms(self._h, C.byref(a) if a else None, C.byref(b) if b else None,
                                             C.byref(c) if c else None), "gv_set_transforms")

    def upload_xyz(self, x, y, z):
        x, y, z = _f32(x), _f32(y), _f32(z)
        self._ck(self._lib.gv_cloud_upload_xyz(self._h, _ptr(x), _ptr(y), _ptr(z), C.c_size_t(len(x))), "upload_xyz")
        self.n = len(x)

    def upload_xyz_async(self, x, y, z):
        """x, y, z: float32 arrays that stay alive and unchanged until upload_wait() (pinned: see PinnedF32)."""
        for a in (x, y, z):
            assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
        self._ck(self._lib.gv_cloud_upload_xyz_async(self._h, _ptr(x), _ptr(y), _ptr(z), C.c_size_t(len(x))),
                 "upload_xyz_async")
        self.n = len(x)

    def upload_wait(self):
        self._ck(self._lib.gv_cloud_upload_wait(self._h), "upload_wait")

    def upload_pointcloud2(self, data: np.ndarray, n, point_step, off_x, off_y, off_z):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        self._ck(self._lib.gv_cloud_upload_pointcloud2(self._h, _ptr(data), C.c_size_t(n), C.c_uint32(point_step),
                                                       C.c_uint32(off_x), C.c_uint32(off_y), C.c_uint32(off_z)),
                 "upload_pointcloud2")
        self.n = n

    def upload_pointcloud2_async(self, data: np.ndarray, n, point_step, off_x, off_y, off_z):
        """data: uint8 bytes (pinned for a truly asynchronous copy) that stay unchanged until upload_wait()"""
        assert data.dtype == np.uint8 and data.flags["C_CONTIGUOUS"] and data.size >= n * point_step
        self._ck(self._lib.gv_cloud_upload_pointcloud2_async(self._h, _ptr(data), C.c_size_t(n), C.c_uint32(point_step),
                                                             C.c_uint32(off_x), C.c_uint32(off_y), C.c_uint32(off_z)),
                 "upload_pointcloud2_async")
        self.n = n

    # ---- reference-surface calls
    def transform_lidar_to_camera(self):
        x, y, z = (np.empty(self.n, np.float32) for _ in range(3))
        self._ck(self._lib.gv_transform_lidar_to_camera(self._h, _ptr(x), _ptr(y), _ptr(z)), "transform")
        return x, y, z

    def extract_cloud_per_bbox(self, bboxes):
        b = _boxes(bboxes)
        ids = np.empty(self.n, np.int32)
        counts = np.zeros(max(len(b), 1), np.int32)
        self._ck(self._lib.gv_extract_cloud_per_bbox(self._h, _ptr(b), C.c_int32(len(b)), _ptr(ids), _ptr(counts)),
                 "extract_cloud_per_bbox")
        return ids, counts[:len(b)]

    def compute_depth_for_bboxes(self, bboxes, k):
        b = _boxes(bboxes)
        depths = np.zeros(len(b), np.float32)
        d2 = np.zeros((len(b), k), np.float32)
        self._ck(self._lib.gv_compute_depth_for_bboxes(self._h, _ptr(b), C.c_int32(len(b)), C.c_int32(k),
                                                       _ptr(depths), _ptr(d2)), "compute_depth_for_bboxes")
        return depths, d2

    def convert_pixels_to_3d(self, bboxes, depths):
        b = _boxes(bboxes)
        d = _f32(depths)
        out = np.zeros((len(b), 3), np.float64)
        self._ck(self._lib.gv_convert_pixels_to_3d(self._h, _ptr(b), _ptr(d), C.c_int32(len(b)), _ptr(out)),
                 "convert_pixels_to_3d")
        return out

    def compute_bbox_pose(self, bboxes):
        b = _boxes(bboxes)
        poses, valid = _pose_outputs(b)
        self._ck(self._lib.gv_compute_bbox_pose(self._h, _ptr(b), C.c_int32(len(b)), _ptr(poses), _ptr(valid)),
                 "compute_bbox_pose")
        return poses[:len(b)], valid[:len(b)]

    def segment_ground_plane(self, threshold=0.04, iterations=50, seed=12345):
        mask = np.zeros(max(self.n, 1), np.uint8)
        coeff = np.zeros(4, np.float32)
        m = C.c_int64(0)
        self._ck(self._lib.gv_segment_ground_plane(self._h, C.c_double(threshold), C.c_int32(iterations),
                                                   C.c_uint64(seed), _ptr(mask), _ptr(coeff), C.byref(m)),
                 "segment_ground_plane")
        return m.value, mask[:self.n], coeff

    def compute_bbox_pose_ground_removed(self, bboxes):
        b = _boxes(bboxes)
        poses, valid = _pose_outputs(b)
        npz = C.c_int32(0)
        self._ck(self._lib.gv_compute_bbox_pose_ground_removed(self._h, _ptr(b), C.c_int32(len(b)), _ptr(poses),
                                                               _ptr(valid), C.byref(npz)), "compute_bbox_pose_gr")
        return poses[:len(b)], valid[:len(b)], npz.value

    def vision_post_process(self, orient, conf, dims, bboxes):
        o, c, d = _f32(orient), _f32(conf), _f32(dims)
        b = _boxes(bboxes)
        poses, _ = _pose_outputs(b)
        m = C.c_int32(0)
        self._ck(self._lib.gv_vision_post_process(self._h, _ptr(o), _ptr(c), _ptr(d), _ptr(b), C.c_int32(len(b)),
                                                  _ptr(poses), C.byref(m)), "vision_post_process")
        return poses[:m.value].copy()

    def vision_sets(self, orient, conf, dims, bboxes):
        """test hook (csrc/gv_test_hooks.h): (nb, 64, 4) loc0, loc1, loc2, err of every constraint set of k_vision, and
        the (nb,) winner, 64 = none"""
        o, c, d = _f32(orient), _f32(conf), _f32(dims)
        b = _boxes(bboxes)
        sets = np.zeros((len(b), 64, 4), np.float32)
        winner = np.zeros(len(b), np.int32)
        self._ck(self._lib.gv_test_vision_sets(self._h, _ptr(o), _ptr(c), _ptr(d), _ptr(b), C.c_int32(len(b)),
                                               _ptr(sets), _ptr(winner)), "gv_test_vision_sets")
        return sets, winner

    def bbox_pose_nodes(self, bboxes, ground_removed=False):
        """test hook (csrc/gv_test_hooks.h): compute_bbox_pose (or compute_bbox_pose_ground_removed) and what it left on
        the device: (poses, valid, nodes, keep) -- nodes: the selected points in bucket order as a structured array
        (x, y, z float32 in the camera frame, id int32), keep: their radius-filter flags"""
        b = _boxes(bboxes)
        poses, valid = _pose_outputs(b)
        nodes = np.zeros(max(self.n, 1), dtype=NODE_DTYPE)
        keep = np.zeros(max(self.n, 1), np.uint8)
        npz, m = C.c_int32(0), C.c_int64(0)
        self._ck(self._lib.gv_test_bbox_pose_nodes(self._h, _ptr(b), C.c_int32(len(b)), C.c_int32(1 if ground_removed else 0),
                                                   _ptr(poses), _ptr(valid), C.byref(npz), _ptr(nodes), _ptr(keep),
                                                   C.byref(m)), "gv_test_bbox_pose_nodes")
        return poses[:len(b)], valid[:len(b)], nodes[:m.value].copy(), keep[:m.value].copy()

    def ransac_state(self, threshold=0.04, iterations=50, seed=12345, bboxes=None):
        """test hook (csrc/gv_test_hooks.h): segment_ground_plane (bboxes None) or compute_bbox_pose_ground_removed
        (bboxes given: its fixed 0.04 / 50 / 12345) and the RANSAC state the call brought home, as a dict: plane and
        refined (float32[4]), m, n_inliers, best_count, and mask (uint8[n]) or poses, valid, n_poses"""
        st = RansacStateOut()
        if bboxes is None:
            mask = np.zeros(max(self.n, 1), np.uint8)
            self._ck(self._lib.gv_test_ransac_state(self._h, C.c_double(threshold), C.c_int32(iterations), C.c_uint64(seed),
                                                    C.c_int32(0), None, C.c_int32(0), _ptr(mask), None, None, None,
                                                    C.byref(st)), "gv_test_ransac_state")
            out = {"mask": mask[:self.n]}
        else:
            b = _boxes(bboxes)
            poses, valid = _pose_outputs(b)
            npz = C.c_int32(0)
            self._ck(self._lib.gv_test_ransac_state(self._h, C.c_double(0.0), C.c_int32(0), C.c_uint64(0), C.c_int32(1),
                                                    _ptr(b), C.c_int32(len(b)), None, _ptr(poses), _ptr(valid),
                                                    C.byref(npz), C.byref(st)), "gv_test_ransac_state")
            out = {"poses": poses[:len(b)], "valid": valid[:len(b)], "n_poses": npz.value}
        out.update(plane=np.array(st.plane, np.float32), refined=np.array(st.refined, np.float32), m=int(st.m),
                   n_inliers=int(st.n_inliers), best_count=int(st.best_count))
        return out

    def transform_lshape_objects(self, poses):
        p = np.ascontiguousarray(poses, dtype=LSHAPE_DTYPE).copy()
        self._ck(self._lib.gv_transform_lshape_objects(self._h, _ptr(p), C.c_int32(len(p))), "transform_lshape")
        return p

    def intrinsics(self):
        k, ki = np.zeros(9), np.zeros(9)
        self._ck(self._lib.gv_get_intrinsics(self._h, _ptr(k), _ptr(ki)), "intrinsics")
        return k, ki

    def update_map(self):
        self._ck(self._lib.gv_update_map(self._h), "gv_update_map")

    def update_map_poses(self, poses):
        p = np.ascontiguousarray(poses, dtype=LSHAPE_DTYPE)
        self._ck(self._lib.gv_update_map_poses(self._h, _ptr(p), C.c_int32(len(p))), "gv_update_map_poses")

    def update_map_points(self, pts, bboxes):
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        b = np.ascontiguousarray(bboxes, dtype=BBOX_DTYPE)
        self._ck(self._lib.gv_update_map_points(self._h, _ptr(pts), _ptr(b), C.c_int32(len(b))), "update_map_points")

    def to_occupancy_grid(self):
        data = np.empty(self.G, np.int8)
        info = GridInfo()
        self._ck(self._lib.gv_to_occupancy_grid(self._h, _ptr(data), C.byref(info)), "to_occupancy_grid")
        return data, info

    def to_occupancy_grid_async(self, pinned_i8):
        """pinned_i8: int8 view of G bytes of pinned memory; complete once gv_stream has passed this point"""
        assert pinned_i8.dtype == np.int8 and pinned_i8.size == self.G
        self._ck(self._lib.gv_to_occupancy_grid_async(self._h, _ptr(pinned_i8)), "to_occupancy_grid_async")

    def publish_grid_async(self, pinned_i8):
        """the packed grid to PINNED host memory by a kernel on the public stream (the copy engines stay with the uploads)"""
        assert pinned_i8.dtype == np.int8 and pinned_i8.size == self.G
        self._ck(self._lib.gv_publish_grid_async(self._h, _ptr(pinned_i8)), "gv_publish_grid_async")

    def log_odds(self):
        out = np.empty(self.G, np.float32)
        self._ck(self._lib.gv_get_log_odds(self._h, _ptr(out)), "get_log_odds")
        return out

    def occupancy(self):
        out = np.empty(self.G, np.float32)
        self._ck(self._lib.gv_get_occupancy(self._h, _ptr(out)), "get_occupancy")
        return out

    def set_log_odds(self, a):
        a = _f32(a)
        assert a.size == self.G
        self._ck(self._lib.gv_set_log_odds(self._h, _ptr(a)), "set_log_odds")

    # ---- [EXTENSION] ego motion
    def grid_move(self, motion):
        """motion: base_prev <- base_now as a 7-vector (qx, qy, qz, qw, tx, ty, tz), like make_tf.  Asynchronous on
        stream(); returns the GridMoveInfo fields as a dict (applied as a bool)."""
        m = make_tf(motion)
        info = GridMoveInfo()
        self._ck(self._lib.gv_grid_move(self._h, C.byref(m), C.byref(info)), "gv_grid_move")
        out = {k: getattr(info, k) for k, _ in GridMoveInfo._fields_}
        out["applied"] = bool(out["applied"])
        return out

    # ---- [EXTENSION] height band of the lidar map update
    def set_height_band(self, z_ground, z_max=None, ground_clears=True):
        """base-frame z < z_ground: ground return (a free-space ray end when ground_clears), z > z_max: ignored;
        set_height_band(None) turns the band off.  Thresholds are rounded to float32 as the C struct holds them;
        ground_clears may also be an int (anything but 0 / 1 is the library's GV_ERR_BAD_ARG)."""
        if z_ground is None:
            self._ck(self._lib.gv_set_height_band(self._h, None), "gv_set_height_band")
            return
        clears = int(ground_clears) if not isinstance(ground_clears, bool) else (1 if ground_clears else 0)
        b = HeightBand(float(z_ground), float(z_max), clears)
        self._ck(self._lib.gv_set_height_band(self._h, C.byref(b)), "gv_set_height_band")

    # ---- [EXTENSION] inflated costmap layer
    def set_inflation(self, inscribed_radius, inflation_radius=None, cost_scaling_factor=10.0, lethal_threshold=65,
                      keep_dist2=False, occupancy_scale=False):
        """the configuration of the inflate() calls that follow; set_inflation(None) turns it off.  The first argument
        may also be an Inflation."""
        if inscribed_radius is None:
            self._ck(self._lib.gv_set_inflation(self._h, None), "gv_set_inflation")
            return
        cfg = inscribed_radius
        if not isinstance(cfg, Inflation):
            flags = (INFLATE_KEEP_DIST2 if keep_dist2 else 0) | (INFLATE_OCCUPANCY_SCALE if occupancy_scale else 0)
            cfg = Inflation(float(inscribed_radius), float(inflation_radius), float(cost_scaling_factor),
                            int(lethal_threshold), flags)
        self._ck(self._lib.gv_set_inflation(self._h, C.byref(cfg)), "gv_set_inflation")

    def inflate(self):
        """obstacle distance and cost of the grid as it stands, asynchronous on stream()"""
        self._ck(self._lib.gv_inflate(self._h), "gv_inflate")

    def costmap(self):
        out = np.empty(self.G, np.uint8)
        self._ck(self._lib.gv_get_costmap(self._h, _ptr(out)), "gv_get_costmap")
        return out

    def obstacle_dist2(self):
        out = np.empty(self.G, np.uint16)
        self._ck(self._lib.gv_get_obstacle_dist2(self._h, _ptr(out)), "gv_get_obstacle_dist2")
        return out

    def publish_costmap_async(self, pinned_u8):
        """the costmap to PINNED host memory (G bytes, int8 or uint8 view), like publish_grid_async"""
        assert pinned_u8.dtype in (np.int8, np.uint8) and pinned_u8.size == self.G
        self._ck(self._lib.gv_publish_costmap_async(self._h, _ptr(pinned_u8)), "gv_publish_costmap_async")

    # ---- [EXTENSION] trajectory scoring against the resident costmap
    def set_footprint(self, footprint, collision_cost=253, off_map_cost=255):
        """the footprint of the score_trajectories() calls that follow: a Footprint, or a sequence of (x, y) vertices
        (empty: the circular robot); set_footprint(None) turns it off"""
        if footprint is None:
            self._ck(self._lib.gv_set_footprint(self._h, None), "gv_set_footprint")
            return
        f = footprint if isinstance(footprint, Footprint) else Footprint.of(footprint, collision_cost, off_map_cost)
        self._ck(self._lib.gv_set_footprint(self._h, C.byref(f)), "gv_set_footprint")

    def score_trajectories_async(self, poses, K, P, scores, pose_cost=None, device_ptr=None):
        """enqueue on stream(): poses float32 (K, P, 3) host array that stays unchanged until completion (or
        device_ptr: the address of K * P * 3 floats in device memory), scores a TRAJ_SCORE_DTYPE array of K, pose_cost
        None or a uint8 array of K * P; both complete after synchronize()"""
        src, K, P, flags = _pose_batch(poses, device_ptr, K, P)
        flags |= TRAJ_KEEP_POSE_COST if pose_cost is not None else 0
        self._ck(self._lib.gv_score_trajectories_async(self._h, src, C.c_int32(K), C.c_int32(P), C.c_uint32(flags),
                                                       _ptr(scores), _ptr(pose_cost)), "gv_score_trajectories_async")

    def score_trajectories(self, poses, keep_pose_cost=False, device_ptr=None):
        """poses: float32 (K, P, 3) of (x, y, yaw) in the grid's frame (with device_ptr only its shape is used: the
        floats are read from that device address).  Returns the TRAJ_SCORE_DTYPE array of K, and with keep_pose_cost
        also the uint8 (K, P) pose costs."""
        src, K, P, flags = _pose_batch(poses, device_ptr)
        flags |= TRAJ_KEEP_POSE_COST if keep_pose_cost else 0
        scores = np.zeros(K, TRAJ_SCORE_DTYPE)
        pc = np.zeros(K * P, np.uint8) if keep_pose_cost else None
        self._ck(self._lib.gv_score_trajectories(self._h, src, C.c_int32(K), C.c_int32(P), C.c_uint32(flags), _ptr(scores),
                                                 _ptr(pc)), "gv_score_trajectories")
        return (scores, pc.reshape(K, P)) if keep_pose_cost else scores

    # ---- [EXTENSION] trajectory scoring against predicted moving objects
    def set_dyn_config(self, cfg):
        """the DynConfig of the score_dynamic() calls, control steps and MPPI updates that follow; None turns it off"""
        self._ck(self._lib.gv_set_dyn_config(self._h, C.byref(cfg) if cfg is not None else None), "gv_set_dyn_config")

    def set_moving_objects(self, objs):
        """replace the set of moving objects: a MOVING_OBJECT_DTYPE array of at most 128 (None or empty: no objects);
        ordered on stream() between the calls before and after it"""
        o = _objects(objs)
        self._ck(self._lib.gv_set_moving_objects(self._h, _ptr(o) if len(o) else None, C.c_int32(len(o))), "gv_set_moving_objects")

    def score_dynamic_async(self, poses, K, P, scores, pose_cost=None, device_ptr=None):
        """enqueue on stream(): poses as in score_trajectories_async, scores a DYN_SCORE_DTYPE array of K, pose_cost None
        or a uint8 array of K * P; both complete after synchronize()"""
        src, K, P, flags = _pose_batch(poses, device_ptr, K, P)
        flags |= TRAJ_KEEP_POSE_COST if pose_cost is not None else 0
        self._ck(self._lib.gv_score_dynamic_async(self._h, src, C.c_int32(K), C.c_int32(P), C.c_uint32(flags), _ptr(scores),
                                                  _ptr(pose_cost)), "gv_score_dynamic_async")

    def score_dynamic(self, poses, keep_pose_cost=False, device_ptr=None):
        """poses: float32 (K, P, 3) as in score_trajectories.  Returns the DYN_SCORE_DTYPE array of K, and with
        keep_pose_cost also the uint8 (K, P) pose costs."""
        src, K, P, flags = _pose_batch(poses, device_ptr)
        flags |= TRAJ_KEEP_POSE_COST if keep_pose_cost else 0
        scores = np.zeros(max(K, 1), DYN_SCORE_DTYPE)
        pc = np.zeros(max(K * P, 1), np.uint8) if keep_pose_cost else None
        self._ck(self._lib.gv_score_dynamic(self._h, src, C.c_int32(K), C.c_int32(P), C.c_uint32(flags), _ptr(scores), _ptr(pc)),
                 "gv_score_dynamic")
        return (scores[:K], pc[:K * P].reshape(K, P)) if keep_pose_cost else scores[:K]

    # ---- [EXTENSION] the tracker over the tick's boxes
    def set_track_config(self, cfg):
        """the TrackConfig of the track_update() calls that follow; None turns the tracker off and empties its tracks"""
        self._ck(self._lib.gv_set_track_config(self._h, C.byref(cfg) if cfg is not None else None), "gv_set_track_config")

    def set_tracks(self, tracks, next_id=1):
        """replace the tracker's state: a TRACK_DTYPE array of at most 128 with distinct ascending slots (None or empty:
        no tracks) and the id counter; ordered on stream() between the calls before and after it"""
        t = np.ascontiguousarray(tracks if tracks is not None else np.zeros(0, TRACK_DTYPE), TRACK_DTYPE).reshape(-1)
        self._ck(self._lib.gv_set_tracks(self._h, _ptr(t) if len(t) else None, C.c_int32(len(t)), C.c_uint32(int(next_id))),
                 "gv_set_tracks")

    def get_tracks(self):
        """(the live TRACK_DTYPE records in ascending slot order, next_id); waits for stream()"""
        out, n, nid = np.zeros(TRACK_SLOTS, TRACK_DTYPE), C.c_int32(0), C.c_uint32(0)
        self._ck(self._lib.gv_get_tracks(self._h, _ptr(out), C.c_int32(TRACK_SLOTS), C.byref(n), C.byref(nid)), "gv_get_tracks")
        return out[:n.value].copy(), nid.value

    def track_update_async(self, dets, dt, motion=None, feed=False, info=None, tracks=None, device_ptr=None, n=None, from_tick=False):
        """enqueue one update on stream(): dets an LSHAPE_DTYPE array, free on return (with
        device_ptr and n: n records at that device address), motion None, a Transform or its seven values, feed: the
        exported tracks become the moving objects of the scoring calls that follow; info None or a TRACK_INFO_DTYPE
        array of 1, tracks None or a TRACK_DTYPE array of 128, both complete after synchronize().  from_tick: the
        detections are the list of the last tick_enqueue(keep_dets=True), read on the device (dets must then be None)"""
        flags = (TRACK_FEED_DYNAMIC if feed else 0) | (TRACK_TICK_DETS if from_tick else 0)
        if device_ptr is not None:
            src, cnt, flags = C.c_void_p(int(device_ptr)), int(n), flags | TRACK_DEVICE_DETS
        else:
            assert dets is None or (dets.dtype == LSHAPE_DTYPE and dets.flags.c_contiguous)
            cnt = 0 if dets is None else len(dets)
            src = _ptr(dets) if cnt else None
        m = _motion(motion)
        self._ck(self._lib.gv_track_update_async(self._h, src, C.c_int32(cnt), C.c_double(dt), C.byref(m) if m is not None else None,
                                                 C.c_uint32(flags), _ptr(info), _ptr(tracks)), "gv_track_update_async")

    def track_update(self, dets, dt, motion=None, feed=False, from_tick=False):
        """one update, waited for: returns (info, tracks), the TRACK_INFO_DTYPE record and the live TRACK_DTYPE records.
        from_tick: as in track_update_async"""
        z, m = _detections(dets), _motion(motion)
        info, tracks = np.zeros(1, TRACK_INFO_DTYPE), np.zeros(TRACK_SLOTS, TRACK_DTYPE)
        self._ck(self._lib.gv_track_update(self._h, _ptr(z) if len(z) else None, C.c_int32(len(z)), C.c_double(dt),
                                           C.byref(m) if m is not None else None, C.c_uint32((TRACK_FEED_DYNAMIC if feed else 0) | (TRACK_TICK_DETS if from_tick else 0)),
                                           _ptr(info), _ptr(tracks)), "gv_track_update")
        return info[0], tracks[:int(info[0]["n_tracks"])].copy()

    # ---- [EXTENSION] scan-to-costmap matching
    def set_match_config(self, cfg):
        """the MatchConfig of the match_scan() calls that follow; None turns it off"""
        self._ck(self._lib.gv_set_match_config(self._h, C.byref(cfg) if cfg is not None else None), "gv_set_match_config")
        self._match_cfg = MatchConfig.from_buffer_copy(cfg) if cfg is not None else None

    def match_scan_async(self, guess, result, scores=None):
        """enqueue on stream(): guess a MatchGuess or (x, y, yaw), result a MATCH_RESULT_DTYPE array of 1, scores None
        or a uint32 array of NT * NY * NX (the whole volume is then kept); pinned arrays are written in place by the
        device; both complete after synchronize()"""
        q = _guess(guess)
        assert result.dtype == MATCH_RESULT_DTYPE and result.size >= 1
        if scores is not None:
            cfg = getattr(self, "_match_cfg", None)
            assert scores.dtype == np.uint32 and scores.flags.c_contiguous
            assert cfg is None or scores.size >= int(np.prod(cfg.shape)), "scores holds NT * NY * NX values"
        self._ck(self._lib.gv_match_scan_async(self._h, C.byref(q), C.c_uint32(MATCH_KEEP_SCORES if scores is not None else 0),
                                               _ptr(result), _ptr(scores)), "gv_match_scan_async")

    def match_scan(self, guess, keep_scores=False):
        """one match, waited for: the MATCH_RESULT_DTYPE record, and with keep_scores also the uint32 (NT, NY, NX)
        volume of every candidate's score"""
        q = _guess(guess)
        res = np.zeros(1, MATCH_RESULT_DTYPE)
        cfg = getattr(self, "_match_cfg", None)
        vol = np.zeros(cfg.shape if cfg is not None else (1, 1, 1), np.uint32) if keep_scores else None
        self._ck(self._lib.gv_match_scan(self._h, C.byref(q), C.c_uint32(MATCH_KEEP_SCORES if keep_scores else 0), _ptr(res),
                                         _ptr(vol)), "gv_match_scan")
        return (res[0], vol) if keep_scores else res[0]

    # ---- [EXTENSION] wide-window matching by branch and bound
    def set_search_config(self, cfg):
        """the SearchConfig of the match_search() calls that follow; None turns it off"""
        self._ck(self._lib.gv_set_search_config(self._h, C.byref(cfg) if cfg is not None else None), "gv_set_search_config")

    def match_search_async(self, guess, result, stats=None):
        """enqueue on stream(): guess a MatchGuess or (x, y, yaw), result a MATCH_RESULT_DTYPE array of 1, stats None or
        a SEARCH_STATS_DTYPE array of 1; pinned arrays are written in place by the device; both complete after
        synchronize()"""
        q = _guess(guess)
        assert result.dtype == MATCH_RESULT_DTYPE and result.size >= 1
        assert stats is None or (stats.dtype == SEARCH_STATS_DTYPE and stats.size >= 1)
        self._ck(self._lib.gv_match_search_async(self._h, C.byref(q), C.c_uint32(0), _ptr(result), _ptr(stats)),
                 "gv_match_search_async")

    def match_search(self, guess, keep_stats=True):
        """one search, waited for: (the MATCH_RESULT_DTYPE record, the SEARCH_STATS_DTYPE record), or the record alone"""
        q = _guess(guess)
        res = np.zeros(1, MATCH_RESULT_DTYPE)
        stats = np.zeros(1, SEARCH_STATS_DTYPE) if keep_stats else None
        self._ck(self._lib.gv_match_search(self._h, C.byref(q), C.c_uint32(0), _ptr(res), _ptr(stats)), "gv_match_search")
        return (res[0], stats[0]) if keep_stats else res[0]

    # ---- [EXTENSION] goal / path distance field over the resident costmap
    def set_nav_config(self, obstacle_cost=253, cost_weight=0):
        """the configuration of the nav_field() calls that follow: a NavConfig, or its two fields; set_nav_config(None)
        turns it off"""
        if obstacle_cost is None:
            self._ck(self._lib.gv_set_nav_config(self._h, None), "gv_set_nav_config")
            return
        cfg = obstacle_cost if isinstance(obstacle_cost, NavConfig) else NavConfig(int(obstacle_cost), int(cost_weight), 0)
        self._ck(self._lib.gv_set_nav_config(self._h, C.byref(cfg)), "gv_set_nav_config")

    def nav_field(self, seeds_xy):
        """the distance field from seeds (S, 2) float32 in the grid's frame over the costmap of the last inflate(); waits
        until the field is complete on the device.  Returns dict(n_seeds_used, rounds)."""
        s = _f32(seeds_xy).reshape(-1, 2)
        info = NavInfo()
        self._ck(self._lib.gv_nav_field(self._h, _ptr(s), C.c_int32(len(s)), C.byref(info)), "gv_nav_field")
        return dict(n_seeds_used=info.n_seeds_used, rounds=info.rounds)

    def nav_field_array(self):
        """the field of the last nav_field(): uint32 (G,) in OccupancyGrid.data order"""
        out = np.empty(self.G, np.uint32)
        self._ck(self._lib.gv_get_nav_field(self._h, _ptr(out)), "gv_get_nav_field")
        return out

    def device_nav_field(self):
        """the device address of the field's G uint32 values (read-only)"""
        p = C.c_void_p()
        self._ck(self._lib.gv_device_nav_field(self._h, C.byref(p)), "gv_device_nav_field")
        return p.value

    def score_nav_async(self, poses, K, P, scores, device_ptr=None):
        """enqueue on stream(): poses as in score_trajectories_async, scores a NAV_SCORE_DTYPE array of K; complete
        after synchronize()"""
        src, K, P, flags = _pose_batch(poses, device_ptr, K, P)
        self._ck(self._lib.gv_score_nav_async(self._h, src, C.c_int32(K), C.c_int32(P), C.c_uint32(flags), _ptr(scores)),
                 "gv_score_nav_async")

    def score_nav(self, poses, device_ptr=None):
        """poses: float32 (K, P, 3) as in score_trajectories (the yaw is never read).  Returns the NAV_SCORE_DTYPE array
        of K."""
        src, K, P, flags = _pose_batch(poses, device_ptr)
        scores = np.zeros(K, NAV_SCORE_DTYPE)
        self._ck(self._lib.gv_score_nav(self._h, src, C.c_int32(K), C.c_int32(P), C.c_uint32(flags), _ptr(scores)),
                 "gv_score_nav")
        return scores

    # ---- [EXTENSION] paths down the distance field
    def nav_path_async(self, starts, cap, info, paths_xy=None, flags=0):
        """enqueue on stream(): starts (S, 2) float32 (copied before the call returns), info a NAV_PATH_INFO_DTYPE array
        of S, paths_xy None (the paths stay resident only) or a float32 array of S * cap * 2; pinned arrays are written
        in place by the device; both complete after synchronize()"""
        s = _starts(starts)
        assert info.dtype == NAV_PATH_INFO_DTYPE and info.size >= len(s)
        assert paths_xy is None or (paths_xy.dtype == np.float32 and paths_xy.size >= len(s) * int(cap) * 2)
        self._ck(self._lib.gv_nav_path_async(self._h, _ptr(s), C.c_int32(len(s)), C.c_int32(cap), C.c_uint32(flags), _ptr(info),
                                             _ptr(paths_xy)), "gv_nav_path_async")

    def nav_path(self, starts, cap, flags=0, keep_xy=True):
        """walk the field of the last nav_field() downhill from starts (S, 2) float32, at most cap cells each, waited
        for.  Returns (info NAV_PATH_INFO_DTYPE (S,), xy float32 (S, cap, 2) or None with keep_xy=False: the paths
        then stay resident only, for nav_path_get and nav_field_from_path)."""
        s = _starts(starts)
        info = np.zeros(len(s), NAV_PATH_INFO_DTYPE)
        ok = 1 <= int(cap) <= PATH_MAX_CAP and len(s) * int(cap) <= PATH_MAX_CELLS
        xy = np.zeros((len(s), int(cap), 2) if ok else (1,), np.float32) if keep_xy else None
        self._ck(self._lib.gv_nav_path(self._h, _ptr(s), C.c_int32(len(s)), C.c_int32(cap), C.c_uint32(flags), _ptr(info),
                                       _ptr(xy)), "gv_nav_path")
        return info, xy

    def device_nav_path(self):
        """dict(entries, xy, info: device addresses; S, cap) of the resident paths (read-only)"""
        e, x, i, S, cap = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int32(), C.c_int32()
        self._ck(self._lib.gv_device_nav_path(self._h, C.byref(e), C.byref(x), C.byref(i), C.byref(S), C.byref(cap)),
                 "gv_device_nav_path")
        return dict(entries=e.value, xy=x.value, info=i.value, S=S.value, cap=cap.value)

    def nav_path_get(self, s, cap_out=None):
        """resident path s read back: (info record, entries int32 (n,), xy float32 (n, 2)), n = min(n_cells, cap_out)"""
        cap_out = self.device_nav_path()["cap"] if cap_out is None else int(cap_out)
        info = np.zeros(1, NAV_PATH_INFO_DTYPE)
        entries, xy = np.zeros(max(cap_out, 1), np.int32), np.zeros((max(cap_out, 1), 2), np.float32)
        self._ck(self._lib.gv_get_nav_path(self._h, C.c_int32(s), _ptr(entries), _ptr(xy), C.c_int32(cap_out), _ptr(info)),
                 "gv_get_nav_path")
        n = min(int(info[0]["n_cells"]), cap_out)
        return info[0], entries[:n].copy(), xy[:n].copy()

    def nav_field_from_path(self, s):
        """nav_field() seeded by every cell of resident path s, on the device.  Returns dict(n_seeds_used, rounds)."""
        info = NavInfo()
        self._ck(self._lib.gv_nav_field_from_path(self._h, C.c_int32(s), C.byref(info)), "gv_nav_field_from_path")
        return dict(n_seeds_used=info.n_seeds_used, rounds=info.rounds)

    # ---- [EXTENSION] frontier clusters of the resident grid
    def set_frontier_config(self, cfg):
        """the FrontierConfig of the frontier() calls that follow; None turns it off"""
        self._ck(self._lib.gvx_set_frontier_config(self._h, C.byref(cfg) if cfg is not None else None), "gvx_set_frontier_config")

    def frontier_async(self, cap, info, out, flags=0):
        """enqueue on stream(): info a FRONTIER_INFO_DTYPE array of 1, out a FRONTIER_DTYPE array of cap; pinned arrays
        are written in place by the device; both complete after synchronize()"""
        assert info.dtype == FRONTIER_INFO_DTYPE and info.size >= 1
        assert out.dtype == FRONTIER_DTYPE and out.size >= int(cap)
        self._ck(self._lib.gvx_frontier_async(self._h, C.c_int32(cap), C.c_uint32(flags), _ptr(info), _ptr(out)), "gvx_frontier_async")

    def frontier(self, cap, flags=0):
        """the frontier clusters of the packed layer, waited for.  Returns (info FRONTIER_INFO_DTYPE record, records
        FRONTIER_DTYPE (cap,)); the labels stay resident (frontier_labels, nav_field_from_frontier)."""
        cap = int(cap)
        info = np.zeros(1, FRONTIER_INFO_DTYPE)
        out = np.zeros(cap if 1 <= cap <= FRONTIER_MAX_CAP else 1, FRONTIER_DTYPE)
        self._ck(self._lib.gvx_frontier(self._h, C.c_int32(cap), C.c_uint32(flags), _ptr(info), _ptr(out)), "gvx_frontier")
        return info[0], out

    def frontier_labels(self):
        """the labels layer of the last frontier(): uint32 (G,) in OccupancyGrid.data order"""
        out = np.empty(self.G, np.uint32)
        self._ck(self._lib.gvx_get_frontier_labels(self._h, _ptr(out)), "gvx_get_frontier_labels")
        return out

    def device_frontier(self):
        """dict(labels, records, info: device addresses; cap) of the resident frontier (read-only)"""
        l, r, i, cap = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int32()
        self._ck(self._lib.gvx_device_frontier(self._h, C.byref(l), C.byref(r), C.byref(i), C.byref(cap)), "gvx_device_frontier")
        return dict(labels=l.value, records=r.value, info=i.value, cap=cap.value)

    def nav_field_from_frontier(self, k=-1):
        """nav_field() seeded by every cell of written cluster k (-1: of every written cluster), on the device.  Returns
        dict(n_seeds_used, rounds)."""
        info = NavInfo()
        self._ck(self._lib.gvx_nav_field_from_frontier(self._h, C.c_int32(k), C.byref(info)), "gvx_nav_field_from_frontier")
        return dict(n_seeds_used=info.n_seeds_used, rounds=info.rounds)

    # ---- [EXTENSION] information gain of exploration goals
    def set_gain_config(self, cfg):
        """the GainConfig of the gain() and frontier_gain() calls that follow; None turns it off"""
        self._ck(self._lib.gvx2_set_gain_config(self._h, C.byref(cfg) if cfg is not None else None), "gvx2_set_gain_config")

    def gain_async(self, entries, info, out, flags=0, device_ptr=None, n=None):
        """enqueue on stream(): entries int32 (n,) (copied before the call returns), or device_ptr the device address of n
        entries; info a GAIN_INFO_DTYPE array of 1, out a GAIN_DTYPE array of n; pinned arrays are written in place by
        the device; both complete after synchronize()"""
        src, n, flags = _gain_entries(entries, device_ptr, n, flags)
        assert info.dtype == GAIN_INFO_DTYPE and info.size >= 1
        assert out.dtype == GAIN_DTYPE and out.size >= n
        self._ck(self._lib.gvx2_gain_async(self._h, C.c_int32(n), src, C.c_uint32(flags), _ptr(info), _ptr(out)), "gvx2_gain_async")

    def gain(self, entries, flags=0, device_ptr=None, n=None):
        """the gain records of the candidate entries, waited for.  Returns (info GAIN_INFO_DTYPE record, records
        GAIN_DTYPE (n,)); both stay resident (device_gain, nav_field_from_gain)."""
        src, n, flags = _gain_entries(entries, device_ptr, n, flags)
        info = np.zeros(1, GAIN_INFO_DTYPE)
        out = np.zeros(n if 1 <= n <= GAIN_MAX_N else 1, GAIN_DTYPE)
        self._ck(self._lib.gvx2_gain(self._h, C.c_int32(n), src, C.c_uint32(flags), _ptr(info), _ptr(out)), "gvx2_gain")
        return info[0], out

    def frontier_gain_async(self, info, out, flags=0):
        """enqueue on stream(): the candidates are the goal cells of the resident frontier's written records; out a
        GAIN_DTYPE array of that frontier's cap"""
        assert info.dtype == GAIN_INFO_DTYPE and info.size >= 1 and out.dtype == GAIN_DTYPE
        self._ck(self._lib.gvx2_frontier_gain_async(self._h, C.c_uint32(flags), _ptr(info), _ptr(out)), "gvx2_frontier_gain_async")

    def frontier_gain(self, flags=0):
        """the gain records of the resident frontier's goal cells, waited for.  Returns (info GAIN_INFO_DTYPE record,
        records GAIN_DTYPE (cap of that frontier,)), zero records behind n_candidates."""
        info = np.zeros(1, GAIN_INFO_DTYPE)
        out = np.zeros(FRONTIER_MAX_CAP, GAIN_DTYPE)
        self._ck(self._lib.gvx2_frontier_gain(self._h, C.c_uint32(flags), _ptr(info), _ptr(out)), "gvx2_frontier_gain")
        return info[0], out[:self.device_gain()["n"]].copy()

    def device_gain(self):
        """dict(records, info: device addresses; n) of the resident gain result (read-only)"""
        r, i, n = C.c_void_p(), C.c_void_p(), C.c_int32()
        self._ck(self._lib.gvx2_device_gain(self._h, C.byref(r), C.byref(i), C.byref(n)), "gvx2_device_gain")
        return dict(records=r.value, info=i.value, n=n.value)

    def nav_field_from_gain(self, k=-1):
        """nav_field() seeded by the cell of resident gain record k (-1: of the resident best), on the device.  Returns
        dict(n_seeds_used, rounds)."""
        info = NavInfo()
        self._ck(self._lib.gvx2_nav_field_from_gain(self._h, C.c_int32(k), C.byref(info)), "gvx2_nav_field_from_gain")
        return dict(n_seeds_used=info.n_seeds_used, rounds=info.rounds)

    # ---- [EXTENSION] shortcuts and waypoints of the resident paths
    def set_shortcut_config(self, cfg):
        """the ShortcutConfig of the shortcut() calls that follow; None turns it off"""
        self._ck(self._lib.gvx3_set_shortcut_config(self._h, C.byref(cfg) if cfg is not None else None), "gvx3_set_shortcut_config")

    def shortcut_async(self, wcap, info, way_xy=None, flags=0):
        """enqueue on stream(): info a SHORTCUT_INFO_DTYPE array of S (that of the resident paths), way_xy None (the
        waypoints stay resident only) or a float32 array of S * wcap * 2; pinned arrays are written in place by the device;
        both complete after synchronize()"""
        assert info.dtype == SHORTCUT_INFO_DTYPE
        assert way_xy is None or way_xy.dtype == np.float32
        self._ck(self._lib.gvx3_shortcut_async(self._h, C.c_int32(wcap), C.c_uint32(flags), _ptr(info), _ptr(way_xy)),
                 "gvx3_shortcut_async")

    def shortcut(self, wcap, flags=0, keep_xy=True):
        """the resident paths pulled tight and thinned to at most wcap waypoints each, waited for.  Returns (info
        SHORTCUT_INFO_DTYPE (S,), xy float32 (S, wcap, 2) or None with keep_xy=False); the waypoints stay resident
        (shortcut_get, device_shortcut, nav_field_from_shortcut)."""
        wcap = int(wcap)
        S = self.device_nav_path()["S"]
        ok = 1 <= wcap <= SHORTCUT_MAX_WCAP and S * wcap <= SHORTCUT_MAX_CELLS
        info = np.zeros(S, SHORTCUT_INFO_DTYPE)
        xy = np.zeros((S, wcap, 2) if ok else (1,), np.float32) if keep_xy else None
        self._ck(self._lib.gvx3_shortcut(self._h, C.c_int32(wcap), C.c_uint32(flags), _ptr(info), _ptr(xy)), "gvx3_shortcut")
        return info, xy

    def device_shortcut(self):
        """dict(entries, index, xy, info: device addresses; S, wcap) of the resident waypoints (read-only)"""
        e, i, x, r, S, wcap = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int32(), C.c_int32()
        self._ck(self._lib.gvx3_device_shortcut(self._h, C.byref(e), C.byref(i), C.byref(x), C.byref(r), C.byref(S), C.byref(wcap)),
                 "gvx3_device_shortcut")
        return dict(entries=e.value, index=i.value, xy=x.value, info=r.value, S=S.value, wcap=wcap.value)

    def shortcut_get(self, s, cap_out=None):
        """resident shortcut s read back: (info record, entries int32 (n,), index int32 (n,), xy float32 (n, 2)),
        n = min(n_waypoints, cap_out)"""
        cap_out = self.device_shortcut()["wcap"] if cap_out is None else int(cap_out)
        info = np.zeros(1, SHORTCUT_INFO_DTYPE)
        room = max(cap_out, 1)
        entries, index, xy = np.zeros(room, np.int32), np.zeros(room, np.int32), np.zeros((room, 2), np.float32)
        self._ck(self._lib.gvx3_get_shortcut(self._h, C.c_int32(s), _ptr(entries), _ptr(index), _ptr(xy), C.c_int32(cap_out), _ptr(info)),
                 "gvx3_get_shortcut")
        n = min(int(info[0]["n_waypoints"]), cap_out)
        return info[0], entries[:n].copy(), index[:n].copy(), xy[:n].copy()

    def nav_field_from_shortcut(self, s):
        """nav_field() seeded by the written waypoints of resident shortcut s, on the device.  Returns dict(n_seeds_used,
        rounds)."""
        info = NavInfo()
        self._ck(self._lib.gvx3_nav_field_from_shortcut(self._h, C.c_int32(s), C.byref(info)), "gvx3_nav_field_from_shortcut")
        return dict(n_seeds_used=info.n_seeds_used, rounds=info.rounds)

    # ---- [EXTENSION] rollout and control step over the resident rollout
    def set_motion_model(self, model, dt=None):
        """the motion model of the rollout() calls that follow: a MotionModel, or MOTION_DIFF / MOTION_OMNI and dt;
        set_motion_model(None) turns it off"""
        if model is None:
            self._motion = None
            self._ck(self._lib.gv_set_motion_model(self._h, None), "gv_set_motion_model")
            return
        m = _motion_model(model, dt)
        self._ck(self._lib.gv_set_motion_model(self._h, C.byref(m)), "gv_set_motion_model")
        self._motion = MotionModel(m.model, m.dt, m.flags)

    def _rollout(self, fn, name, start, controls, constant, device_ptr, P):
        flags = ROLLOUT_CONSTANT if constant else 0
        if device_ptr is not None:
            shape = tuple(controls)            # with device_ptr `controls` is the shape of the device array
            src, K, flags = C.c_void_p(device_ptr), int(shape[0]), flags | ROLLOUT_DEVICE_CONTROLS
            P = int(P) if constant else int(shape[1])
        else:
            c = _f32(controls)                 # a contiguous float32 array (pinned memory, say) is used where it is
            assert c.ndim == (2 if constant else 3), "controls is (K, P, C), or (K, C) when constant"
            assert self._motion is None or c.shape[-1] == self._motion.n_controls, "the motion model takes other controls per step"
            src, K = _ptr(c), int(c.shape[0])
            P = int(P) if constant else int(c.shape[1])
            self._pending_controls.append(c)   # every call in flight keeps its own array (c may be a converted copy)
        s = (C.c_double * 3)(*[float(v) for v in start])
        self._ck(fn(self._h, s, src, C.c_int32(K), C.c_int32(P), C.c_uint32(flags)), name)
        if name == "gv_rollout" and K > 0:
            self._pending_controls.clear()     # the call waited for the stream

    def rollout(self, start, controls, constant=False, device_ptr=None, P=None):
        """roll float32 controls (K, P, C) -- or (K, C) held for P steps when constant -- out from start = (x, y, yaw)
        into the handle's resident pose buffer and wait.  device_ptr: the controls are read from that device address
        and `controls` is their shape."""
        self._rollout(self._lib.gv_rollout, "gv_rollout", start, controls, constant, device_ptr, P)

    def rollout_async(self, start, controls, constant=False, device_ptr=None, P=None):
        """rollout() enqueued on stream() without the wait.  The caller leaves host controls unchanged until completion;
        the handle keeps every such array alive until synchronize() or a synchronous rollout()."""
        self._rollout(self._lib.gv_rollout_async, "gv_rollout_async", start, controls, constant, device_ptr, P)

    def device_rollout(self):
        """(device address, K, P) of the resident rollout, for score_trajectories(..., device_ptr=) and score_nav"""
        p, K, P = C.c_void_p(), C.c_int32(), C.c_int32()
        self._ck(self._lib.gv_device_rollout(self._h, C.byref(p), C.byref(K), C.byref(P)), "gv_device_rollout")
        return p.value, K.value, P.value

    def rollout_array(self):
        """the resident rollout: float32 (K, P, 3)"""
        _, K, P = self.device_rollout()
        out = np.empty((K, P, 3), np.float32)
        self._ck(self._lib.gv_get_rollout(self._h, _ptr(out)), "gv_get_rollout")
        return out

    def control_step_async(self, weights, result, totals=None):
        """enqueue on stream(): result a CONTROL_RESULT_DTYPE array of 1, totals None or a uint64 array of K; both
        complete after synchronize()"""
        flags = CONTROL_KEEP_TOTALS if totals is not None else 0
        self._ck(self._lib.gv_control_step_async(self._h, C.byref(weights), C.c_uint32(flags), _ptr(result), _ptr(totals)),
                 "gv_control_step_async")

    def control_step(self, weights, keep_totals=False):
        """score the resident rollout against the costmap (and the distance field when a nav weight is set), combine,
        select.  Returns the CONTROL_RESULT_DTYPE record, and with keep_totals also the uint64 (K,) totals."""
        res = np.zeros(1, CONTROL_RESULT_DTYPE)
        totals = None
        if keep_totals:
            totals = np.zeros(self.device_rollout()[1], np.uint64)
        flags = CONTROL_KEEP_TOTALS if keep_totals else 0
        self._ck(self._lib.gv_control_step(self._h, C.byref(weights), C.c_uint32(flags), _ptr(res), _ptr(totals)),
                 "gv_control_step")
        return (res[0], totals) if keep_totals else res[0]

    # ---- [EXTENSION] MPPI sampling and softmax update
    def set_mppi(self, cfg):
        """the MppiConfig of the mppi_* calls that follow; set_mppi(None) turns it off"""
        self._ck(self._lib.gv_set_mppi(self._h, C.byref(cfg) if cfg is not None else None), "gv_set_mppi")

    def mppi_set_nominal(self, nominal):
        """the resident nominal sequence: float32 (P, C), C the controls per step of the motion model in force"""
        nom = _f32(nominal)
        assert nom.ndim == 2 and (self._motion is None or nom.shape[1] == self._motion.n_controls), "nominal is (P, C)"
        self._ck(self._lib.gv_mppi_set_nominal(self._h, _ptr(nom), C.c_int32(nom.shape[0])), "gv_mppi_set_nominal")
        self._nominal_c = int(nom.shape[1])

    def mppi_nominal(self):
        """the resident nominal sequence: float32 (P, C)"""
        P = C.c_int32()
        self._ck(self._lib.gv_get_mppi_nominal(self._h, None, C.byref(P)), "gv_get_mppi_nominal")
        out = np.empty((P.value, self._nominal_c), np.float32)
        self._ck(self._lib.gv_get_mppi_nominal(self._h, _ptr(out), None), "gv_get_mppi_nominal")
        return out

    def mppi_sample(self, K, seed, iteration, shift=False, wait=True):
        """sample K control sequences around the resident nominal into the handle's controls buffer (wait=False: enqueue
        on stream() only)"""
        fn, name = (self._lib.gv_mppi_sample, "gv_mppi_sample") if wait else (self._lib.gv_mppi_sample_async, "gv_mppi_sample_async")
        self._ck(fn(self._h, C.c_int32(K), C.c_uint64(seed), C.c_uint64(iteration), C.c_uint32(MPPI_SHIFT if shift else 0)), name)

    def device_controls(self):
        """(device address, K, P, C) of the sampled controls, for rollout(..., device_ptr=)"""
        p, K, P, Cn = C.c_void_p(), C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self._lib.gv_device_controls(self._h, C.byref(p), C.byref(K), C.byref(P), C.byref(Cn)), "gv_device_controls")
        return p.value, K.value, P.value, Cn.value

    def controls_array(self):
        """the sampled controls: float32 (K, P, C)"""
        _, K, P, Cn = self.device_controls()
        out = np.empty((K, P, Cn), np.float32)
        self._ck(self._lib.gv_get_controls(self._h, _ptr(out)), "gv_get_controls")
        return out

    def mppi_update_async(self, weights, result, totals=None, nominal_out=None):
        """enqueue on stream(): result a CONTROL_RESULT_DTYPE array of 1, totals None or a uint64 array of K, nominal_out
        None or a float32 array of P * C; all complete after synchronize()"""
        flags = CONTROL_KEEP_TOTALS if totals is not None else 0
        self._ck(self._lib.gv_mppi_update_async(self._h, C.byref(weights), C.c_uint32(flags), _ptr(result), _ptr(totals),
                                                _ptr(nominal_out)), "gv_mppi_update_async")

    def mppi_update(self, weights):
        """score the resident rollout as control_step does and replace the resident nominal by the softmax average of the
        sampled controls.  Returns (CONTROL_RESULT_DTYPE record, uint64 (K,) totals, float32 (P, C) new nominal)."""
        _, K, P, Cn = self.device_controls()
        res, totals, nom = np.zeros(1, CONTROL_RESULT_DTYPE), np.zeros(max(K, 1), np.uint64), np.zeros((P, Cn), np.float32)
        self._ck(self._lib.gv_mppi_update(self._h, C.byref(weights), C.c_uint32(CONTROL_KEEP_TOTALS), _ptr(res), _ptr(totals),
                                          _ptr(nom)), "gv_mppi_update")
        return res[0], totals[:K], nom

    def mppi_cycle_async(self, start, K, seed, iteration, weights, result, totals=None, nominal_out=None, shift=False):
        """mppi_sample + rollout of the sampled controls + mppi_update enqueued on stream() without a wait"""
        s = (C.c_double * 3)(*[float(v) for v in start])
        flags = CONTROL_KEEP_TOTALS if totals is not None else 0
        self._ck(self._lib.gv_mppi_cycle_async(self._h, s, C.c_int32(K), C.c_uint64(seed), C.c_uint64(iteration),
                                               C.c_uint32(MPPI_SHIFT if shift else 0), C.byref(weights), C.c_uint32(flags),
                                               _ptr(result), _ptr(totals), _ptr(nominal_out)), "gv_mppi_cycle_async")

    def mppi_cycle(self, start, K, seed, iteration, weights, shift=False):
        """one MPPI iteration from the resident nominal to the next one, and the wait.  Returns (CONTROL_RESULT_DTYPE
        record, uint64 (K,) totals, float32 (P, C) new nominal)."""
        P = C.c_int32()
        self._ck(self._lib.gv_get_mppi_nominal(self._h, None, C.byref(P)), "gv_get_mppi_nominal")
        res, totals = np.zeros(1, CONTROL_RESULT_DTYPE), np.zeros(max(K, 1), np.uint64)
        nom = np.zeros((P.value, self._nominal_c), np.float32)
        s = (C.c_double * 3)(*[float(v) for v in start])
        self._ck(self._lib.gv_mppi_cycle(self._h, s, C.c_int32(K), C.c_uint64(seed), C.c_uint64(iteration),
                                         C.c_uint32(MPPI_SHIFT if shift else 0), C.byref(weights), C.c_uint32(CONTROL_KEEP_TOTALS),
                                         _ptr(res), _ptr(totals), _ptr(nom)), "gv_mppi_cycle")
        return res[0], totals[:K], nom

    def set_mppi_limits(self, limits):
        """the MppiLimits of the mppi_* calls that follow; set_mppi_limits(None) turns them off"""
        self._ck(self._lib.gv_set_mppi_limits(self._h, C.byref(limits) if limits is not None else None), "gv_set_mppi_limits")

    def mppi_control_costs(self):
        """the fp64 (K,) control costs g_k of the last mppi_update / mppi_cycle that ran with gamma > 0"""
        out = np.zeros(max(self.device_controls()[1], 1), np.float64)
        self._ck(self._lib.gv_get_mppi_control_costs(self._h, _ptr(out)), "gv_get_mppi_control_costs")
        return out[:self.device_controls()[1]]

    # ---- fused frame
    def _desc(self, flags, bboxes=None, poses=None, net=None):
        self._keep = []
        d = FrameDesc()
        d.flags = flags
        if bboxes is not None and len(bboxes):
            b = np.ascontiguousarray(bboxes, dtype=BBOX_DTYPE)
            self._keep.append(b)
            d.bboxes, d.n_bboxes = b.ctypes.data, len(b)
        if poses is not None and len(poses):
            p = np.ascontiguousarray(poses, dtype=LSHAPE_DTYPE)
            self._keep.append(p)
            d.poses, d.n_poses = p.ctypes.data, len(p)
        if net is not None:
            o, c, dm = (_f32(t) for t in net)
            self._keep += [o, c, dm]
            d.orient, d.conf, d.dims = o.ctypes.data, c.ctypes.data, dm.ctypes.data
        return d

    def set_detections(self, flags, bboxes=None, poses=None, net=None):
        d = self._desc(flags, bboxes, poses, net)
        self._ck(self._lib.gv_frame_set_detections(self._h, C.byref(d)), "frame_set_detections")

    def set_detections_async(self, flags, bboxes=None, poses=None, net=None):
        d = self._desc(flags, bboxes, poses, net)
        self._ck(self._lib.gv_frame_set_detections_async(self._h, C.byref(d)), "frame_set_detections_async")

    def frame_fence(self):
        self._ck(self._lib.gv_frame_fence(self._h), "frame_fence")

    def stream(self):
        return self._lib.gv_stream(self._h)

    def device_layers(self):
        """device addresses (ints) of occ_i8, log_odds, occupancy"""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._ck(self._lib.gv_device_layers(self._h, C.byref(a), C.byref(b), C.byref(c)), "device_layers")
        return a.value, b.value, c.value

    def enqueue_frame(self):
        self._ck(self._lib.gv_frame_enqueue(self._h), "frame_enqueue")

    def synchronize(self):
        self._ck(self._lib.gv_synchronize(self._h), "synchronize")
        self._pending_controls.clear()

    def process_frame(self, flags, bboxes=None, poses=None, net=None):
        d = self._desc(flags, bboxes, poses, net)
        self._ck(self._lib.gv_process_frame(self._h, C.byref(d)), "process_frame")

    def hits(self):
        out = np.empty(self.G, np.int32)
        self._ck(self._lib.gv_get_hits(self._h, _ptr(out)), "get_hits")
        return out

    def miss(self):
        out = np.empty(self.G, np.int32)
        self._ck(self._lib.gv_get_miss(self._h, _ptr(out)), "get_miss")
        return out

    def cell_idx(self):
        out = np.empty(self.n, np.int32)
        self._ck(self._lib.gv_get_cell_idx(self._h, _ptr(out)), "get_cell_idx")
        return out

    def bbox_id(self):
        out = np.empty(self.n, np.int32)
        self._ck(self._lib.gv_get_bbox_id(self._h, _ptr(out)), "get_bbox_id")
        return out

    def ray_stats(self):
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._ck(self._lib.gv_get_ray_stats(self._h, C.byref(a), C.byref(b)), "ray_stats")
        return a.value, b.value

    # ---- the node's tick (timerCallback from filterBBoxes on, one host wait)
    def tick_enqueue(self, bboxes, k_near=4, net=None, vision=False, lidar_bin=False, lidar_raymarch=False, grid_out=None,
                     keep_dets=False):
        """net: (orient, conf, dims) of the DYNAMIC boxes in filter_bboxes order (vision=True); grid_out: PinnedI8 array;
        keep_dets: the tick leaves its detection list on the device for track_update*(from_tick=True)"""
        b = np.ascontiguousarray(bboxes if bboxes is not None else np.zeros(0, BBOX_DTYPE), dtype=BBOX_DTYPE)
        d = TickDesc()
        d.flags = (TICK_VISION_ORIENT if vision else 0) | (TICK_LIDAR_BIN if lidar_bin else 0) | (TICK_LIDAR_RAYMARCH if lidar_raymarch else 0)
        d.flags |= TICK_KEEP_DETS if keep_dets else 0
        d.bboxes, d.n_bboxes = (b.ctypes.data if len(b) else None), len(b)
        keep = [b]
        if net is not None:
            o, c, dm = (_f32(t) for t in net)
            keep += [o, c, dm]
            d.orient, d.conf, d.dims, d.n_net = o.ctypes.data, c.ctypes.data, dm.ctypes.data, len(o.reshape(-1, 4))
        d.k_near = k_near
        if grid_out is not None:
            assert grid_out.dtype == np.int8 and grid_out.size == self.G
            d.grid_out = grid_out.ctypes.data
        self._tick_keep = keep
        self._tick_nb = len(b)
        self._ck(self._lib.gv_tick_enqueue(self._h, C.byref(d)), "gv_tick_enqueue")

    def tick_wait(self):
        nb = max(self._tick_nb, 1)
        st = np.zeros(nb, dtype=BBOX_DTYPE)
        depths = np.zeros(nb, np.float32)
        pts = np.zeros((nb, 3), np.float64)
        poses = np.zeros(nb, dtype=LSHAPE_DTYPE)
        r = TickResult()
        r.static_bboxes, r.depths, r.base_points_xyz, r.poses = st.ctypes.data, depths.ctypes.data, pts.ctypes.data, poses.ctypes.data
        self._ck(self._lib.gv_tick_wait(self._h, C.byref(r)), "gv_tick_wait")
        return {"n_static": r.n_static, "n_dynamic": r.n_dynamic, "static_bboxes": st[:r.n_static], "depths": depths[:r.n_static],
                "base_points": pts[:r.n_static], "poses": poses[:r.n_poses], "pca_empty": bool(r.pca_empty)}

    def tick(self, bboxes, **kw):
        self.tick_enqueue(bboxes, **kw)
        return self.tick_wait()

    def tick_dets(self):
        """test hook (csrc/gv_test_hooks.h): (the 128 records, n, n_total) of the detection list the last
        tick_enqueue(keep_dets=True) left on the device; waits for stream()"""
        out, n, nt = np.zeros(TICK_DETS, LSHAPE_DTYPE), C.c_int32(-1), C.c_int32(-1)
        self._ck(self._lib.gv_test_tick_dets(self._h, _ptr(out), C.byref(n), C.byref(nt)), "gv_test_tick_dets")
        return out, n.value, nt.value

    def test_end_bitmaps(self):
        """test hook (csrc/gv_test_hooks.h): the raw words of the four end bitmaps the tile pass of the last synchronous
        process_frame wrote, and their geometry: (hitN, clipN, hitT, clipT, (nxw, nyw, nx_pad, ny_pad)).  N arrays hold
        nxw * ny_pad words, T arrays nyw * nx_pad; decoding them is the caller's business."""
        g = [C.c_int32() for _ in range(4)]
        self._ck(self._lib.gv_test_end_bitmaps(self._h, None, None, None, None, *[C.byref(v) for v in g]), "gv_test_end_bitmaps")
        nxw, nyw, nx_pad, ny_pad = (v.value for v in g)
        hn, cn = np.empty(nxw * ny_pad, np.uint32), np.empty(nxw * ny_pad, np.uint32)
        ht, ct = np.empty(nyw * nx_pad, np.uint32), np.empty(nyw * nx_pad, np.uint32)
        self._ck(self._lib.gv_test_end_bitmaps(self._h, _ptr(hn), _ptr(cn), _ptr(ht), _ptr(ct), *[C.byref(v) for v in g]),
                 "gv_test_end_bitmaps")
        return hn, cn, ht, ct, (nxw, nyw, nx_pad, ny_pad)

    def test_wave(self, op, values, active=None, arg=0, threads=256):
        """test hook (csrc/gv_test_hooks.h): helper `op` (a name of WAVE_OPS or its number) of csrc/gv_wave.hpp over
        `values`, (n_waves, 64) uint64, under the lane masks `active` ((n_waves,) uint64; None: every lane).  Returns
        (out (n_waves, 64) uint64, the append counter's final value)."""
        v = np.ascontiguousarray(values, dtype=np.uint64)
        assert v.ndim == 2 and v.shape[1] == 64
        a = np.full(len(v), WAVE_ALL_LANES, np.uint64) if active is None else np.ascontiguousarray(active, dtype=np.uint64)
        assert a.shape == (len(v),)
        out, counter = np.zeros(v.shape, np.uint64), C.c_uint32(0xFFFFFFFF)
        self._ck(self._lib.gv_test_wave(self._h, C.c_int32(WAVE_OPS.index(op) if isinstance(op, str) else op), C.c_int32(arg),
                                        C.c_int32(threads), _ptr(v), _ptr(a), C.c_int64(len(v)), _ptr(out), C.byref(counter)),
                 "gv_test_wave")
        return out, counter.value

    # ---- multi-GPU (RCCL inside the library)
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        rc = load().gv_comm_unique_id(buf)
        if rc:
            raise GVError(rc, "gv_comm_unique_id")
        return bytes(buf)

    def comm_init(self, uid: bytes, rank: int, world: int):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._ck(self._lib.gv_comm_init(self._h, buf, C.c_int32(rank), C.c_int32(world)), "gv_comm_init")

    def comm_info(self):
        """(ranks in the communicator, this rank, its device) as RCCL reports them"""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self._lib.gv_comm_info(self._h, C.byref(a), C.byref(b), C.byref(c)), "gv_comm_info")
        return a.value, b.value, c.value

    def comm_destroy(self):
        self._ck(self._lib.gv_comm_destroy(self._h), "gv_comm_destroy")

    def comm_band(self):
        b, e = C.c_int64(), C.c_int64()
        self._ck(self._lib.gv_comm_band(self._h, C.byref(b), C.byref(e)), "gv_comm_band")
        return b.value, e.value

    def enqueue_frame_sharded(self):
        self._ck(self._lib.gv_frame_enqueue_sharded(self._h), "frame_enqueue_sharded")

    def time_frame_sharded_stages(self, frames):
        ms = (C.c_float * 6)()
        self._ck(self._lib.gv_time_frame_sharded_stages(self._h, C.c_int32(frames), ms), "time_frame_sharded_stages")
        return dict(zip(("bin", "exchange_ends", "sectors", "exchange_free", "grid_pass", "gather"), [float(v) for v in ms]))

    def process_frame_sharded(self, flags, bboxes=None, poses=None, net=None):
        d = self._desc(flags, bboxes, poses, net)
        self._ck(self._lib.gv_process_frame_sharded(self._h, C.byref(d)), "process_frame_sharded")

    def frame_sharded_emulated(self, world, flags, bboxes=None, poses=None, net=None):
        d = self._desc(flags, bboxes, poses, net)
        self._ck(self._lib.gv_test_frame_sharded_emulated(self._h, C.byref(d), C.c_int32(world)), "frame_sharded_emulated")

    def time_frames(self, frames):
        ms = C.c_float(0)
        self._ck(self._lib.gv_time_frames(self._h, C.c_int32(frames), C.byref(ms)), "time_frames")
        return ms.value

    def time_frame_stages(self, frames):
        ms = (C.c_float * len(STAGES))()
        self._ck(self._lib.gv_time_frame_stages(self._h, C.c_int32(frames), ms), "time_frame_stages")
        return dict(zip(STAGES, [float(v) for v in ms]))
