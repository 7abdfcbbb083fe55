"""ctypes binding of libfxjps.so (include/fxjps.h).  No CPU fallback: if the HIP
library cannot be loaded, or no MI355X is visible, every entry point raises."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# FXJPS_LIB: bring-up override (e.g. the traced build); the package default is the in-tree library
LIB_PATH = os.environ.get("FXJPS_LIB") or os.path.join(_HERE, "libfxjps.so")

OK = 0
E_ARG, E_NODEV, E_HIP, E_NOGRID, E_NOMEM, E_COMM = -1, -2, -3, -4, -5, -6
Q_NOPATH, Q_PATH_TOO_LONG, Q_BAD_START, Q_CAPACITY = 0, -1, -2, -3
BACKEND_HIP = 1

# every symbol include/fxjps.h declares (tests check the .so exports all of them)
VERSION = 880  # FXJPS_VERSION of include/fxjps.h
PATH_VALID, PATH_EMPTY, PATH_BLOCKED, PATH_OUTSIDE, PATH_MALFORMED = 1, 0, 2, 3, -1  # FXJPS_PATH_*: fxjps_check_path's verdicts
SYMBOLS = ("fxjps_version", "fxjps_timing_size", "fxjps_last_timing_sized", "fxjps_rank_preflight", "fxjps_reserve_grid",
           "fxjps_device_count", "fxjps_create", "fxjps_rank_unique_id", "fxjps_create_rank", "fxjps_set_grid_rank", "fxjps_destroy", "fxjps_last_error",
           "fxjps_set_grid", "fxjps_set_grid_device", "fxjps_prepare_grid", "fxjps_prepare_occupancy_msg", "fxjps_get_grid", "fxjps_get_grid_context", "fxjps_publish_map", "fxjps_set_grid_image", "fxjps_snapshot_image", "fxjps_update_cells", "fxjps_update_cells_deferred", "fxjps_set_queries", "fxjps_replan_frame", "fxjps_plan_batch",
           "fxjps_plan_batch_csr", "fxjps_last_cells", "fxjps_last_timing", "fxjps_last_timing_device", "fxjps_comm_info", "fxjps_set_memory_share", "fxjps_selftest_sqrt", "fxjps_selftest_wavemin", "fxjps_selftest_openlist", "fxjps_debug_read_nbmask", "fxjps_debug_read_maps", "fxjps_debug_counters", "fxjps_debug_qstat",
           "fxjps_waypoint_st", "fxjps_waypoint_ccst", "fxjps_waypoint_ccst_batch", "fxjps_waypoint_st_batch",
           "fxjps_set_grid_slot", "fxjps_get_grid_slot", "fxjps_plan_batch_slots_csr", "fxjps_debug_read_slot_maps", "fxjps_debug_read_sets", "fxjps_debug_live_bytes",
           "fxjps_prepare_slots", "fxjps_slot_job_size", "fxjps_waypoint_slots_batch", "fxjps_publish_slots", "fxjps_slot_publish_size",
           "fxjps_tick_outputs_slots", "fxjps_refresh_slots", "fxjps_debug_read_slot_context", "fxjps_replan_slots",
           "fxjps_set_prior_map", "fxjps_get_prior_map", "fxjps_prepare_slots_world", "fxjps_refresh_slots_world", "fxjps_world_job_size",
           "fxjps_prepare_slots_cropped", "fxjps_refresh_slots_cropped", "fxjps_crop_size",
           "fxjps_refresh_grid", "fxjps_refresh_occupancy_msg", "fxjps_last_refresh_cells", "fxjps_replan_frame_raw",
           "fxjps_set_grid_slots", "fxjps_refresh_grid_slots", "fxjps_grid_job_size",
           "fxjps_set_slot_reuse", "fxjps_debug_slot_tiles", "fxjps_debug_slot_read_sets",
           "fxjps_check_path", "fxjps_check_paths_slots",
           "fxjps_absorb_prior", "fxjps_absorb_check", "fxjps_absorb_job_size",
           "fxjps_absorb_prior_grow", "fxjps_grow_check", "fxjps_grow_job_size", "fxjps_prior_grown_size",
           "fxjps_absorb_prior_slide", "fxjps_slide_check", "fxjps_prior_keep_size", "fxjps_prior_slid_size")
MAX_GRID_SLOTS = 256  # FXJPS_MAX_GRID_SLOTS
MAX_PRIOR_MAPS = 16  # FXJPS_MAX_PRIOR_MAPS
ABSORB_OVERWRITE, ABSORB_OCCUPIED, ABSORB_KNOWN = 0, 1, 2  # FXJPS_ABSORB_*: fxjps_absorb_prior's modes
ABSORB_MODES = {"overwrite": ABSORB_OVERWRITE, "occupied": ABSORB_OCCUPIED, "known": ABSORB_KNOWN}
KEEP_NONE, KEEP_ALWAYS, KEEP_OVER_LIMIT = 0, 1, 2  # FXJPS_KEEP_*: how fxjps_absorb_prior_slide uses a prior's keep window
KEEP_USES = {"none": KEEP_NONE, "always": KEEP_ALWAYS, "over_limit": KEEP_OVER_LIMIT}
JOB_NOT_PLANNED = 1  # FXJPS_JOB_NOT_PLANNED: a job's status from the cropped calls, the node does not plan on this tick


class Timing(C.Structure):
    _fields_ = [("search_kernel_ms", C.c_double), ("total_ms", C.c_double), ("search_launches", C.c_int64),
                ("retried", C.c_int64), ("pops", C.c_int64), ("pushes", C.c_int64), ("far_refills", C.c_int64),
                ("slow_pops", C.c_int64), ("table_wipes", C.c_int64), ("reused", C.c_int64), ("table_direct", C.c_int64),
                ("waves", C.c_int64), ("waves_short", C.c_int64), ("head_launch_ms", C.c_double), ("batch_launch_ms", C.c_double),
                ("solo_timeouts", C.c_int64), ("host_tail_queries", C.c_int64), ("host_tail_ms", C.c_double),
                ("host_tail_late", C.c_int64)]


class SlotJob(C.Structure):
    """fxjps_slot_job_t: one vehicle's raw map on its way into a grid slot (fxjps_prepare_slots)."""
    _fields_ = [("raw", C.c_void_p), ("slot", C.c_int32), ("layout", C.c_int32), ("W0", C.c_int32), ("H0", C.c_int32),
                ("ifa", C.c_int32), ("variant", C.c_int32), ("start_xy", C.c_int32 * 2), ("goal_xy", C.c_int32 * 2),
                ("W", C.c_int32), ("H", C.c_int32), ("map_d", C.c_int32 * 2), ("end_occu", C.c_int32), ("status", C.c_int32)]


class GridJob(C.Structure):
    """fxjps_grid_job_t: one prepared grid on its way into a grid slot (fxjps_set_grid_slots)."""
    _fields_ = [("occ", C.POINTER(C.c_uint8)), ("slot", C.c_int32), ("W", C.c_int32), ("H", C.c_int32), ("reserved", C.c_int32)]


class WorldJob(C.Structure):
    """fxjps_world_job_t: one vehicle's detected map, position and goal in the world frame on their way into a grid slot
    (fxjps_prepare_slots_world)."""
    _fields_ = [("raw", C.c_void_p), ("slot", C.c_int32), ("layout", C.c_int32), ("W0", C.c_int32), ("H0", C.c_int32),
                ("ifa", C.c_int32), ("variant", C.c_int32), ("prior", C.c_int32), ("status", C.c_int32),
                ("map_o", C.c_double * 2), ("map_t", C.c_double * 2), ("map_reso", C.c_double), ("pos_xy", C.c_double * 2),
                ("goal_xy", C.c_double * 2), ("ori_pre", C.c_double * 2), ("canvas_o", C.c_double * 2), ("origin", C.c_double * 2),
                ("start_xy", C.c_int32 * 2), ("goal_xy_cell", C.c_int32 * 2), ("W", C.c_int32), ("H", C.c_int32),
                ("map_d", C.c_int32 * 2), ("end_occu", C.c_int32), ("canvas_W", C.c_int32), ("canvas_H", C.c_int32),
                ("reserved_", C.c_int32)]


class Crop(C.Structure):
    """fxjps_crop_t: what remove_zero_rowscols (global_planner_ccst.py:36-63) makes of one map message
    (fxjps_prepare_slots_cropped)."""
    _fields_ = [("bbox", C.c_int32 * 4), ("start0", C.c_int32 * 2), ("lo", C.c_int32 * 2), ("win", C.c_int32 * 2),
                ("map_o", C.c_double * 2), ("map_t", C.c_double * 2)]


class AbsorbJob(C.Structure):
    """fxjps_absorb_job_t: one vehicle's detected rectangle on its way into a prior map (fxjps_absorb_prior)."""
    _fields_ = [("raw", C.c_void_p), ("layout", C.c_int32), ("W0", C.c_int32), ("H0", C.c_int32), ("lo", C.c_int32 * 2),
                ("win", C.c_int32 * 2), ("prior", C.c_int32), ("reserved_", C.c_int32), ("map_o", C.c_double * 2),
                ("map_reso", C.c_double), ("ori_pre", C.c_double * 2), ("inside", C.c_int64), ("outside", C.c_int64)]


class GrowJob(C.Structure):
    """fxjps_grow_job_t: fxjps_absorb_job_t's fields, then the rectangle's top and where it landed in the grown prior
    (fxjps_absorb_prior_grow)."""
    _fields_ = AbsorbJob._fields_ + [("map_t", C.c_double * 2), ("at", C.c_int32 * 2)]


class PriorGrown(C.Structure):
    """fxjps_prior_grown_t: what fxjps_absorb_prior_grow made of one prior map."""
    _fields_ = [("named", C.c_int32), ("W", C.c_int32), ("H", C.c_int32), ("shift", C.c_int32 * 2), ("reserved_", C.c_int32),
                ("origin", C.c_double * 2), ("changed", C.c_int64)]


class PriorKeep(C.Structure):
    """fxjps_prior_keep_t: one prior's keep window, world metres (fxjps_absorb_prior_slide)."""
    _fields_ = [("use", C.c_int32), ("reserved_", C.c_int32), ("lo", C.c_double * 2), ("hi", C.c_double * 2)]


class PriorSlid(C.Structure):
    """fxjps_prior_slid_t: what fxjps_absorb_prior_slide made of one prior map: fxjps_prior_grown_t's fields, `trimmed`
    where that one has its reserved word, then what was cut."""
    _fields_ = [("trimmed", C.c_int32) if f[0] == "reserved_" else f for f in PriorGrown._fields_] + \
        [("grown_wh", C.c_int32 * 2), ("cut_lo", C.c_int32 * 2), ("cut_hi", C.c_int32 * 2)]


class SlotPublish(C.Structure):
    """fxjps_slot_publish_t: one slot's map on its way out as a message and / or a snapshot image (fxjps_publish_slots)."""
    _fields_ = [("msg_data", C.c_void_p), ("image", C.c_void_p), ("slot", C.c_int32), ("channels", C.c_int32), ("W", C.c_int32),
                ("H", C.c_int32)]


class FxjpsError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "fxjps error %d: %s" % (code, msg))
        self.code = code


_lib = None


def bind_host(L):
    """Prototypes of the host-only entry points (csrc/fxjps_waypoints.cpp); also used on the sanitizer build of that
    translation unit by the CPU test-suite."""
    p_i32 = C.POINTER(C.c_int32)
    p_u8 = C.POINTER(C.c_uint8)
    p_f64 = C.POINTER(C.c_double)
    L.fxjps_waypoint_st.restype = C.c_int
    L.fxjps_waypoint_st.argtypes = [p_i32, C.c_int32, p_i32, C.c_double, p_f64, p_f64, p_f64, C.c_int32, C.c_double, C.c_double,
                                    p_f64, C.c_int32, p_f64, p_i32, p_f64, p_f64]
    L.fxjps_waypoint_ccst.restype = C.c_int
    L.fxjps_waypoint_ccst.argtypes = [p_i32, C.c_int32, p_u8, C.c_int32, C.c_int32, C.c_double, p_f64, p_f64, p_f64, C.c_int32, p_f64, p_f64,
                                      p_i32, p_i32]
    L.fxjps_check_path.restype = C.c_int
    L.fxjps_check_path.argtypes = [p_i32, C.c_int32, p_u8, C.c_int32, C.c_int32, p_i32, p_i32, p_i32, p_i32]
    return L


def load():
    """Load libfxjps.so; raises (loudly) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FxjpsError(E_NODEV, "%s is missing: build it with `make -C %s` (hipcc, gfx950); "
                         "there is no CPU fallback" % (LIB_PATH, _HERE))
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    p_i32 = C.POINTER(C.c_int32)
    p_i64 = C.POINTER(C.c_int64)
    p_u8 = C.POINTER(C.c_uint8)
    p_f64 = C.POINTER(C.c_double)
    L.fxjps_version.restype = C.c_int
    L.fxjps_timing_size.restype = C.c_int
    # (neither call touches a device)
    if L.fxjps_version() != VERSION or L.fxjps_timing_size() != C.sizeof(Timing):
        raise FxjpsError(E_ARG, "%s is version %d with a %d-byte timing record; this binding is for version %d / %d bytes: rebuild it"
                         % (LIB_PATH, L.fxjps_version(), L.fxjps_timing_size(), VERSION, C.sizeof(Timing)))
    L.fxjps_slot_job_size.restype = C.c_int
    if L.fxjps_slot_job_size() != C.sizeof(SlotJob):
        raise FxjpsError(E_ARG, "%s has a %d-byte slot job; this binding's is %d bytes: rebuild it" % (LIB_PATH, L.fxjps_slot_job_size(), C.sizeof(SlotJob)))
    L.fxjps_grid_job_size.restype = C.c_int
    if L.fxjps_grid_job_size() != C.sizeof(GridJob):
        raise FxjpsError(E_ARG, "%s has a %d-byte grid job; this binding's is %d bytes: rebuild it" % (LIB_PATH, L.fxjps_grid_job_size(), C.sizeof(GridJob)))
    L.fxjps_slot_publish_size.restype = C.c_int
    if L.fxjps_slot_publish_size() != C.sizeof(SlotPublish):
        raise FxjpsError(E_ARG, "%s has a %d-byte slot publish job; this binding's is %d bytes: rebuild it"
                         % (LIB_PATH, L.fxjps_slot_publish_size(), C.sizeof(SlotPublish)))
    L.fxjps_world_job_size.restype = C.c_int
    if L.fxjps_world_job_size() != C.sizeof(WorldJob):
        raise FxjpsError(E_ARG, "%s has a %d-byte world job; this binding's is %d bytes: rebuild it"
                         % (LIB_PATH, L.fxjps_world_job_size(), C.sizeof(WorldJob)))
    L.fxjps_crop_size.restype = C.c_int
    if L.fxjps_crop_size() != C.sizeof(Crop):
        raise FxjpsError(E_ARG, "%s has a %d-byte crop record; this binding's is %d bytes: rebuild it" % (LIB_PATH, L.fxjps_crop_size(), C.sizeof(Crop)))
    L.fxjps_absorb_job_size.restype = C.c_int
    if L.fxjps_absorb_job_size() != C.sizeof(AbsorbJob):
        raise FxjpsError(E_ARG, "%s has a %d-byte absorb job; this binding's is %d bytes: rebuild it"
                         % (LIB_PATH, L.fxjps_absorb_job_size(), C.sizeof(AbsorbJob)))
    L.fxjps_grow_job_size.restype = C.c_int
    L.fxjps_prior_grown_size.restype = C.c_int
    if L.fxjps_grow_job_size() != C.sizeof(GrowJob) or L.fxjps_prior_grown_size() != C.sizeof(PriorGrown):
        raise FxjpsError(E_ARG, "%s has a %d-byte grow job and a %d-byte grown-prior record; this binding's are %d and %d bytes: rebuild it"
                         % (LIB_PATH, L.fxjps_grow_job_size(), L.fxjps_prior_grown_size(), C.sizeof(GrowJob), C.sizeof(PriorGrown)))
    L.fxjps_prior_keep_size.restype = C.c_int
    L.fxjps_prior_slid_size.restype = C.c_int
    if L.fxjps_prior_keep_size() != C.sizeof(PriorKeep) or L.fxjps_prior_slid_size() != C.sizeof(PriorSlid):
        raise FxjpsError(E_ARG, "%s has a %d-byte keep window and a %d-byte slid-prior record; this binding's are %d and %d bytes: rebuild it"
                         % (LIB_PATH, L.fxjps_prior_keep_size(), L.fxjps_prior_slid_size(), C.sizeof(PriorKeep), C.sizeof(PriorSlid)))
    L.fxjps_last_timing_sized.restype = C.c_int
    L.fxjps_last_timing_sized.argtypes = [vp, vp, C.c_int64]
    L.fxjps_rank_preflight.restype = C.c_int
    L.fxjps_rank_preflight.argtypes = [C.c_int]
    L.fxjps_reserve_grid.restype = C.c_int
    L.fxjps_reserve_grid.argtypes = [vp, C.c_int32, C.c_int32]
    L.fxjps_device_count.restype = C.c_int
    L.fxjps_create.restype = C.c_int
    L.fxjps_create.argtypes = [C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
    L.fxjps_destroy.restype = None
    L.fxjps_destroy.argtypes = [vp]
    L.fxjps_last_error.restype = C.c_char_p
    L.fxjps_last_error.argtypes = [vp]
    L.fxjps_set_grid.restype = C.c_int
    L.fxjps_set_grid.argtypes = [vp, p_u8, C.c_int32, C.c_int32]
    L.fxjps_set_grid_device.restype = C.c_int
    L.fxjps_set_grid_device.argtypes = [vp, vp, C.c_int32, C.c_int32]
    L.fxjps_prepare_grid.restype = C.c_int
    L.fxjps_prepare_grid.argtypes = [vp, p_u8, C.c_int32, C.c_int32, C.c_int32, C.c_int32, p_i32, p_i32, p_i32, p_i32, p_i32, p_i32]
    L.fxjps_prepare_occupancy_msg.restype = C.c_int
    L.fxjps_prepare_occupancy_msg.argtypes = [vp, C.POINTER(C.c_int8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, p_i32, p_i32,
                                              p_i32, p_i32, p_i32, p_i32]
    L.fxjps_publish_map.restype = C.c_int
    L.fxjps_publish_map.argtypes = [vp, C.POINTER(C.c_int8), p_i32, p_i32]
    L.fxjps_set_grid_image.restype = C.c_int
    L.fxjps_set_grid_image.argtypes = [vp, p_u8, C.c_int32, C.c_int32]
    L.fxjps_snapshot_image.restype = C.c_int
    L.fxjps_snapshot_image.argtypes = [vp, p_u8, C.c_int32, p_i32, p_i32]
    L.fxjps_get_grid.restype = C.c_int
    L.fxjps_get_grid.argtypes = [vp, p_u8, p_i32, p_i32]
    L.fxjps_get_grid_context.restype = C.c_int
    L.fxjps_get_grid_context.argtypes = [vp, C.c_int32, p_u8, p_i32, p_i32]
    L.fxjps_update_cells.restype = C.c_int
    L.fxjps_update_cells.argtypes = [vp, p_i32, p_u8, C.c_int64]
    L.fxjps_update_cells_deferred.restype = C.c_int
    L.fxjps_update_cells_deferred.argtypes = [vp, p_i32, p_u8, C.c_int64]
    L.fxjps_set_queries.restype = C.c_int
    L.fxjps_set_queries.argtypes = [vp, p_i32, p_i32, C.c_int64, C.c_int32, C.c_int32]
    L.fxjps_replan_frame.restype = C.c_int
    L.fxjps_replan_frame.argtypes = [vp, p_i32, p_u8, C.c_int64, p_i64, p_i32, C.c_int64, p_i32, p_f64, p_f64]
    L.fxjps_refresh_grid.restype = C.c_int
    L.fxjps_refresh_grid.argtypes = [vp, p_u8, C.c_int32, C.c_int32, C.c_int32, C.c_int32, p_i32, p_i32, p_i32, p_i32, p_i32, p_i32, p_i64, p_i32]
    L.fxjps_refresh_occupancy_msg.restype = C.c_int
    L.fxjps_refresh_occupancy_msg.argtypes = [vp, C.POINTER(C.c_int8), C.c_int32, C.c_int32, C.c_int32, C.c_int32, p_i32, p_i32,
                                              p_i32, p_i32, p_i32, p_i32, p_i64, p_i32]
    L.fxjps_last_refresh_cells.restype = C.c_int
    L.fxjps_last_refresh_cells.argtypes = [vp, p_i32, p_u8, C.c_int64, p_i64]
    L.fxjps_replan_frame_raw.restype = C.c_int
    L.fxjps_replan_frame_raw.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, p_i32, p_i32, p_i32, p_i32, p_i32, p_i32,
                                         p_i64, p_i32, p_i64, p_i32, C.c_int64, p_i32, p_f64, p_f64]
    L.fxjps_plan_batch.restype = C.c_int
    L.fxjps_plan_batch.argtypes = [vp, p_i32, p_i32, C.c_int64, C.c_int32, C.c_int32, p_i32, p_i32, p_f64, p_f64]
    L.fxjps_plan_batch_csr.restype = C.c_int
    L.fxjps_plan_batch_csr.argtypes = [vp, p_i32, p_i32, C.c_int64, C.c_int32, C.c_int32, p_i64, p_i32,
                                       C.c_int64, p_i32, p_f64, p_f64]
    L.fxjps_set_grid_slot.restype = C.c_int
    L.fxjps_set_grid_slot.argtypes = [vp, C.c_int32, p_u8, C.c_int32, C.c_int32]
    L.fxjps_get_grid_slot.restype = C.c_int
    L.fxjps_get_grid_slot.argtypes = [vp, C.c_int32, p_u8, p_i32, p_i32]
    L.fxjps_plan_batch_slots_csr.restype = C.c_int
    L.fxjps_plan_batch_slots_csr.argtypes = [vp, p_i32, p_i32, p_i32, C.c_int64, C.c_int32, C.c_int32, p_i64, p_i32,
                                             C.c_int64, p_i32, p_f64, p_f64]
    L.fxjps_replan_slots.restype = C.c_int
    L.fxjps_replan_slots.argtypes = [vp, p_i32, p_i32, p_i32, C.c_int64, C.c_int32, C.c_int32, p_i64, p_i32,
                                     C.c_int64, p_i32, p_f64, p_i32, p_f64]
    L.fxjps_prepare_slots.restype = C.c_int
    L.fxjps_prepare_slots.argtypes = [vp, C.POINTER(SlotJob), C.c_int32]
    L.fxjps_refresh_slots.restype = C.c_int
    L.fxjps_refresh_slots.argtypes = [vp, C.POINTER(SlotJob), C.c_int32, p_i32]
    L.fxjps_set_grid_slots.restype = C.c_int
    L.fxjps_set_grid_slots.argtypes = [vp, C.POINTER(GridJob), C.c_int32]
    L.fxjps_refresh_grid_slots.restype = C.c_int
    L.fxjps_refresh_grid_slots.argtypes = [vp, C.POINTER(GridJob), C.c_int32, p_i32]
    L.fxjps_set_prior_map.restype = C.c_int
    L.fxjps_set_prior_map.argtypes = [vp, C.c_int32, p_u8, C.c_int32, C.c_int32]
    L.fxjps_get_prior_map.restype = C.c_int
    L.fxjps_get_prior_map.argtypes = [vp, C.c_int32, p_u8, p_i32, p_i32]
    L.fxjps_prepare_slots_world.restype = C.c_int
    L.fxjps_prepare_slots_world.argtypes = [vp, C.POINTER(WorldJob), C.c_int32]
    L.fxjps_refresh_slots_world.restype = C.c_int
    L.fxjps_refresh_slots_world.argtypes = [vp, C.POINTER(WorldJob), C.c_int32, p_i32]
    L.fxjps_prepare_slots_cropped.restype = C.c_int
    L.fxjps_prepare_slots_cropped.argtypes = [vp, C.POINTER(WorldJob), C.c_int32, C.POINTER(Crop)]
    L.fxjps_refresh_slots_cropped.restype = C.c_int
    L.fxjps_refresh_slots_cropped.argtypes = [vp, C.POINTER(WorldJob), C.c_int32, p_i32, C.POINTER(Crop)]
    L.fxjps_publish_slots.restype = C.c_int
    L.fxjps_publish_slots.argtypes = [vp, C.POINTER(SlotPublish), C.c_int32]
    L.fxjps_debug_read_slot_maps.restype = C.c_int
    L.fxjps_debug_read_slot_maps.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_int64, p_i64]
    L.fxjps_debug_read_slot_context.restype = C.c_int
    L.fxjps_debug_read_slot_context.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int64, p_i64]
    L.fxjps_debug_live_bytes.restype = C.c_int
    L.fxjps_debug_live_bytes.argtypes = [p_i64, p_i64]
    L.fxjps_debug_read_sets.restype = C.c_int
    L.fxjps_debug_read_sets.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int64, p_i32]
    L.fxjps_set_slot_reuse.restype = C.c_int
    L.fxjps_set_slot_reuse.argtypes = [vp, C.c_int32]
    L.fxjps_debug_slot_tiles.restype = C.c_int
    L.fxjps_debug_slot_tiles.argtypes = [vp, C.c_int32, C.POINTER(C.c_uint64), p_i32, p_i32]
    L.fxjps_debug_slot_read_sets.restype = C.c_int
    L.fxjps_debug_slot_read_sets.argtypes = [vp, C.POINTER(C.c_uint64), C.c_int64, p_i32, p_i32]
    L.fxjps_last_cells.restype = C.c_int
    L.fxjps_last_cells.argtypes = [vp, p_i32, C.c_int64]
    L.fxjps_last_timing.restype = C.c_int
    L.fxjps_last_timing.argtypes = [vp, C.POINTER(Timing)]
    L.fxjps_last_timing_device.restype = C.c_int
    L.fxjps_last_timing_device.argtypes = [vp, C.c_int32, p_i32, p_i64, p_f64, p_i64]
    L.fxjps_rank_unique_id.restype = C.c_int
    L.fxjps_rank_unique_id.argtypes = [vp]
    L.fxjps_create_rank.restype = C.c_int
    L.fxjps_create_rank.argtypes = [C.c_int, C.c_int, C.c_int, vp, C.POINTER(vp)]
    L.fxjps_set_grid_rank.restype = C.c_int
    L.fxjps_set_grid_rank.argtypes = [vp, C.POINTER(C.c_uint8), C.c_int32, C.c_int32]
    L.fxjps_comm_info.restype = C.c_int
    L.fxjps_comm_info.argtypes = [vp, p_i32, p_i32, p_i32]
    L.fxjps_set_memory_share.restype = C.c_int
    L.fxjps_set_memory_share.argtypes = [vp, C.c_int32]
    L.fxjps_selftest_sqrt.restype = C.c_int
    L.fxjps_selftest_sqrt.argtypes = [vp, C.c_uint32, C.c_uint32, p_f64]
    L.fxjps_selftest_wavemin.restype = C.c_int
    L.fxjps_selftest_wavemin.argtypes = [vp, C.c_int32, C.c_uint64, p_i64]
    L.fxjps_debug_read_maps.restype = C.c_int
    L.fxjps_debug_read_maps.argtypes = [vp, C.c_int32, vp, C.c_int64, p_i64]
    p_u32, p_u64 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    L.fxjps_selftest_openlist.restype = C.c_int
    L.fxjps_selftest_openlist.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_double, p_u64, p_u32, C.c_int64, p_u32, p_u32, C.c_int32,
                                          p_u64, p_u32, p_u32, p_u32, p_u32]
    L.fxjps_debug_read_nbmask.restype = C.c_int
    L.fxjps_debug_read_nbmask.argtypes = [vp, p_u8]
    L.fxjps_debug_qstat.restype = C.c_int
    L.fxjps_debug_qstat.argtypes = [vp, p_u64, C.c_int64]
    L.fxjps_debug_counters.restype = C.c_int
    L.fxjps_debug_counters.argtypes = [vp, p_u64]
    L.fxjps_waypoint_ccst_batch.restype = C.c_int
    L.fxjps_waypoint_ccst_batch.argtypes = [vp, C.c_int64, p_i64, p_i32, C.c_double, p_f64, p_f64, p_f64, p_i32, p_f64, p_f64, p_i32, p_i32,
                                            C.c_int64]
    L.fxjps_waypoint_st_batch.restype = C.c_int
    L.fxjps_waypoint_st_batch.argtypes = [vp, C.c_int64, p_i64, p_i32, p_i32, C.c_double, p_f64, p_f64, p_f64, p_i32, C.c_double, C.c_double,
                                          p_f64, p_i32, p_f64, p_i32, p_f64, p_f64, C.c_int32]
    L.fxjps_waypoint_slots_batch.restype = C.c_int
    L.fxjps_waypoint_slots_batch.argtypes = [vp, C.c_int64, p_i64, p_i32, p_i32, p_i32, p_i32, p_f64, p_f64, p_f64, p_f64, p_i32, C.c_double,
                                             C.c_double, p_f64, p_i32, p_f64, p_i32, p_f64, p_f64, p_i32, p_i32, C.c_int64, C.c_int32]
    L.fxjps_tick_outputs_slots.restype = C.c_int
    L.fxjps_tick_outputs_slots.argtypes = [vp, C.c_int64, p_i64, p_i32, p_i32, p_i32, p_i32, p_f64, p_f64, p_f64, p_f64, p_i32, C.c_double,
                                           C.c_double, p_f64, p_i32, p_f64, p_f64, p_i32, p_f64, p_f64, p_i32, p_i32, C.c_int64, p_f64, p_f64,
                                           C.c_int64, p_f64, p_i32, p_i32, C.c_int64, C.c_int32]
    L.fxjps_check_paths_slots.restype = C.c_int
    L.fxjps_check_paths_slots.argtypes = [vp, C.c_int64, p_i64, p_i32, p_i32, p_i32, p_i32, p_i32, p_i32]
    L.fxjps_absorb_prior.restype = C.c_int
    L.fxjps_absorb_prior.argtypes = [vp, C.POINTER(AbsorbJob), C.c_int32, C.c_int32, p_i64]
    L.fxjps_absorb_check.restype = C.c_int  # (no handle, no device: the call's argument check and placement)
    L.fxjps_absorb_check.argtypes = [C.POINTER(AbsorbJob), C.c_int32, C.c_int32, p_i32, C.c_char_p, C.c_int32]
    L.fxjps_absorb_prior_grow.restype = C.c_int
    L.fxjps_absorb_prior_grow.argtypes = [vp, C.POINTER(GrowJob), C.c_int32, C.c_int32, p_i32, C.POINTER(PriorGrown)]
    L.fxjps_grow_check.restype = C.c_int  # (no handle, no device: the call's geometry and refusals)
    L.fxjps_grow_check.argtypes = [C.POINTER(GrowJob), C.c_int32, C.c_int32, p_i32, p_i32, C.POINTER(PriorGrown), C.c_char_p, C.c_int32]
    L.fxjps_absorb_prior_slide.restype = C.c_int
    L.fxjps_absorb_prior_slide.argtypes = [vp, C.POINTER(GrowJob), C.c_int32, C.c_int32, p_i32, C.POINTER(PriorKeep), C.POINTER(PriorSlid)]
    L.fxjps_slide_check.restype = C.c_int  # (no handle, no device: the call's geometry and refusals)
    L.fxjps_slide_check.argtypes = [C.POINTER(GrowJob), C.c_int32, C.c_int32, p_i32, p_i32, C.POINTER(PriorKeep), C.POINTER(PriorSlid), C.c_char_p,
                                    C.c_int32]
    bind_host(L)
    _lib = L
    return L


def ptr(a, ty):
    return a.ctypes.data_as(C.POINTER(ty))
