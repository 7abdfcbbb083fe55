"""Host-side planner object: owns one libfxjps handle (one or more MI355X) and
mirrors the reference's call surface for the grid search.

Reference interface being replaced: jps1.method(matrix, start, goal, hchoice)
(scripts/jps1.py:183-230), called from scripts/global_planner_st.py:285 and
scripts/global_planner_ccst.py:477.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import FxjpsError


def as_occ(matrix):
    """The reference treats a cell as an obstacle iff it compares equal to 1
    (jps1.py:20-29); 100, 0.5, -1 ... are free."""
    return np.ascontiguousarray(np.asarray(matrix) == 1).view(np.uint8)  # (bool -> uint8 is a view: no second pass over the cells)


class Planner(object):
    """A resident occupancy grid plus batched (start, goal) planning on the GPU."""
    _slot_reuse = 0  # set_slot_reuse: the handle's mode
    _slot_nq = 0     # the last replan_slots call's number of queries

    def __init__(self, devices=None):
        L = _lib.load()
        n = L.fxjps_device_count()
        if n <= 0:
            raise FxjpsError(_lib.E_NODEV, "no HIP device visible: fuxi-planner_amd has no CPU fallback")
        if devices is None:
            devices = [0]
        ids = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        rc = L.fxjps_create(_lib.BACKEND_HIP, ids, len(devices), C.byref(h))
        if rc != 0:
            raise FxjpsError(rc, (L.fxjps_last_error(None) or b"").decode())
        self._L = L
        self._h = h
        self.devices = list(devices)
        self.shape = None

    @classmethod
    def for_rank(cls, device, rank, world, unique_id=None):
        """One process per GPU without torch: this process is `rank` of `world` and plans on `device`; `unique_id` is the
        128-byte RCCL id rank 0 got from `Planner.rank_unique_id()` (None for world == 1).  Collective: every rank calls it."""
        L = _lib.load()
        if L.fxjps_device_count() <= 0:
            raise FxjpsError(_lib.E_NODEV, "no HIP device visible: fuxi-planner_amd has no CPU fallback")
        h = C.c_void_p()
        buf = C.create_string_buffer(bytes(unique_id), 128) if unique_id is not None else None
        rc = L.fxjps_create_rank(int(device), int(rank), int(world), buf, C.byref(h))
        if rc != 0:
            raise FxjpsError(rc, (L.fxjps_last_error(None) or b"").decode())
        self = cls.__new__(cls)
        self._L = L
        self._h = h
        self.devices = [int(device)]
        self.shape = None
        self.rank, self.world = int(rank), int(world)
        return self

    @staticmethod
    def rank_unique_id():
        """The id of a new RCCL communicator (ncclGetUniqueId): rank 0 makes it and hands it to the other ranks."""
        L = _lib.load()
        buf = C.create_string_buffer(128)
        rc = L.fxjps_rank_unique_id(buf)
        if rc != 0:
            raise FxjpsError(rc, (L.fxjps_last_error(None) or b"").decode())
        return buf.raw

    @staticmethod
    def rank_preflight(device):
        """What can keep THIS process out of the ranks' collectives, checked without one: the device exists and takes an
        allocation, librccl loads and has the entry points used.  -> None, or the reason as text."""
        try:
            L = _lib.load()
            rc = L.fxjps_rank_preflight(int(device))
        except (OSError, FxjpsError) as e:
            return str(e)
        return None if rc == 0 else "fxjps error %d: %s" % (rc, (L.fxjps_last_error(None) or b"").decode())

    def reserve_grid(self, W, H):
        """Allocate the device buffers of a W x H grid (what the next set_grid* call would allocate), nothing else."""
        self._chk(self._L.fxjps_reserve_grid(self._h, int(W), int(H)))
        self._resident = None

    def set_grid_rank(self, occ, W, H):
        """Collective over the ranks of `for_rank`: rank 0 passes the uint8 [W][H] occupancy, the others None; ONE
        ncclBroadcast of the W*H bytes inside the library, then every rank builds its maps."""
        if occ is not None:
            occ = np.ascontiguousarray(occ, dtype=np.uint8)
            if occ.shape != (W, H):
                raise ValueError("grid shape %r is not (%d, %d)" % (occ.shape, W, H))
        self._chk(self._L.fxjps_set_grid_rank(self._h, _lib.ptr(occ, C.c_uint8) if occ is not None else None, int(W), int(H)))
        self.shape = (int(W), int(H))

    # -- lifetime
    @staticmethod
    def live_bytes():
        """-> (device, pinned): the bytes of device and of pinned host memory that the open handles of this process hold.
        A closed handle leaves both where they were before it was created."""
        dev, pin = C.c_int64(), C.c_int64()
        _lib.load().fxjps_debug_live_bytes(C.byref(dev), C.byref(pin))
        return dev.value, pin.value

    def close(self):
        if getattr(self, "_h", None):
            self._L.fxjps_destroy(self._h)
            self._h = None

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
        if rc != 0:
            raise FxjpsError(rc, (self._L.fxjps_last_error(self._h) or b"").decode())

    # -- grid
    @property
    def shape(self):
        """(W, H) of the resident grid, None before the first one."""
        return self._shape

    @shape.setter
    def shape(self, v):  # (every call that replaces the resident grid sets it: what set_grid remembers is void then)
        self._shape = v
        self._resident = None

    def set_grid(self, matrix):
        """Upload `matrix` (any 2-D array, matrix[x][y], obstacle iff == 1).

        The node hands jps1.method its map anew every tick (global_planner_st.py:246-262 builds `mapu` from scratch each
        time) whether or not a map message arrived in between: a matrix equal to the grid that is resident is not uploaded
        again -- the comparison costs microseconds, the upload and the map build ~ 120 us at the node's map size."""
        occ = as_occ(matrix)
        r = self._resident
        if r is not None and r.shape == occ.shape and np.array_equal(r, occ):
            return
        self.set_grid_occ(occ)
        self._resident = occ  # (as_occ made a new array: nobody else holds it)

    def set_grid_occ(self, occ):
        """Upload a uint8 [W][H] occupancy array (non-zero = obstacle).  The bytes go to the device as they are; every reader
        tests non-zero, so 1, 100 and 255 are the same obstacle."""
        occ = np.ascontiguousarray(occ, dtype=np.uint8)
        if occ.ndim != 2:
            raise ValueError("grid must be 2-D")
        W, H = occ.shape
        self._resident = None  # (a failing upload leaves the handle without a grid, or with half of this one: nothing is resident)
        self._chk(self._L.fxjps_set_grid(self._h, _lib.ptr(occ, C.c_uint8), W, H))
        self.shape = (W, H)

    def set_grid_device(self, dev_ptr, W, H):
        """Adopt a uint8 [W][H] grid that already lives in device memory
        (e.g. the output of an RCCL broadcast done by the host framework)."""
        self._chk(self._L.fxjps_set_grid_device(self._h, C.c_void_p(int(dev_ptr)), int(W), int(H)))
        self.shape = (int(W), int(H))

    def prepare_grid(self, raw, start, goal, ifa, variant="st"):
        """The callers' grid preparation on the device (global_planner_st.py:230-272 / global_planner_ccst.py:415-458):
        pad `raw` (> 0 = occupied) so that start and goal fit, dilate by `ifa`, keep the result resident.
        -> (start', goal', map_d, (W, H), end_occu) with start'/goal' in the prepared grid (goal moved off obstacles)
        and the reference's end_occu flag (global_planner_st.py:268-275 / global_planner_ccst.py:461-464)."""
        raw = np.ascontiguousarray(np.asarray(raw) > 0, dtype=np.uint8)
        if raw.ndim != 2:
            raise ValueError("grid must be 2-D")
        v = {"st": 0, "ccst": 1}[variant] if isinstance(variant, str) else int(variant)
        s = (C.c_int32 * 2)(int(start[0]), int(start[1]))
        g = (C.c_int32 * 2)(int(goal[0]), int(goal[1]))
        W, H, eo = C.c_int32(), C.c_int32(), C.c_int32()
        md = (C.c_int32 * 2)()
        self._chk(self._L.fxjps_prepare_grid(self._h, _lib.ptr(raw, C.c_uint8), raw.shape[0], raw.shape[1], int(ifa), v,
                                             s, g, C.byref(W), C.byref(H), md, C.byref(eo)))
        self.shape = (W.value, H.value)
        return (s[0], s[1]), (g[0], g[1]), (md[0], md[1]), self.shape, eo.value

    @staticmethod
    def shifted_origin(map_o, map_d, map_reso):
        """The map origin after the preparation (global_planner_st.py:235-236 / global_planner_ccst.py:420-421): the
        padding moves it by -map_d cells.  Same expression, same rounding, as the reference's."""
        return list(-np.asarray(map_d) * map_reso + np.asarray(map_o, dtype=np.float64))

    def prepare_occupancy_msg(self, data, width, height, start, goal, ifa, variant="st"):
        """prepare_grid straight from a nav_msgs/OccupancyGrid (`data` = msg.data, int8, row-major [y][x]):
        map_callback (global_planner_st.py:15-20) is fused into the device kernel."""
        data = np.ascontiguousarray(data, dtype=np.int8).reshape(-1)
        if data.size != width * height:
            raise ValueError("data has %d cells, expected %d" % (data.size, width * height))
        v = {"st": 0, "ccst": 1}[variant] if isinstance(variant, str) else int(variant)
        s = (C.c_int32 * 2)(int(start[0]), int(start[1]))
        g = (C.c_int32 * 2)(int(goal[0]), int(goal[1]))
        W, H, eo = C.c_int32(), C.c_int32(), C.c_int32()
        md = (C.c_int32 * 2)()
        self._chk(self._L.fxjps_prepare_occupancy_msg(self._h, _lib.ptr(data, C.c_int8), int(width), int(height), int(ifa), v,
                                                      s, g, C.byref(W), C.byref(H), md, C.byref(eo)))
        self.shape = (W.value, H.value)
        return (s[0], s[1]), (g[0], g[1]), (md[0], md[1]), self.shape, eo.value

    # -- streaming replan from whole raw maps
    @staticmethod
    def _prep_args(start, goal, variant):
        v = {"st": 0, "ccst": 1}[variant] if isinstance(variant, str) else int(variant)
        s = (C.c_int32 * 2)(int(start[0]), int(start[1]))
        g = (C.c_int32 * 2)(int(goal[0]), int(goal[1]))
        return v, s, g, C.c_int32(), C.c_int32(), (C.c_int32 * 2)(), C.c_int32(), C.c_int64(), C.c_int32()

    def refresh_grid(self, raw, start, goal, ifa, variant="st"):
        """prepare_grid for a tick whose raw map mostly did not change: the prepared grid is compared with the resident one on
        the device and only the cells that differ are applied (a partial rebuild).  -> prepare_grid's tuple + (changed, mode);
        mode 0: nothing differs, 1: `changed` cells were updated, 2: the whole build ran (changed -1: nothing to compare with)."""
        raw = np.ascontiguousarray(np.asarray(raw) > 0, dtype=np.uint8)
        if raw.ndim != 2:
            raise ValueError("grid must be 2-D")
        v, s, g, W, H, md, eo, ch, mode = self._prep_args(start, goal, variant)
        self._resident = None
        self._chk(self._L.fxjps_refresh_grid(self._h, _lib.ptr(raw, C.c_uint8), raw.shape[0], raw.shape[1], int(ifa), v,
                                             s, g, C.byref(W), C.byref(H), md, C.byref(eo), C.byref(ch), C.byref(mode)))
        self.shape = (W.value, H.value)
        return (s[0], s[1]), (g[0], g[1]), (md[0], md[1]), self.shape, eo.value, ch.value, mode.value

    def refresh_occupancy_msg(self, data, width, height, start, goal, ifa, variant="st"):
        """refresh_grid straight from a nav_msgs/OccupancyGrid (as prepare_occupancy_msg)."""
        data = np.ascontiguousarray(data, dtype=np.int8).reshape(-1)
        if data.size != width * height:
            raise ValueError("data has %d cells, expected %d" % (data.size, width * height))
        v, s, g, W, H, md, eo, ch, mode = self._prep_args(start, goal, variant)
        self._resident = None
        self._chk(self._L.fxjps_refresh_occupancy_msg(self._h, _lib.ptr(data, C.c_int8), int(width), int(height), int(ifa), v,
                                                      s, g, C.byref(W), C.byref(H), md, C.byref(eo), C.byref(ch), C.byref(mode)))
        self.shape = (W.value, H.value)
        return (s[0], s[1]), (g[0], g[1]), (md[0], md[1]), self.shape, eo.value, ch.value, mode.value

    def last_refresh_cells(self):
        """The cells the last refresh_grid / replan_frame_raw applied in mode 1: -> (xy int32[n, 2], val uint8[n]) in ascending
        order of x * H + y (empty after modes 0 and 2)."""
        n = C.c_int64()
        self._resident = None
        self._chk(self._L.fxjps_last_refresh_cells(self._h, None, None, 0, C.byref(n)))
        xy, val = np.zeros((n.value, 2), np.int32), np.zeros(n.value, np.uint8)
        if n.value:
            self._chk(self._L.fxjps_last_refresh_cells(self._h, _lib.ptr(xy, C.c_int32), _lib.ptr(val, C.c_uint8), n.value, C.byref(n)))
        return xy, val

    def replan_frame_raw(self, raw, start, goal, ifa, variant="st"):
        """replan_frame whose frame is a whole raw map (a matrix as for prepare_grid; an int8 array is taken as a message's
        [height][width] data): diff against the resident grid, reuse what the changed cells cannot reach, plan the stored
        queries.  Needs set_queries and a resident grid of the prepared extents.
        -> (offsets, cells, cost, status) + prepare_grid's tuple + (changed, mode)."""
        raw = np.asarray(raw)
        if raw.ndim != 2:
            raise ValueError("grid must be 2-D")
        if raw.dtype == np.int8:
            layout, raw, W0, H0 = 1, np.ascontiguousarray(raw), raw.shape[1], raw.shape[0]
        else:
            layout, raw, W0, H0 = 0, np.ascontiguousarray(raw > 0, dtype=np.uint8), raw.shape[0], raw.shape[1]
        v, s, g, W, H, md, eo, ch, mode = self._prep_args(start, goal, variant)
        n = getattr(self, "_nq", 0)  # (before set_queries: the library refuses the call)
        self._resident = None
        offsets = np.zeros(n + 1, dtype=np.int64)
        status = np.zeros(n, dtype=np.int32)
        cost = np.zeros(n, dtype=np.float64)
        secs = C.c_double(0.0)
        self._chk(self._L.fxjps_replan_frame_raw(self._h, raw.ctypes.data_as(C.c_void_p), layout, W0, H0, int(ifa), v, s, g, C.byref(W),
                                                 C.byref(H), md, C.byref(eo), C.byref(ch), C.byref(mode), _lib.ptr(offsets, C.c_int64), None, 0,
                                                 _lib.ptr(status, C.c_int32), _lib.ptr(cost, C.c_double), C.byref(secs)))
        cells = np.empty((int(offsets[n]), 2), dtype=np.int32)
        if offsets[n] > 0:
            self._chk(self._L.fxjps_last_cells(self._h, _lib.ptr(cells, C.c_int32), int(offsets[n])))
        self.last_seconds = secs.value
        return offsets, cells, cost, status, (s[0], s[1]), (g[0], g[1]), (md[0], md[1]), (W.value, H.value), eo.value, ch.value, mode.value

    def get_grid(self, context=0):
        """The resident uint8 [W][H] occupancy grid (e.g. the prepared map the node publishes); of a multi-device handle:
        the bytes context `context` holds (equal on every device after the broadcast).  Non-zero = obstacle:
        a grid the library prepared holds 0 / 1, of an uploaded one only the truth of a byte is to be relied on."""
        W, H = C.c_int32(), C.c_int32()
        self._chk(self._L.fxjps_get_grid_context(self._h, int(context), None, C.byref(W), C.byref(H)))
        out = np.empty((W.value, H.value), dtype=np.uint8)
        self._chk(self._L.fxjps_get_grid_context(self._h, int(context), _lib.ptr(out, C.c_uint8), None, None))
        return out

    # -- wire / on-disk adapters
    def publish_map(self):
        """What publish_map (global_planner_st.py:102-115) sends: -> (data int8[W*H] row-major [y][x] with 100 = occupied,
        width, height) of the resident grid."""
        w, h = C.c_int32(), C.c_int32()
        self._chk(self._L.fxjps_publish_map(self._h, None, C.byref(w), C.byref(h)))
        data = np.empty(w.value * h.value, dtype=np.int8)
        self._chk(self._L.fxjps_publish_map(self._h, _lib.ptr(data, C.c_int8), None, None))
        return data, w.value, h.value

    def set_grid_image(self, gray):
        """Adopt a decoded 8-bit grey image (rows x cols) as the resident grid with the prior-map convention of
        global_planner_st.py:176-182: > 200 free, else occupied, grid = img[::-1].T."""
        gray = np.ascontiguousarray(gray, dtype=np.uint8)
        if gray.ndim != 2:
            raise ValueError("image must be 2-D (convert('L'))")
        self._chk(self._L.fxjps_set_grid_image(self._h, _lib.ptr(gray, C.c_uint8), gray.shape[0], gray.shape[1]))
        self.shape = (gray.shape[1], gray.shape[0])

    def snapshot_image(self, channels=1):
        """The snapshot convention of global_planner_st.py:365-374: uint8 [H][W] (or [H][W][3]) image, 255 = free."""
        r, c = C.c_int32(), C.c_int32()
        self._chk(self._L.fxjps_snapshot_image(self._h, None, int(channels), C.byref(r), C.byref(c)))
        out = np.empty((r.value, c.value) if channels == 1 else (r.value, c.value, channels), dtype=np.uint8)
        self._chk(self._L.fxjps_snapshot_image(self._h, _lib.ptr(out, C.c_uint8), int(channels), None, None))
        return out

    def update_cells(self, xy, val, rebuild=True):
        """Set cells of the resident grid.  rebuild=False: the derived maps are rebuilt by the next planning call (or
        the next update with rebuild=True) instead of now -- for several updates in a row."""
        xy = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1, 2)
        val = np.ascontiguousarray(val, dtype=np.uint8).reshape(-1)
        if len(val) != len(xy):
            raise ValueError("xy and val lengths differ")
        self._resident = None
        fn = self._L.fxjps_update_cells if rebuild else self._L.fxjps_update_cells_deferred
        self._chk(fn(self._h, _lib.ptr(xy, C.c_int32), _lib.ptr(val, C.c_uint8), len(val)))

    # -- planning
    def default_max_path_len(self):
        W, H = self.shape
        return int(min(W * H + 1, max(256, 4 * max(W, H))))

    def plan_batch(self, starts, goals, hchoice=2, max_path_len=None):
        """-> (offsets int64[n+1], cells int32[total,2], cost float64[n], status int32[n]).

        status[q] > 0: number of jump points of query q (cells[offsets[q]:offsets[q+1]]),
        0: no path, < 0: a per-query error code (_lib.Q_*)."""
        if self.shape is None:
            raise FxjpsError(_lib.E_NOGRID, "plan_batch before set_grid")
        starts = np.ascontiguousarray(starts, dtype=np.int32).reshape(-1, 2)
        goals = np.ascontiguousarray(goals, dtype=np.int32).reshape(-1, 2)
        if len(starts) != len(goals):
            raise ValueError("starts and goals lengths differ")
        if hchoice not in (1, 2):
            # heuristic() returns None and jps1.py:188/227 then fails on None + float
            raise TypeError("unsupported operand type(s) for +: 'float' and 'NoneType' (hchoice must be 1 or 2)")
        n = len(starts)
        auto = max_path_len is None
        mpl = self.default_max_path_len() if auto else int(max_path_len)
        limit = self.shape[0] * self.shape[1] + 1
        while True:
            offsets = np.zeros(n + 1, dtype=np.int64)
            status = np.zeros(n, dtype=np.int32)
            cost = np.zeros(n, dtype=np.float64)
            secs = C.c_double(0.0)
            # sizing call (cells stay in the handle), then one copy into an exactly sized array
            self._chk(self._L.fxjps_plan_batch_csr(self._h, _lib.ptr(starts, C.c_int32), _lib.ptr(goals, C.c_int32), n,
                                                   int(hchoice), mpl, _lib.ptr(offsets, C.c_int64), None, 0,
                                                   _lib.ptr(status, C.c_int32), _lib.ptr(cost, C.c_double),
                                                   C.byref(secs)))
            cells = np.empty((int(offsets[n]), 2), dtype=np.int32)
            if offsets[n] > 0:
                self._chk(self._L.fxjps_last_cells(self._h, _lib.ptr(cells, C.c_int32), int(offsets[n])))
            if auto and mpl < limit and (status == _lib.Q_PATH_TOO_LONG).any():
                mpl = min(limit, mpl * 8)  # rare: a path with more jump points than the default slot
                continue
            break
        self.last_seconds = secs.value
        return offsets, cells, cost, status

    # -- grid slots: several resident grids, one batch over all of them
    def set_grid_slot(self, slot, matrix):
        """Upload `matrix` (as set_grid takes it: matrix[x][y], obstacle iff == 1) into grid slot `slot`
        (0 .. _lib.MAX_GRID_SLOTS - 1) and build its maps.  The resident grid is not touched."""
        occ = as_occ(matrix)
        if occ.ndim != 2:
            raise ValueError("grid must be 2-D")
        W, H = occ.shape
        self._chk(self._L.fxjps_set_grid_slot(self._h, int(slot), _lib.ptr(occ, C.c_uint8), W, H))

    def clear_grid_slot(self, slot):
        """Release grid slot `slot` (its device memory goes back; a batch that names it is refused)."""
        self._chk(self._L.fxjps_set_grid_slot(self._h, int(slot), None, 0, 0))

    def get_grid_slot(self, slot):
        """The uint8 [W][H] occupancy grid of slot `slot` (non-zero = obstacle; 1 when set_grid_slot or a prepare call wrote it)."""
        W, H = C.c_int32(), C.c_int32()
        self._chk(self._L.fxjps_get_grid_slot(self._h, int(slot), None, C.byref(W), C.byref(H)))
        out = np.empty((W.value, H.value), dtype=np.uint8)
        self._chk(self._L.fxjps_get_grid_slot(self._h, int(slot), _lib.ptr(out, C.c_uint8), None, None))
        return out

    def prepare_slots(self, jobs):
        """The fleet's map half of a tick in ONE call (fxjps_prepare_slots): every job's raw map is padded, dilated and
        built into its grid slot as prepare_grid / prepare_occupancy_msg would prepare the resident grid.  A job is
        (slot, raw, start, goal, ifa, variant) with raw[x][y] (> 0 = occupied), or (slot, (data, width, height), start,
        goal, ifa, variant) for a nav_msgs/OccupancyGrid; variant "st" / "ccst".  -> per job (start', goal', map_d,
        (W, H), end_occu, ok); ok False: the goal's row and column are fully occupied (the reference raises there) and
        that slot is empty.  The resident grid is not touched."""
        jobs = list(jobs)
        arr, keep = self._slot_jobs(jobs)  # (keep: the raws, alive until the call has returned)
        self._chk(self._L.fxjps_prepare_slots(self._h, arr, len(jobs)))
        del keep
        return self._slot_outs(arr, len(jobs))

    def refresh_slots(self, jobs):
        """prepare_slots for the tick after (fxjps_refresh_slots): the same jobs, the same slots and outputs afterwards, but
        a job whose prepared grid is byte for byte what its slot already holds keeps the slot's maps and costs no build
        work.  -> per job (start', goal', map_d, (W, H), end_occu, ok, kept); kept False: the slot was built (it was
        empty, its extents or a byte differed, the prepared grid has more than 2^18 cells, or the job failed)."""
        jobs = list(jobs)
        arr, keep = self._slot_jobs(jobs)
        n = len(jobs)
        kept = np.zeros(max(n, 1), dtype=np.int32)
        self._chk(self._L.fxjps_refresh_slots(self._h, arr, n, _lib.ptr(kept, C.c_int32)))
        del keep
        return [o + (bool(k),) for o, k in zip(self._slot_outs(arr, n), kept[:n])]

    def set_grid_slots(self, jobs):
        """set_grid_slot for many slots in ONE call (fxjps_set_grid_slots): jobs is a list of (slot, matrix), matrix[x][y]
        with an obstacle iff == 1, as set_grid_slot takes it.  Afterwards every named slot is what set_grid_slot would have
        left; the launches and host waits of the call do not depend on len(jobs)."""
        arr, keep = self._grid_jobs(jobs)  # (keep: the grids, alive until the call has returned)
        self._chk(self._L.fxjps_set_grid_slots(self._h, arr, len(keep)))
        del keep

    def refresh_grid_slots(self, jobs):
        """set_grid_slots for the tick after (fxjps_refresh_grid_slots): the same slots afterwards, but a slot that already
        holds a grid of the same extents and bytes keeps its maps and its generation, so replan_slots does not search its
        unchanged queries again.  -> one bool per job, kept; False: the slot was built (it was empty, its extents or a byte
        differed, or the grid has more than 2^18 cells)."""
        arr, keep = self._grid_jobs(jobs)
        n = len(keep)
        kept = np.zeros(max(n, 1), dtype=np.int32)
        self._chk(self._L.fxjps_refresh_grid_slots(self._h, arr, n, _lib.ptr(kept, C.c_int32)))
        del keep
        return [bool(k) for k in kept[:n]]

    @staticmethod
    def _grid_jobs(jobs):
        """-> the fxjps_grid_job_t array of set_grid_slots' jobs, and the grids it points into."""
        jobs = list(jobs)
        arr = (_lib.GridJob * max(len(jobs), 1))()
        keep = []
        for j, (slot, matrix) in zip(arr, jobs):
            occ = as_occ(matrix)
            if occ.ndim != 2:
                raise ValueError("grid must be 2-D")
            keep.append(occ)
            j.occ, j.slot, j.W, j.H = _lib.ptr(occ, C.c_uint8), int(slot), occ.shape[0], occ.shape[1]
        return arr, keep

    @staticmethod
    def _job_raw(j, slot, raw, ifa, variant):
        """Fill what fxjps_slot_job_t and fxjps_world_job_t share -- raw, layout, W0, H0, slot, ifa, variant -- from a job's
        raw[x][y] or (data, width, height).  -> the array j.raw points into."""
        if isinstance(raw, tuple):
            data, width, height = raw
            a = np.ascontiguousarray(data, dtype=np.int8).reshape(-1)
            if a.size != width * height:
                raise ValueError("data has %d cells, expected %d" % (a.size, width * height))
            j.layout, j.W0, j.H0 = 1, int(width), int(height)
        else:
            a = np.ascontiguousarray(np.asarray(raw) > 0, dtype=np.uint8)
            if a.ndim != 2:
                raise ValueError("grid must be 2-D")
            j.layout, j.W0, j.H0 = 0, a.shape[0], a.shape[1]
        j.raw = a.ctypes.data
        j.slot, j.ifa = int(slot), int(ifa)
        j.variant = {"st": 0, "ccst": 1}[variant] if isinstance(variant, str) else int(variant)
        return a

    @staticmethod
    def _slot_jobs(jobs):
        """-> the fxjps_slot_job_t array of prepare_slots' jobs, and the raws it points into (the caller holds them until the
        C call has returned)."""
        arr = (_lib.SlotJob * max(len(jobs), 1))()
        keep = []
        for j, (slot, raw, start, goal, ifa, variant) in zip(arr, jobs):
            keep.append(Planner._job_raw(j, slot, raw, ifa, variant))
            j.start_xy[0], j.start_xy[1] = int(start[0]), int(start[1])
            j.goal_xy[0], j.goal_xy[1] = int(goal[0]), int(goal[1])
        return arr, keep

    @staticmethod
    def _slot_outs(arr, n, goal="goal_xy"):
        """(goal: the field of the goal's cell -- goal_xy_cell in a fxjps_world_job_t, whose goal_xy is the position)"""
        return [((j.start_xy[0], j.start_xy[1]), tuple(getattr(j, goal)), (j.map_d[0], j.map_d[1]), (j.W, j.H), j.end_occu,
                 j.status == 0) for j in arr[:n]]

    # -- world-frame ticks: a prior map on the device, positions instead of cells (fxjps_prepare_slots_world)
    def set_prior_map(self, prior, matrix):
        """Upload `matrix` ([x][y], > 0 = occupied: a map known before the flight, st:176-187) as prior map `prior`
        (0 .. _lib.MAX_PRIOR_MAPS - 1).  Once per flight; no slot and not the resident grid is touched."""
        occ = np.ascontiguousarray(np.asarray(matrix) > 0, dtype=np.uint8)
        if occ.ndim != 2:
            raise ValueError("a prior map must be 2-D")
        self._origins().pop(int(prior), None)  # (an uploaded prior lies at the caller's ori_pre again)
        self._chk(self._L.fxjps_set_prior_map(self._h, int(prior), _lib.ptr(occ, C.c_uint8), occ.shape[0], occ.shape[1]))

    def set_prior_image(self, prior, gray):
        """set_prior_map from a decoded 8-bit grey image (rows x cols) with the loader convention of
        global_planner_st.py:179-182: > 200 free, else occupied, map = img[::-1].T."""
        from . import worldprep
        self.set_prior_map(prior, worldprep.prior_from_image(gray))

    def get_prior_map(self, prior):
        """The uint8 [W][H] bytes of prior map `prior` (non-zero = occupied)."""
        W, H = C.c_int32(), C.c_int32()
        self._chk(self._L.fxjps_get_prior_map(self._h, int(prior), None, C.byref(W), C.byref(H)))
        out = np.empty((W.value, H.value), dtype=np.uint8)
        self._chk(self._L.fxjps_get_prior_map(self._h, int(prior), _lib.ptr(out, C.c_uint8), None, None))
        return out

    def clear_prior_map(self, prior):
        """Release prior map `prior` (a world job that names it is refused)."""
        self._origins().pop(int(prior), None)
        self._chk(self._L.fxjps_set_prior_map(self._h, int(prior), None, 0, 0))

    def prepare_slots_world(self, jobs):
        """prepare_slots from what a node holds at the top of its tick (fxjps_prepare_slots_world): the prior-map merge
        (st:210-225 / ccst:395-409) and the world -> cell conversion (st:226-227) happen in the call, the prior stays on the
        device and only the detected map is staged.  A job is (slot, raw or (data, width, height), map_o, map_reso, pos_xy,
        goal_xy, ifa, variant[, prior=None[, ori_pre=(-15, -15)[, map_t=None]]]); map_t None: map_o + extent * map_reso
        (st:24).  -> per job prepare_slots' tuple followed by origin (the origin after the padding, st:236),
        canvas_shape and canvas_o (the merged origin).  worldprep.merge_host is the same conversion on the host."""
        jobs = list(jobs)
        arr, keep = self._world_jobs(jobs)
        self._chk(self._L.fxjps_prepare_slots_world(self._h, arr, len(jobs)))
        del keep
        return [o + w for o, w in zip(self._slot_outs(arr, len(jobs), "goal_xy_cell"), self._world_outs(arr, len(jobs)))]

    def refresh_slots_world(self, jobs):
        """refresh_slots from world-frame jobs (fxjps_refresh_slots_world): -> per job refresh_slots' tuple (kept last)
        followed by origin, canvas_shape, canvas_o."""
        jobs = list(jobs)
        arr, keep = self._world_jobs(jobs)
        n = len(jobs)
        kept = np.zeros(max(n, 1), dtype=np.int32)
        self._chk(self._L.fxjps_refresh_slots_world(self._h, arr, n, _lib.ptr(kept, C.c_int32)))
        del keep
        return [o + (bool(k),) + w for o, k, w in zip(self._slot_outs(arr, n, "goal_xy_cell"), kept[:n], self._world_outs(arr, n))]

    def prepare_slots_cropped(self, jobs):
        """prepare_slots_world with the ccst node's crop in front (fxjps_prepare_slots_cropped): a job's raw, map_o (and
        extents) are those of the map MESSAGE as map_callback left it, and remove_zero_rowscols (ccst:36-63) -- the cut to
        the box of the non-zero cells and the vehicle's cell, the moved map_o / map_t -- happens in the call, the box found
        on the device.  Jobs as prepare_slots_world takes them (map_t is not read).  A matrix raw[x][y] counts as > 0 =
        occupied, as everywhere; a (data, width, height) message counts for the box as the reference's nonzero() does.
        -> per job prepare_slots_world's tuple, then status (0; _lib.JOB_NOT_PLANNED: the node does not plan on this
        tick; _lib.E_ARG: refused, the vehicle lies left of or below the message, or the goal has no free cell) and the
        crop record (a dict with fxjps_crop_t's fields).  Unless status is 0 the slot is empty and ok is False.
        worldprep.crop_host is the same crop on the host."""
        jobs = list(jobs)
        arr, keep = self._world_jobs(jobs)
        n = len(jobs)
        crop = (_lib.Crop * max(n, 1))()
        self._chk(self._L.fxjps_prepare_slots_cropped(self._h, arr, n, crop))
        del keep
        return [o + w + c for o, w, c in zip(self._slot_outs(arr, n, "goal_xy_cell"), self._world_outs(arr, n), self._crop_outs(arr, crop, n))]

    def refresh_slots_cropped(self, jobs):
        """refresh_slots_world with the crop in front (fxjps_refresh_slots_cropped): -> per job refresh_slots_world's tuple
        followed by status and the crop record.  A job that is not planned or refused is never kept."""
        jobs = list(jobs)
        arr, keep = self._world_jobs(jobs)
        n = len(jobs)
        kept = np.zeros(max(n, 1), dtype=np.int32)
        crop = (_lib.Crop * max(n, 1))()
        self._chk(self._L.fxjps_refresh_slots_cropped(self._h, arr, n, _lib.ptr(kept, C.c_int32), crop))
        del keep
        return [o + (bool(k),) + w + c for o, k, w, c in zip(self._slot_outs(arr, n, "goal_xy_cell"), kept[:n], self._world_outs(arr, n),
                                                             self._crop_outs(arr, crop, n))]

    @staticmethod
    def _crop_outs(arr, crop, n):
        return [(j.status, {"bbox": list(c.bbox), "start0": list(c.start0), "lo": list(c.lo), "win": list(c.win), "map_o": list(c.map_o),
                            "map_t": list(c.map_t)}) for j, c in zip(arr[:n], crop[:n])]

    @staticmethod
    def _world_jobs(jobs):
        """-> the fxjps_world_job_t array of prepare_slots_world's jobs, and the raws it points into."""
        from . import worldprep
        arr = (_lib.WorldJob * max(len(jobs), 1))()
        keep = []
        for j, job in zip(arr, jobs):
            slot, raw, map_o, map_reso, pos_xy, goal_xy, ifa, variant = job[:8]
            prior, ori_pre, map_t = (tuple(job[8:]) + (None, (-15, -15), None)[len(job) - 8:])[:3]
            keep.append(Planner._job_raw(j, slot, raw, ifa, variant))
            j.prior = -1 if prior is None else int(prior)
            j.map_reso = float(map_reso)
            if map_t is None:
                map_t = worldprep.map_top(map_o, (j.W0, j.H0), map_reso)
            for k in range(2):
                j.map_o[k], j.map_t[k], j.pos_xy[k] = float(map_o[k]), float(map_t[k]), float(pos_xy[k])
                j.goal_xy[k], j.ori_pre[k] = float(goal_xy[k]), float(ori_pre[k])
        return arr, keep

    @staticmethod
    def _world_outs(arr, n):
        return [([j.origin[0], j.origin[1]], (j.canvas_W, j.canvas_H), [j.canvas_o[0], j.canvas_o[1]]) for j in arr[:n]]

    def absorb_prior(self, jobs, mode="overwrite", crops=None):
        """Fold the vehicles' detected maps into the prior maps they name, on the device (fxjps_absorb_prior: one launch
        whatever len(jobs) is): every job's rectangle is pasted into its prior where the world-frame calls' canvas puts it,
        cells outside the prior are dropped, and the next world-frame call of ANY vehicle sees the result under its own
        detected map.  jobs: world jobs as prepare_slots_world takes them (the slot, pos_xy, goal_xy, ifa, variant and
        map_t are not read; prior None is a ValueError), at most 256, applied in order.  crops[j]: None, or the crop record
        prepare_slots_cropped returned for job j -- then the job's raw is the map MESSAGE and the rectangle is the record's
        window (lo, win) at the record's map_o.  mode "overwrite" (the reference's slice assignment: a free detected cell
        clears the prior's), "occupied" (only ever adds obstacles) or "known" (cells that are -1 in a message leave the
        prior as it is).  -> ([(inside, outside) per job], {prior: cells whose occupancy flipped}).  No slot, no stored
        result and not the resident grid is touched.  worldprep.absorb_host is the same paste on the host."""
        arr, n, _, keep = self._prior_jobs(jobs, mode, crops, None, _lib.AbsorbJob)
        changed = np.zeros(_lib.MAX_PRIOR_MAPS, dtype=np.int64)
        self._chk(self._L.fxjps_absorb_prior(self._h, arr, n, _lib.ABSORB_MODES[mode], _lib.ptr(changed, C.c_int64)))
        del keep
        named = sorted({int(a.prior) for a in arr[:n]})
        return [(int(a.inside), int(a.outside)) for a in arr[:n]], {p: int(changed[p]) for p in named}

    def absorb_prior_grow(self, jobs, mode="overwrite", crops=None, limit=None):
        """absorb_prior on priors that GROW to what the vehicles have seen (fxjps_absorb_prior_grow: one launch whatever
        len(jobs) is): every named prior becomes the canvas the nodes build each tick -- the union of the prior and the
        detected map (st:212-220) -- kept, job after job; no cell of a rectangle is dropped.  jobs, crops and mode as
        absorb_prior takes them; a job's ori_pre is the prior's origin as it is NOW, the same in every job that names the
        prior (prior_origin(prior) once it has grown); its map_t comes from the job, or from the crop record, or is map_o +
        extent * map_reso.  limit: None (8190), one number or a pair: the largest side a prior may grow to, per axis -- a
        job that would exceed it refuses the whole call.  -> ([at per job: the cell of the grown prior that the
        rectangle's cell (0, 0) landed on], {prior: {"W", "H", "shift", "origin", "changed"}}): the new extents, where
        old cell (0, 0) lies now, the new world origin and the cells whose occupancy differs from the old byte at that
        place.  The planner remembers each grown prior's origin (prior_origin); the library stores none.  On a refusal or
        a failure every prior is what it was, byte for byte.  worldprep.grow_host is the same fold on the host."""
        arr, n, lim, keep = self._prior_jobs(jobs, mode, crops, limit, _lib.GrowJob)
        out = (_lib.PriorGrown * _lib.MAX_PRIOR_MAPS)()
        self._chk(self._L.fxjps_absorb_prior_grow(self._h, arr, n, _lib.ABSORB_MODES[mode], None if lim is None else _lib.ptr(lim, C.c_int32), out))
        del keep
        grown = {p: self._prior_record(p, g) for p, g in enumerate(out) if g.named}
        return [(int(a.at[0]), int(a.at[1])) for a in arr[:n]], grown

    @staticmethod
    def _prior_jobs(jobs, mode, crops, limit, job_type):
        """absorb_prior's (job_type _lib.AbsorbJob), absorb_prior_grow's and absorb_prior_slide's (_lib.GrowJob: with map_t)
        arguments as the library takes them -> (job array, n, limit_wh or None, the raws: alive until the call has returned)."""
        from . import worldprep
        jobs = list(jobs)
        n = len(jobs)
        if mode not in _lib.ABSORB_MODES:
            raise ValueError("mode %r is not one of %r" % (mode, tuple(_lib.ABSORB_MODES)))
        if crops is not None and len(crops) != n:
            raise ValueError("%d crop records for %d jobs" % (len(crops), n))
        lim = None
        if limit is not None:
            lim = np.array([limit, limit] if np.isscalar(limit) else [limit[0], limit[1]], dtype=np.int32)
        arr = (job_type * max(n, 1))()
        keep = []
        for v, (a, job) in enumerate(zip(arr, jobs)):
            raw, map_o, map_reso = job[1], job[2], job[3]
            prior, ori_pre, map_t = (tuple(job[8:11]) + (None, (-15, -15), None)[len(job[8:11]):])[:3]
            if prior is None:
                raise ValueError("job %d names no prior map" % v)
            w = _lib.WorldJob()  # (raw, layout and extents as the world-frame calls take them)
            keep.append(Planner._job_raw(w, 0, raw, 0, 0))
            a.raw, a.layout, a.W0, a.H0 = w.raw, w.layout, w.W0, w.H0
            rec = None if crops is None else crops[v]
            lo, win = ((0, 0), (a.W0, a.H0)) if rec is None else (rec["lo"], rec["win"])
            if rec is not None:
                map_o = rec["map_o"]
            a.prior, a.map_reso = int(prior), float(map_reso)
            for k in range(2):
                a.lo[k], a.win[k], a.map_o[k], a.ori_pre[k] = int(lo[k]), int(win[k]), float(map_o[k]), float(ori_pre[k])
            if job_type is _lib.GrowJob:
                if rec is not None:
                    map_t = rec["map_t"]
                if map_t is None:
                    map_t = worldprep.map_top(map_o, win, map_reso)
                a.map_t[0], a.map_t[1] = float(map_t[0]), float(map_t[1])
        return arr, n, lim, keep

    def _prior_record(self, p, g):
        """What absorb_prior_grow and absorb_prior_slide return of prior p, from the keys their out records share; the
        planner remembers the new origin."""
        self._origins()[p] = (float(g.origin[0]), float(g.origin[1]))
        return {"W": int(g.W), "H": int(g.H), "shift": (int(g.shift[0]), int(g.shift[1])), "origin": [float(g.origin[0]), float(g.origin[1])],
                "changed": int(g.changed)}

    def absorb_prior_slide(self, jobs, mode="overwrite", crops=None, limit=None, keep=None, use="over_limit"):
        """absorb_prior_grow followed, per prior, by a cut to a keep window, in the same single launch
        (fxjps_absorb_prior_slide): a prior that moves with the fleet instead of refusing the call once a side would pass
        the limit.  jobs, mode, crops and limit as absorb_prior_grow takes them.  keep: {prior: (lo_xy, hi_xy)}, the window
        in world metres (an infinite bound: no cut on that side); a prior without one behaves exactly as under
        absorb_prior_grow.  use: "always" -- cut on every call; "over_limit" -- the whole window is applied if and only
        if a grown side exceeds the limit; "none"; or {prior: use} (a prior of keep that it leaves out: "none").  A prior
        with a window is not held to the limit job after job; a window above the limit, one that holds no cell of the
        grown prior and one for a prior no job names refuse the whole call.  -> ([(at, inside, outside) per job], {prior:
        record}): at -- the cell of the prior as the call leaves it that the rectangle's cell (0, 0) lies on (it may be
        negative), inside / outside -- the rectangle's cells in the window and the rest, which are dropped; the record
        holds absorb_prior_grow's keys (shift may be negative; changed counts cells of the window only) and trimmed
        (whether the window was applied), grown_wh (the extents the fold reached) and cut_lo / cut_hi (the cells cut off
        each side of them).  prior_origin is updated as absorb_prior_grow updates it; on a refusal or a failure every
        prior is what it was.  worldprep.slide_host is the same on the host."""
        arr, n, lim, raws = self._prior_jobs(jobs, mode, crops, limit, _lib.GrowJob)
        win = None
        if keep:
            win = (_lib.PriorKeep * _lib.MAX_PRIOR_MAPS)()
            for p, (lo, hi) in keep.items():
                u = use.get(p, "none") if isinstance(use, dict) else use
                if u not in _lib.KEEP_USES:
                    raise ValueError("use %r is not one of %r" % (u, tuple(_lib.KEEP_USES)))
                if not 0 <= int(p) < _lib.MAX_PRIOR_MAPS:
                    raise ValueError("keep names prior %r: not in 0 .. %d" % (p, _lib.MAX_PRIOR_MAPS - 1))
                w = win[int(p)]
                w.use = _lib.KEEP_USES[u]
                for k in range(2):
                    w.lo[k], w.hi[k] = float(lo[k]), float(hi[k])
        out = (_lib.PriorSlid * _lib.MAX_PRIOR_MAPS)()
        self._chk(self._L.fxjps_absorb_prior_slide(self._h, arr, n, _lib.ABSORB_MODES[mode], None if lim is None else _lib.ptr(lim, C.c_int32), win, out))
        del raws
        slid = {p: dict(self._prior_record(p, g), trimmed=bool(g.trimmed), grown_wh=(int(g.grown_wh[0]), int(g.grown_wh[1])),
                        cut_lo=(int(g.cut_lo[0]), int(g.cut_lo[1])), cut_hi=(int(g.cut_hi[0]), int(g.cut_hi[1])))
                for p, g in enumerate(out) if g.named}
        return [((int(a.at[0]), int(a.at[1])), int(a.inside), int(a.outside)) for a in arr[:n]], slid

    def _origins(self):
        if getattr(self, "_prior_origin", None) is None:
            self._prior_origin = {}
        return self._prior_origin

    def prior_origin(self, prior):
        """The world origin of prior map `prior` as absorb_prior_grow last left it, or None: the prior has not grown since
        it was uploaded (set_prior_map and clear_prior_map forget the origin; it is then the caller's ori_pre again)."""
        return self._origins().get(int(prior))

    def _tick_absorb(self, absorb, jobs, outs, crop, recs, grow=None):
        """fleet_tick_world's absorb=: after the tick's prepare / refresh call, every job that names a prior is absorbed --
        a cropped job through its window, unless it has none (not planned, refused).  recs[v]["absorbed"] is set.  grow:
        None, or (grow_limit, slide): through absorb_prior_grow, and recs[v]["ori_pre"] / ["grown"] are set as well; slide not
        None: through absorb_prior_slide with each prior's keep box (_keep_boxes), and recs[v]["slid"] is set too."""
        if absorb is None:
            return
        take, crops = [], []
        for v, job in enumerate(jobs):
            recs[v]["absorbed"] = None
            if grow is not None:
                recs[v]["grown"] = None
                if grow[1] is not None:
                    recs[v]["slid"] = None
                recs[v]["ori_pre"] = None if len(job) <= 8 or job[8] is None else tuple(float(x) for x in (job[9] if len(job) > 9 else (-15, -15)))
            if len(job) <= 8 or job[8] is None:
                continue
            if crop and outs[v][-2] in (_lib.JOB_NOT_PLANNED, _lib.E_ARG):
                continue
            take.append(v)
            crops.append(outs[v][-1] if crop else None)
        if take and grow is not None and grow[1] is not None:
            sub = [jobs[v] for v in take]
            per_job, slid = self.absorb_prior_slide(sub, absorb, crops if crop else None, grow[0], self._keep_boxes(sub, crops, grow[1]), "over_limit")
            for v, (_, inside, outside) in zip(take, per_job):
                recs[v]["absorbed"] = (inside, outside)
                recs[v]["grown"] = recs[v]["slid"] = slid[int(jobs[v][8])]
        elif take and grow is not None:
            _, grown = self.absorb_prior_grow([jobs[v] for v in take], absorb, crops if crop else None, grow[0])
            for v, c in zip(take, crops):
                raw = jobs[v][1]
                win = c["win"] if crop else (raw[1], raw[2]) if isinstance(raw, tuple) else np.asarray(raw).shape
                recs[v]["absorbed"] = (int(win[0]) * int(win[1]), 0)  # (nothing is dropped: the prior grows)
                recs[v]["grown"] = grown[int(jobs[v][8])]
        elif take:
            counts, _ = self.absorb_prior([jobs[v] for v in take], absorb, crops if crop else None)
            for v, c in zip(take, counts):
                recs[v]["absorbed"] = c

    @staticmethod
    def _keep_boxes(jobs, crops, margin):
        """fleet_tick_world's slide=: per prior the box over the jobs that name it -- each job's rectangle [map_o, map_t] (the
        crop record's for a cropped job), its pos_xy and its goal_xy -- widened by margin metres on every side: the
        neighbourhood of the vehicles and of the way to their goals.  -> {prior: (lo_xy, hi_xy)}."""
        from . import worldprep
        boxes = {}
        for job, rec in zip(jobs, crops):
            raw, map_o = job[1], job[2]
            if rec is not None:
                map_o, map_t = rec["map_o"], rec["map_t"]
            elif len(job) > 10 and job[10] is not None:
                map_t = job[10]
            else:
                map_t = worldprep.map_top(map_o, (raw[1], raw[2]) if isinstance(raw, tuple) else np.asarray(raw).shape, job[3])
            lo, hi = boxes.setdefault(int(job[8]), ([float("inf")] * 2, [float("-inf")] * 2))
            for k in range(2):
                pts = (float(map_o[k]), float(map_t[k]), float(job[4][k]), float(job[5][k]))
                lo[k], hi[k] = min(lo[k], min(pts) - margin), max(hi[k], max(pts) + margin)
        return {p: (tuple(lo), tuple(hi)) for p, (lo, hi) in boxes.items()}

    def fleet_tick_world(self, jobs, pos, global_goals, home, prev_wp=None, prev_dim=None, publish=True, image_channels=None, refresh=False,
                         reuse=False, crop=False, throttle=None, check_kept=True, absorb=None, grow=False, grow_limit=None, slide=None):
        """fleet_tick from world-frame jobs (as prepare_slots_world takes them): the maps are prepared through
        prepare_slots_world (refresh=True: refresh_slots_world), and each vehicle's resolution and shifted origin are the
        job's and the call's instead of the caller's.  The same records; kept / reused where refresh / reuse ask for them
        (reuse=True plans through replan_slots).  crop=True: the jobs hold the ccst node's map MESSAGES and are prepared
        through prepare_slots_cropped / refresh_slots_cropped; every record has a further key, not_planned (bool), and a
        vehicle that is not planned on this tick (ccst:351) or was refused has ok False.  throttle / check_kept: the ccst
        node's replan throttle, as fleet_tick_throttled describes it.  absorb: None, or "overwrite" / "occupied" / "known": after the
        tick's prepare / refresh call every job that names a prior is folded into it through absorb_prior (a cropped job
        through its window; not one that is not planned or refused), so THIS tick's records are what absorb=None gives and
        the next tick of every vehicle sees the merged prior; every record then has a further key, absorbed: (inside,
        outside), or None for a job that was not absorbed.  grow=True (needs absorb): the absorb step goes through
        absorb_prior_grow, so a prior grows to what the vehicles have seen instead of dropping the cells outside it
        (grow_limit: its `limit`); every record gains ori_pre -- the prior origin the job was prepared and absorbed with, None
        without a prior -- and grown, the prior's record from absorb_prior_grow, or None for a job that was not absorbed.
        Once a prior has a remembered origin (prior_origin), every job that names it is prepared and absorbed with that
        origin instead of the job's own ori_pre, on grow=False ticks as well: the job's is the origin of the upload.
        slide: None, or a margin in metres, at least 0 (needs grow=True): the absorb step goes through absorb_prior_slide
        with use="over_limit", so a prior that would pass grow_limit is cut to its keep box instead of refusing the tick --
        per prior the box over the absorbed jobs that name it, covering each job's rectangle [map_o, map_t] (the crop
        record's for a cropped job), pos_xy and goal_xy, widened by the margin on every side: the pre-known map between
        the fleet and its goals survives, the strip left behind is dropped.  Every record gains slid: the prior's record from
        absorb_prior_slide (grown is that record too), or None for a job that was not absorbed; absorbed is (inside,
        outside) from the call.  slide=None: every output is what it is without it."""
        if grow and absorb is None:
            raise ValueError("grow=True needs absorb=")
        if slide is not None:
            if not grow:
                raise ValueError("slide= needs grow=True")
            slide = float(slide)
            if not slide >= 0.0:
                raise ValueError("slide= is a margin in metres, at least 0: not %r" % (slide,))
        jobs = [tuple(j) for j in jobs]
        for v, j in enumerate(jobs):
            at = self.prior_origin(j[8]) if len(j) > 8 and j[8] is not None else None
            if at is not None:
                jobs[v] = j[:9] + (at,) + j[10:]
        return self._fleet_tick(refresh, jobs, pos, global_goals, home, [float(j[3]) for j in jobs], None, prev_wp, prev_dim, publish,
                                image_channels, reuse, world=True, crop=crop, throttle=throttle, check_kept=check_kept, absorb=absorb,
                                grow=(grow_limit, slide) if grow else None)

    def check_paths_slots(self, grid_ids, offsets, cells, shift=None):
        """Which kept paths do their slots' grids, as they are now, still allow (fxjps_check_paths_slots: one launch for
        the fleet, one wavefront per path): path q -- cells[offsets[q]:offsets[q + 1]], jump points as the plan calls return
        them -- is moved by the integer shift[q] (one pair, n x 2, or None) and walked unit step by unit step on the grid of
        slot grid_ids[q] with blocked() of scripts/jps1.py:14-31.  -> (verdict int32[n], seg int32[n], cell int32[n, 2]) as
        waypoints.check_path gives them path by path on get_grid_slot(grid_ids[q]).  Nothing of the handle changes."""
        ids = np.ascontiguousarray(grid_ids, dtype=np.int32).reshape(-1)
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        n = len(ids)
        if len(off) != n + 1:
            raise ValueError("%d offsets for %d paths" % (len(off), n))
        c = np.ascontiguousarray(np.asarray(cells, dtype=np.int32).reshape(-1, 2))
        if n and int(off.max()) > c.shape[0]:
            raise ValueError("the offsets name %d cells, there are %d" % (int(off.max()), c.shape[0]))
        if c.shape[0] == 0:
            c = np.zeros((1, 2), dtype=np.int32)  # (empty paths only: the pointer is still required)
        s = None if shift is None else np.ascontiguousarray(np.broadcast_to(np.asarray(shift, dtype=np.int32), (n, 2)))
        verdict, seg, cell = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros((n, 2), dtype=np.int32)
        self._chk(self._L.fxjps_check_paths_slots(self._h, n, _lib.ptr(off, C.c_int64), _lib.ptr(c, C.c_int32), _lib.ptr(ids, C.c_int32),
                                                  None if s is None else _lib.ptr(s, C.c_int32), _lib.ptr(verdict, C.c_int32),
                                                  _lib.ptr(seg, C.c_int32), _lib.ptr(cell, C.c_int32)))
        return verdict, seg, cell

    def fleet_tick_throttled(self, jobs, pos, global_goals, home, map_reso, map_o, throttle, prev_wp=None, prev_dim=None, publish=True,
                             image_channels=None, check_kept=True):
        """fleet_tick under the ccst node's replan throttle (global_planner_ccst.py:476): a vehicle is searched again only
        when it has moved more than 0.3 m since its last search, 0.3 s have passed, or nothing has been searched yet; on
        every other tick it republishes the outputs of its last search with a new pointw.z and its new map.  (A sibling
        method: fleet_tick's parameter list is pinned; fleet_tick_refresh and fleet_tick_world take throttle= / check_kept=
        themselves.)

        throttle: a replan.FleetThrottle(len(jobs)); it also keeps every vehicle's previous record, the caller keeps no
        state.  The maps of ALL vehicles are prepared and published as in fleet_tick.  due = throttle.due(pos); a vehicle
        without a previous record, or whose previous record has ok False, is due.  check_kept (the node does not do this:
        it republishes a kept path whatever the new map says): the live, not-due vehicles whose previous record holds a
        path are checked in ONE check_paths_slots call against this tick's slots, each path moved by shift = (previous
        origin - this tick's origin) / reso -- the previous origin being that of the tick the path was searched on, which
        the throttle keeps while the path is kept; a vehicle whose resolution changed, whose shift is farther than 1e-6 from a
        whole number of cells on either axis, or whose verdict is not PATH_VALID is forced due.  The due vehicles are
        planned and post-processed as fleet_tick does it, over the due subset (with reuse=True through replan_slots, which
        compares by query index: a subset that changes from tick to tick reuses less, never wrongly), then
        throttle.mark(due, pos[due]).

        -> fleet_tick's records with four further keys: cells (the path's int32 cells, so that it can be checked later),
        due (bool), forced (bool: due only because of the check) and path_check (the verdict, None if not checked).  A
        not-due vehicle's record takes status, cost, wp, dim, goal_out, ang_wp, n_kept, path, dir_path, dir_back and cells
        from its previous record and start, goal, map_d, shape, end_occu, origin, msg, image (and kept) from this tick;
        point is (wp[0], wp[1], z) with z by st:335 / ccst:559-562 from this tick's pos and end_occu; reused, where the
        records have it, is False."""
        return self._fleet_tick(False, jobs, pos, global_goals, home, map_reso, map_o, prev_wp, prev_dim, publish, image_channels,
                                throttle=throttle, check_kept=check_kept)

    @staticmethod
    def _point_z(variant, wp, goal_out, home, pos, end_occu):
        """pointw.z of st:335 / ccst:559-562 in the arithmetic of the tick-outputs call's host form (IEEE multiply, add,
        divide and sqrt; min is Python's: 1 iff 1 < r)."""
        f = np.float64
        with np.errstate(all="ignore"):
            def norm2(x, y):
                return np.sqrt(f(x) * f(x) + f(y) * f(y))
            if variant == 1 and (norm2(f(goal_out[0]) - f(pos[0]), f(goal_out[1]) - f(pos[1])) < 0.5 or end_occu != 0):
                return f(0.0)
            r = norm2(f(wp[0]) - f(home[0]), f(wp[1]) - f(home[1])) / norm2(f(goal_out[0]) - f(home[0]), f(goal_out[1]) - f(home[1]))
            r1 = f(1.0) if 1.0 < r else r
            return f(1.0) + r1 * (f(goal_out[2]) - f(1.0))

    def publish_slots(self, slots, msg=True, image_channels=None):
        """The fleet's publishing quarter of a tick in ONE call (fxjps_publish_slots): for every slot named what publish_map
        and / or snapshot_image would return were it the resident grid.  msg (bool) and image_channels (None, 1 or 3) are
        one value for all slots or one per slot.  -> per slot (data int8[W*H] or None, (W, H), image uint8 [H, W] /
        [H, W, 3] or None).  Two C calls: the extents, then the data.  A slot may be named more than once."""
        slots = [int(s) for s in slots]
        n = len(slots)
        msgs = list(msg) if isinstance(msg, (list, tuple, np.ndarray)) else [msg] * n
        chans = list(image_channels) if isinstance(image_channels, (list, tuple, np.ndarray)) else [image_channels] * n
        if len(msgs) != n or len(chans) != n:
            raise ValueError("msg and image_channels must be one value or one per slot")
        arr = (_lib.SlotPublish * max(n, 1))()
        for j, s in zip(arr, slots):
            j.slot = s
        self._chk(self._L.fxjps_publish_slots(self._h, arr, n))
        out = []
        for j, m, c in zip(arr, msgs, chans):
            data = np.empty(j.W * j.H, dtype=np.int8) if m else None
            img = None
            if c is not None:
                c = int(c)
                img = np.empty((j.H, j.W) if c == 1 else (j.H, j.W, c), dtype=np.uint8)
                j.image, j.channels = img.ctypes.data, c
            if data is not None:
                j.msg_data = data.ctypes.data
            out.append((data, (j.W, j.H), img))
        self._chk(self._L.fxjps_publish_slots(self._h, arr, n))
        return out

    def fleet_tick(self, jobs, pos, global_goals, home, map_reso, map_o, prev_wp=None, prev_dim=None, publish=True, image_channels=None):
        """One tick of a fleet, raw maps in, every node's outgoing messages out: prepare_slots, plan_batch_slots,
        waypoints.tick_outputs_slots on the resident paths and publish_slots, composed as INTEGRATION.md section 3d
        composes them.  jobs: as prepare_slots takes them, vehicle v in jobs[v]; pos, global_goals (n x 3), home (n x 2),
        map_reso (a scalar or n) and map_o (one pair or n x 2: the origin of the RAW map) per vehicle; prev_wp (n x 3) /
        prev_dim (n) as select_slots_batch takes them.  publish: bring out each live slot's OccupancyGrid data;
        image_channels: None, 1 or 3.  A vehicle whose job failed (the goal's row and column are fully occupied) is left out
        of the three later calls.  -> one dict per vehicle: ok, and when ok: status, cost, start, goal, map_d, shape,
        end_occu, origin (the shifted origin), wp, dim, goal_out, ang_wp, n_kept, point, path, dir_path, dir_back, msg,
        image; when not ok the other values are None."""
        return self._fleet_tick(False, jobs, pos, global_goals, home, map_reso, map_o, prev_wp, prev_dim, publish, image_channels)

    def fleet_tick_refresh(self, jobs, pos, global_goals, home, map_reso, map_o, prev_wp=None, prev_dim=None, publish=True, image_channels=None,
                           reuse=False, throttle=None, check_kept=True):
        """fleet_tick for the tick after: the maps are prepared through refresh_slots, so a vehicle whose prepared map is
        what its slot already holds keeps the slot's maps.  The same arguments, the same records, and in every live
        vehicle's record a further key, kept (bool).  reuse=True: the batch is planned through replan_slots, so a vehicle
        whose slot was kept and whose start and goal cells did not move is not searched again; its record says so in a
        further key, reused (bool).  Every other value is what reuse=False gives.  After set_slot_reuse("tiles") a vehicle
        whose slot changed only where its path's search did not read is not searched either: reused is True and a further
        key, reused_tiles (bool), says that this was why.  throttle (a replan.FleetThrottle) / check_kept: the ccst
        node's replan throttle, as fleet_tick_throttled describes it; with throttle=None nothing of that runs and the
        records are what they were."""
        return self._fleet_tick(True, jobs, pos, global_goals, home, map_reso, map_o, prev_wp, prev_dim, publish, image_channels, reuse,
                                throttle=throttle, check_kept=check_kept)

    def _fleet_tick(self, refresh, jobs, pos, global_goals, home, map_reso, map_o, prev_wp, prev_dim, publish, image_channels, reuse=False,
                    world=False, crop=False, throttle=None, check_kept=True, absorb=None, grow=None):
        if throttle is not None:
            return self._fleet_tick_throttled(refresh, jobs, pos, global_goals, home, map_reso, map_o, prev_wp, prev_dim, publish, image_channels,
                                              reuse, world, crop, throttle, check_kept, absorb, grow)
        from . import waypoints
        jobs = list(jobs)
        n = len(jobs)
        pos = np.asarray(pos, dtype=np.float64).reshape(n, 3)
        goals = np.asarray(global_goals, dtype=np.float64).reshape(n, 3)
        home = np.broadcast_to(np.asarray(home, dtype=np.float64), (n, 2))
        reso = np.broadcast_to(np.asarray(map_reso, dtype=np.float64), (n,))
        orig = None if world else np.broadcast_to(np.asarray(map_o, dtype=np.float64), (n, 2))
        keys = ("status", "cost", "start", "goal", "map_d", "shape", "end_occu", "origin", "wp", "dim", "goal_out", "ang_wp", "n_kept", "point",
                "path", "dir_path", "dir_back", "msg", "image")
        recs = [dict({"ok": False}, **{k: None for k in keys}) for _ in range(n)]
        if crop:  # (status and the crop record lie behind the world call's tuple: they are taken off it here)
            outs = self.refresh_slots_cropped(jobs) if refresh else self.prepare_slots_cropped(jobs)
            for v in range(n):
                recs[v]["not_planned"] = outs[v][-2] == _lib.JOB_NOT_PLANNED
            self._tick_absorb(absorb, jobs, outs, True, recs, grow)
            outs = [o[:-2] for o in outs]
        elif world:  # (the call's own origin, canvas_shape and canvas_o lie behind the existing tuple)
            outs = self.refresh_slots_world(jobs) if refresh else self.prepare_slots_world(jobs)
            self._tick_absorb(absorb, jobs, outs, False, recs, grow)
        else:
            outs = self.refresh_slots(jobs) if refresh else self.prepare_slots(jobs)
        variant_at = 7 if world else 5
        live = [v for v in range(n) if outs[v][5]]
        if not live:
            return recs
        slots = [int(jobs[v][0]) for v in live]
        offsets, _, cost, status, reused = self._plan_slots(reuse, slots, [outs[v][0] for v in live], [outs[v][1] for v in live], 2, None)
        origin = [outs[v][-3] if world else Planner.shifted_origin(orig[v], outs[v][2], reso[v]) for v in live]
        pw = pd = None
        if prev_wp is not None:
            pw = np.asarray(prev_wp, dtype=np.float64).reshape(n, 3)[live]
            pd = np.asarray(prev_dim, dtype=np.int32).reshape(n)[live]
        wp, dim, gout, ang, nk, point, paths, dirs, back = waypoints.tick_outputs_slots(
            self, [jobs[v][variant_at] for v in live], [outs[v][0] for v in live], reso[live], origin, pos[live], goals[live], home[live],
            [outs[v][4] for v in live], pw, pd, offsets=offsets)
        pub = self.publish_slots(slots, msg=publish, image_channels=image_channels) if (publish or image_channels is not None) else None
        for i, v in enumerate(live):
            o = outs[v]
            recs[v].update(ok=True, status=int(status[i]), cost=float(cost[i]), start=o[0], goal=o[1], map_d=o[2], shape=o[3], end_occu=o[4],
                           origin=origin[i], wp=wp[i, :dim[i]], dim=int(dim[i]), goal_out=gout[i], ang_wp=float(ang[i]), n_kept=int(nk[i]),
                           point=point[i], path=paths[i], dir_path=dirs[i], dir_back=int(back[i]))
            if pub is not None:
                recs[v].update(msg=pub[i][0], image=pub[i][2])
            if refresh:
                recs[v]["kept"] = o[6]
            if reuse:
                recs[v]["reused"] = bool(reused[i])
                if self._slot_reuse == 1:
                    recs[v]["reused_tiles"] = int(reused[i]) == 2
        return recs

    def _fleet_tick_throttled(self, refresh, jobs, pos, global_goals, home, map_reso, map_o, prev_wp, prev_dim, publish, image_channels,
                              reuse, world, crop, throttle, check_kept, absorb=None, grow=None):
        """_fleet_tick under a replan.FleetThrottle (fleet_tick_throttled's docstring): the same calls in the same order, the
        plan and the tick outputs over the due vehicles only, one check_paths_slots call in front of them."""
        from . import waypoints
        jobs = list(jobs)
        n = len(jobs)
        if throttle.n != n:
            raise ValueError("the throttle is for %d vehicles, the tick has %d" % (throttle.n, n))
        pos = np.asarray(pos, dtype=np.float64).reshape(n, 3)
        goals = np.asarray(global_goals, dtype=np.float64).reshape(n, 3)
        home = np.broadcast_to(np.asarray(home, dtype=np.float64), (n, 2))
        reso = np.broadcast_to(np.asarray(map_reso, dtype=np.float64), (n,))
        orig = None if world else np.broadcast_to(np.asarray(map_o, dtype=np.float64), (n, 2))
        keys = ("status", "cost", "start", "goal", "map_d", "shape", "end_occu", "origin", "wp", "dim", "goal_out", "ang_wp", "n_kept", "point",
                "path", "dir_path", "dir_back", "msg", "image", "cells", "path_check")
        recs = [dict({"ok": False, "due": True, "forced": False}, **{k: None for k in keys}) for _ in range(n)]
        # ---- every vehicle's map, as without a throttle
        if crop:
            outs = self.refresh_slots_cropped(jobs) if refresh else self.prepare_slots_cropped(jobs)
            for v in range(n):
                recs[v]["not_planned"] = outs[v][-2] == _lib.JOB_NOT_PLANNED
            self._tick_absorb(absorb, jobs, outs, True, recs, grow)
            outs = [o[:-2] for o in outs]
        elif world:
            outs = self.refresh_slots_world(jobs) if refresh else self.prepare_slots_world(jobs)
            self._tick_absorb(absorb, jobs, outs, False, recs, grow)
        else:
            outs = self.refresh_slots(jobs) if refresh else self.prepare_slots(jobs)
        variant_at = 7 if world else 5
        variant = [{"st": 0, "ccst": 1}[j[variant_at]] if isinstance(j[variant_at], str) else int(j[variant_at]) for j in jobs]
        live = [v for v in range(n) if outs[v][5]]
        origin = {v: outs[v][-3] if world else Planner.shifted_origin(orig[v], outs[v][2], reso[v]) for v in live}
        # ---- who is due: the node's condition, then the kept paths against this tick's slots
        prev = throttle.records
        due = throttle.due(pos)
        for v in range(n):
            if prev[v] is None or not prev[v]["ok"]:
                due[v] = True
        if check_kept:
            ask, shifts = [], []
            for v in live:
                if due[v] or prev[v]["status"] <= 0:
                    continue
                # (the kept cells are cells of the grid the vehicle was last SEARCHED on: the previous record's origin when that
                # was a search tick, and the throttle's copy of it on every later one)
                s = (throttle.search_origin[v] - np.asarray(origin[v], dtype=np.float64)) / reso[v]
                if throttle.search_reso[v] != reso[v] or not np.all(np.abs(s - np.rint(s)) <= 1e-6):
                    due[v] = recs[v]["forced"] = True
                    continue
                ask.append(v)
                shifts.append(np.rint(s).astype(np.int32))
            if ask:
                off = np.concatenate([[0], np.cumsum([len(prev[v]["cells"]) for v in ask])]).astype(np.int64)
                verdict, _, _ = self.check_paths_slots([int(jobs[v][0]) for v in ask], off, np.concatenate([prev[v]["cells"] for v in ask]),
                                                       np.array(shifts, dtype=np.int32))
                for i, v in enumerate(ask):
                    recs[v]["path_check"] = int(verdict[i])
                    if verdict[i] != _lib.PATH_VALID:
                        due[v] = recs[v]["forced"] = True
        # ---- the due vehicles: planned and post-processed as without a throttle
        go = [v for v in live if due[v]]
        if go:
            offsets, cells, cost, status, reused = self._plan_slots(reuse, [int(jobs[v][0]) for v in go], [outs[v][0] for v in go],
                                                                    [outs[v][1] for v in go], 2, None)
            pw = pd = None
            if prev_wp is not None:
                pw = np.asarray(prev_wp, dtype=np.float64).reshape(n, 3)[go]
                pd = np.asarray(prev_dim, dtype=np.int32).reshape(n)[go]
            wp, dim, gout, ang, nk, point, paths, dirs, back = waypoints.tick_outputs_slots(
                self, [variant[v] for v in go], [outs[v][0] for v in go], reso[go], [origin[v] for v in go], pos[go], goals[go], home[go],
                [outs[v][4] for v in go], pw, pd, offsets=offsets)
            for i, v in enumerate(go):
                recs[v].update(status=int(status[i]), cost=float(cost[i]), wp=wp[i, :dim[i]], dim=int(dim[i]), goal_out=gout[i], ang_wp=float(ang[i]),
                               n_kept=int(nk[i]), point=point[i], path=paths[i], dir_path=dirs[i], dir_back=int(back[i]),
                               cells=cells[int(offsets[i]):int(offsets[i + 1])].copy())
                if reuse:
                    recs[v]["reused"] = bool(reused[i])
                    if self._slot_reuse == 1:
                        recs[v]["reused_tiles"] = int(reused[i]) == 2
            throttle.mark(go, pos[go])
            throttle.search_origin[go] = [origin[v] for v in go]
            throttle.search_reso[go] = reso[go]
        pub = None
        if live and (publish or image_channels is not None):
            pub = self.publish_slots([int(jobs[v][0]) for v in live], msg=publish, image_channels=image_channels)
        for i, v in enumerate(live):
            o, r = outs[v], recs[v]
            r.update(ok=True, due=bool(due[v]), start=o[0], goal=o[1], map_d=o[2], shape=o[3], end_occu=o[4], origin=origin[v])
            if pub is not None:
                r.update(msg=pub[i][0], image=pub[i][2])
            if refresh:
                r["kept"] = o[6]
            if not due[v]:  # the outputs of the vehicle's last search, pointw.z anew (ccst:559-562 / st:335)
                p = prev[v]
                for k in ("status", "cost", "wp", "dim", "goal_out", "ang_wp", "n_kept", "path", "dir_path", "dir_back", "cells"):
                    r[k] = p[k]
                r["point"] = np.array([p["wp"][0], p["wp"][1], Planner._point_z(variant[v], p["wp"], p["goal_out"], home[v], pos[v], o[4])])
                if reuse:
                    r["reused"] = False
                    if self._slot_reuse == 1:
                        r["reused_tiles"] = False
        throttle.records = list(recs)
        return recs

    def plan_batch_slots(self, grid_ids, starts, goals, hchoice=2, max_path_len=None):
        """plan_batch with a grid per query: query q runs on the grid of slot grid_ids[q].  -> (offsets, cells, cost,
        status) as plan_batch.  max_path_len=None: the default slot of the largest grid named, grown when a path needs it."""
        return self._plan_slots(False, grid_ids, starts, goals, hchoice, max_path_len)[:4]

    def replan_slots(self, grid_ids, starts, goals, hchoice=2, max_path_len=None):
        """plan_batch_slots for the tick after (fxjps_replan_slots): a query whose slot, start and goal are those of the
        previous replan_slots call, on a slot nothing has written since, hands back its stored path without a search.
        -> (offsets, cells, cost, status, reused); reused: the call's flag per query (int32): 0 searched, 1 handed back
        because nothing wrote its slot, 2 (only after set_slot_reuse("tiles")) handed back although its slot changed,
        because no changed cell touches a tile its search read.  The results are byte for byte those of
        plan_batch_slots.  A max_path_len that grows makes that retry a full search."""
        return self._plan_slots(True, grid_ids, starts, goals, hchoice, max_path_len)

    SLOT_REUSE_MODES = {"generation": 0, "tiles": 1}

    def set_slot_reuse(self, mode):
        """Which stored paths replan_slots hands back (fxjps_set_slot_reuse): "generation" (the default: those of slots
        nothing has written) or "tiles" (also those of slots whose refresh changed bytes only in read-set tiles the stored
        search did not read).  A change of mode drops the stored results."""
        if mode not in self.SLOT_REUSE_MODES:
            raise ValueError("mode must be 'generation' or 'tiles'")
        self._chk(self._L.fxjps_set_slot_reuse(self._h, self.SLOT_REUSE_MODES[mode]))
        self._slot_reuse = self.SLOT_REUSE_MODES[mode]

    def debug_slot_tiles(self, slot):
        """The changed-tile record of a slot (fxjps_debug_slot_tiles): -> (uint64[128], tsh, valid).  Tile (tx, ty) is
        marked iff bit tx of [ty] and bit ty of [64 + tx] are set."""
        out = np.zeros(128, dtype=np.uint64)
        tsh, valid = C.c_int32(-1), C.c_int32(-1)
        self._chk(self._L.fxjps_debug_slot_tiles(self._h, int(slot), _lib.ptr(out, C.c_uint64), C.byref(tsh), C.byref(valid)))
        return out, tsh.value, bool(valid.value)

    def debug_slot_read_sets(self):
        """The read sets kept with the stored results of the last replan_slots under the tile rule
        (fxjps_debug_slot_read_sets): -> (uint64[nq, 128], tsh int32[nq], have bool[nq]), laid out as debug_read_sets'."""
        n = self._slot_nq  # (of the last replan_slots)
        out = np.zeros((n, 128), dtype=np.uint64)
        tsh = np.zeros(n, dtype=np.int32)
        have = np.zeros(n, dtype=np.int32)
        self._chk(self._L.fxjps_debug_slot_read_sets(self._h, _lib.ptr(out, C.c_uint64), n, _lib.ptr(tsh, C.c_int32), _lib.ptr(have, C.c_int32)))
        return out, tsh, have.astype(bool)

    def _plan_slots(self, replan, grid_ids, starts, goals, hchoice, max_path_len):
        ids = np.ascontiguousarray(grid_ids, dtype=np.int32).reshape(-1)
        starts = np.ascontiguousarray(starts, dtype=np.int32).reshape(-1, 2)
        goals = np.ascontiguousarray(goals, dtype=np.int32).reshape(-1, 2)
        if len(starts) != len(goals) or len(ids) != len(starts):
            raise ValueError("grid_ids, starts and goals lengths differ")
        if hchoice not in (1, 2):
            raise TypeError("unsupported operand type(s) for +: 'float' and 'NoneType' (hchoice must be 1 or 2)")
        n = len(starts)
        auto = max_path_len is None
        if auto:  # (each referenced slot's own default and bound, the largest of them)
            mpl, limit = 1, 1
            for k in np.unique(ids):  # (an empty or unknown slot is the call's to refuse)
                w, h = C.c_int32(), C.c_int32()
                if 0 <= k < _lib.MAX_GRID_SLOTS and self._L.fxjps_get_grid_slot(self._h, int(k), None, C.byref(w), C.byref(h)) == 0:
                    W, H = w.value, h.value
                    mpl = max(mpl, int(min(W * H + 1, max(256, 4 * max(W, H)))))
                    limit = max(limit, W * H + 1)
        else:
            mpl = int(max_path_len)
        while True:
            offsets = np.zeros(n + 1, dtype=np.int64)
            status = np.zeros(n, dtype=np.int32)
            cost = np.zeros(n, dtype=np.float64)
            secs = C.c_double(0.0)
            reused = np.zeros(n, dtype=np.int32)
            if replan:
                self._slot_nq = n
                self._chk(self._L.fxjps_replan_slots(self._h, _lib.ptr(ids, C.c_int32), _lib.ptr(starts, C.c_int32),
                                                     _lib.ptr(goals, C.c_int32), n, int(hchoice), mpl, _lib.ptr(offsets, C.c_int64),
                                                     None, 0, _lib.ptr(status, C.c_int32), _lib.ptr(cost, C.c_double),
                                                     _lib.ptr(reused, C.c_int32), C.byref(secs)))
            else:
                self._chk(self._L.fxjps_plan_batch_slots_csr(self._h, _lib.ptr(ids, C.c_int32), _lib.ptr(starts, C.c_int32),
                                                             _lib.ptr(goals, C.c_int32), n, int(hchoice), mpl, _lib.ptr(offsets, C.c_int64),
                                                             None, 0, _lib.ptr(status, C.c_int32), _lib.ptr(cost, C.c_double), C.byref(secs)))
            cells = np.empty((int(offsets[n]), 2), dtype=np.int32)
            if offsets[n] > 0:
                self._chk(self._L.fxjps_last_cells(self._h, _lib.ptr(cells, C.c_int32), int(offsets[n])))
            if auto and mpl < limit and (status == _lib.Q_PATH_TOO_LONG).any():
                mpl = min(limit, mpl * 8)  # rare: a path with more jump points than the default slot
                continue
            break
        self.last_seconds = secs.value
        return offsets, cells, cost, status, reused

    # -- streaming replan (persistent goals, one call per frame)
    def set_queries(self, starts, goals, hchoice=2, max_path_len=None):
        """Store the persistent (start, goal) set that replan_frame plans every frame."""
        if self.shape is None:
            raise FxjpsError(_lib.E_NOGRID, "set_queries before set_grid")
        starts = np.ascontiguousarray(starts, dtype=np.int32).reshape(-1, 2)
        goals = np.ascontiguousarray(goals, dtype=np.int32).reshape(-1, 2)
        if len(starts) != len(goals):
            raise ValueError("starts and goals lengths differ")
        if hchoice not in (1, 2):
            raise TypeError("unsupported operand type(s) for +: 'float' and 'NoneType' (hchoice must be 1 or 2)")
        mpl = self.default_max_path_len() if max_path_len is None else int(max_path_len)
        self._chk(self._L.fxjps_set_queries(self._h, _lib.ptr(starts, C.c_int32), _lib.ptr(goals, C.c_int32), len(starts),
                                            int(hchoice), mpl))
        self._nq = len(starts)

    def replan_frame(self, xy=None, val=None):
        """One frame: apply the cell updates (xy int32[n, 2], val uint8[n]; may be empty), rebuild the maps, plan the
        stored queries.  -> (offsets, cells, cost, status) as plan_batch."""
        if xy is None:
            xy, val = np.zeros((0, 2), np.int32), np.zeros(0, np.uint8)
        xy = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1, 2)
        val = np.ascontiguousarray(val, dtype=np.uint8).reshape(-1)
        if len(val) != len(xy):
            raise ValueError("xy and val lengths differ")
        n = self._nq
        self._resident = None
        offsets = np.zeros(n + 1, dtype=np.int64)
        status = np.zeros(n, dtype=np.int32)
        cost = np.zeros(n, dtype=np.float64)
        secs = C.c_double(0.0)
        self._chk(self._L.fxjps_replan_frame(self._h, _lib.ptr(xy, C.c_int32), _lib.ptr(val, C.c_uint8), len(val),
                                             _lib.ptr(offsets, C.c_int64), None, 0, _lib.ptr(status, C.c_int32),
                                             _lib.ptr(cost, C.c_double), C.byref(secs)))
        cells = np.empty((int(offsets[n]), 2), dtype=np.int32)
        if offsets[n] > 0:
            self._chk(self._L.fxjps_last_cells(self._h, _lib.ptr(cells, C.c_int32), int(offsets[n])))
        self.last_seconds = secs.value
        return offsets, cells, cost, status

    def plan_one(self, start, goal, hchoice=2):
        """One query -- the node's call, once per tick -- without the per-call allocations of plan_batch: the arrays of a
        one-query call are kept, the cells come back with the call itself (no sizing call).  -> (status, cost, cells
        int32[n, 2] view valid until the next call)."""
        if self.shape is None:
            raise FxjpsError(_lib.E_NOGRID, "plan before set_grid")
        if hchoice not in (1, 2):
            raise TypeError("unsupported operand type(s) for +: 'float' and 'NoneType' (hchoice must be 1 or 2)")
        mpl = self.default_max_path_len()
        o = getattr(self, "_one", None)
        if o is None or o["mpl"] != mpl:
            o = {"mpl": mpl, "s": np.zeros((1, 2), np.int32), "g": np.zeros((1, 2), np.int32), "off": np.zeros(2, np.int64),
                 "st": np.zeros(1, np.int32), "cost": np.zeros(1, np.float64), "cells": np.zeros((mpl, 2), np.int32), "secs": C.c_double(0.0)}
            o["args"] = (_lib.ptr(o["s"], C.c_int32), _lib.ptr(o["g"], C.c_int32), _lib.ptr(o["off"], C.c_int64), _lib.ptr(o["cells"], C.c_int32),
                         _lib.ptr(o["st"], C.c_int32), _lib.ptr(o["cost"], C.c_double), C.byref(o["secs"]))
            self._one = o
        o["s"][0, 0], o["s"][0, 1] = start[0], start[1]
        o["g"][0, 0], o["g"][0, 1] = goal[0], goal[1]
        a = o["args"]
        self._chk(self._L.fxjps_plan_batch_csr(self._h, a[0], a[1], 1, int(hchoice), mpl, a[2], a[3], mpl, a[4], a[5], a[6]))
        st = int(o["st"][0])
        if st == _lib.Q_PATH_TOO_LONG and mpl < self.shape[0] * self.shape[1] + 1:  # (rare: the general path grows the slot)
            offsets, cells, cost, status = self.plan_batch([start], [goal], hchoice)
            return int(status[0]), float(cost[0]), cells[offsets[0]:offsets[1]]
        self.last_seconds = o["secs"].value
        return st, float(o["cost"][0]), o["cells"][:max(st, 0)]

    def plan(self, start, goal, hchoice=2):
        """plan(start, goal) -> waypoint list [(x, y), ...] (jump points, start and
        goal inclusive); [] when there is no path."""
        st, cost, cells = self.plan_one(start, goal, hchoice)
        self.last_cost = cost
        if st == _lib.Q_BAD_START:
            raise IndexError("start %r is outside the %dx%d grid" % (tuple(start), self.shape[0], self.shape[1]))
        if st < 0:
            raise FxjpsError(st, "query failed")
        return [(int(x), int(y)) for x, y in cells]

    def timing(self):
        t = _lib.Timing()
        self._chk(self._L.fxjps_last_timing(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in _lib.Timing._fields_}

    def timing_per_context(self):
        """Per context of the handle (one per entry of `devices`): device, queries of its shard, search-kernel ms,
        resident wavefronts of the last batch."""
        out = []
        for r in range(len(self.devices)):
            dev, nq, ms, wv = C.c_int32(), C.c_int64(), C.c_double(), C.c_int64()
            self._chk(self._L.fxjps_last_timing_device(self._h, r, C.byref(dev), C.byref(nq), C.byref(ms), C.byref(wv)))
            out.append({"device": dev.value, "queries": nq.value, "kernel_ms": ms.value, "waves": wv.value})
        return out

    def comm_info(self):
        """-> {"contexts", "devices", "rccl_ranks"}: rccl_ranks is ncclCommCount of the handle's communicator (0 while
        no collective has run: one device, or contexts sharing a device)."""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._chk(self._L.fxjps_comm_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"contexts": a.value, "devices": b.value, "rccl_ranks": c.value}

    def set_memory_share(self, handles_per_device):
        """This handle is one of `handles_per_device` on its device(s): scratch pools and resident wavefronts are sized
        for that share (FramePipeline sets it)."""
        self._chk(self._L.fxjps_set_memory_share(self._h, int(handles_per_device)))

    # -- test hooks
    def selftest_sqrt(self, n0, n1):
        out = np.empty(n1 - n0, dtype=np.float64)
        self._chk(self._L.fxjps_selftest_sqrt(self._h, n0, n1, _lib.ptr(out, C.c_double)))
        return out

    def selftest_wavemin(self, rounds=4096, seed=1):
        bad = C.c_int64(-1)
        self._chk(self._L.fxjps_selftest_wavemin(self._h, rounds, seed, C.byref(bad)))
        return bad.value

    def selftest_openlist(self, keys_f, keys_x, step_pops, step_off, banded=False, far_cap=8192, near_max=512, delta0=2.0):
        """Run a push / pop script through the open list of the search kernel (fxjps_selftest_openlist).
        -> (popped f bits uint64[n], popped x uint32[n], pushed-entry index uint32[n], pops per step uint32[nsteps],
        {fail, far_refills, slow_pops})"""
        kf = np.ascontiguousarray(keys_f, dtype=np.uint64)
        kx = np.ascontiguousarray(keys_x, dtype=np.uint32)
        sp = np.ascontiguousarray(step_pops, dtype=np.uint32)
        so = np.ascontiguousarray(step_off, dtype=np.uint32)
        n, ns = len(kf), len(sp)
        of, ox, os_ = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        ok, info = np.zeros(max(ns, 1), np.uint32), np.zeros(8, np.uint32)
        self._chk(self._L.fxjps_selftest_openlist(self._h, int(bool(banded)), int(far_cap), int(near_max), float(delta0),
                                                  _lib.ptr(kf, C.c_uint64), _lib.ptr(kx, C.c_uint32), n, _lib.ptr(sp, C.c_uint32),
                                                  _lib.ptr(so, C.c_uint32), ns, _lib.ptr(of, C.c_uint64), _lib.ptr(ox, C.c_uint32),
                                                  _lib.ptr(os_, C.c_uint32), _lib.ptr(ok, C.c_uint32), _lib.ptr(info, C.c_uint32)))
        t = int(info[0])
        return of[:t], ox[:t], os_[:t], ok[:ns], {"fail": int(info[1]), "far_refills": int(info[2]), "slow_pops": int(info[3]), "held": [int(v) for v in info[4:8]]}

    def debug_maps(self):
        """The derived device maps (fxjps_debug_read_maps): {"bm": uint64[4, LINES, WORDS, 2], "ci": uint16[W+2, H+2],
        "comp": int32[W, H] (union-find parent links), "nb8": uint8[W+2, H+2], "dbm": uint64[4, W+H+3, WORDS, 2] (the
        diagonal scan words), "jd": uint16[W+2, H+2, 8] (the jump distances)}."""
        W, H = self.shape
        return self._read_maps(W, H, lambda which, buf, cap, nb: self._L.fxjps_debug_read_maps(self._h, which, buf, cap, nb))

    def debug_slot_maps(self, slot):
        """The derived device maps of grid slot `slot` (fxjps_debug_read_slot_maps), as debug_maps() returns them."""
        W, H = C.c_int32(), C.c_int32()
        self._chk(self._L.fxjps_get_grid_slot(self._h, int(slot), None, C.byref(W), C.byref(H)))
        return self._read_maps(W.value, H.value,
                               lambda which, buf, cap, nb: self._L.fxjps_debug_read_slot_maps(self._h, int(slot), which, buf, cap, nb))

    def debug_slot_context(self, context, slot):
        """The copy of grid slot `slot` on context `context` (fxjps_debug_read_slot_context): -> (uint8 [W][H] occupancy,
        the derived maps as debug_maps() returns them)."""
        W, H = C.c_int32(), C.c_int32()
        self._chk(self._L.fxjps_get_grid_slot(self._h, int(slot), None, C.byref(W), C.byref(H)))
        occ = np.empty((W.value, H.value), dtype=np.uint8)
        nb = C.c_int64(0)
        self._chk(self._L.fxjps_debug_read_slot_context(self._h, int(context), int(slot), -1, occ.ctypes.data_as(C.c_void_p), occ.nbytes, C.byref(nb)))
        assert nb.value == occ.nbytes, (nb.value, occ.nbytes)
        return occ, self._read_maps(W.value, H.value, lambda which, buf, cap, n_: self._L.fxjps_debug_read_slot_context(
            self._h, int(context), int(slot), which, buf, cap, n_))

    def _read_maps(self, W, H, read):
        PW, PH = W + 2, H + 2
        NS = (PH + 63) & ~63
        LINES = max(PW, PH)
        WORDS = (LINES + 63) // 64
        out = {}
        for which, name, dt, shape in ((0, "bm", np.uint64, (4, LINES, WORDS, 2)), (1, "ci", np.uint16, (PW, NS)), (2, "comp", np.int32, (W, H)),
                                       (3, "nb8", np.uint8, (PW, NS)), (4, "dbm", np.uint64, (4, PW + PH - 1, WORDS, 2)), (5, "jd", np.uint16, (PW, NS, 8))):
            a = np.zeros(shape, dtype=dt)
            nb = C.c_int64(0)
            self._chk(read(which, a.ctypes.data_as(C.c_void_p), a.nbytes, C.byref(nb)))
            assert nb.value == a.nbytes, (name, nb.value, a.nbytes)
            out[name] = a[:, :PH] if name in ("ci", "nb8", "jd") else a
        # (lines the kernels neither write nor read -- the +-x scans have a line per padded y, the +-y scans per padded
        # x, the array has max(PW, PH) of each -- hold whatever the allocation held)
        out["bm"][0:2, PH:] = 0
        out["bm"][2:4, PW:] = 0
        return out

    def debug_read_sets(self):
        """The read sets of the stored results of replan_frame (fxjps_debug_read_sets): -> (uint64[nq, 128], tsh).  Tile
        (tx, ty) of (1 << tsh)^2 cells is marked for query q iff bit tx of [q, ty] or bit ty of [q, 64 + tx] is set."""
        out = np.zeros((self._nq, 128), dtype=np.uint64)
        tsh = C.c_int32(-1)
        self._chk(self._L.fxjps_debug_read_sets(self._h, _lib.ptr(out, C.c_uint64), self._nq, C.byref(tsh)))
        return out, tsh.value

    def debug_qstat(self, nq):
        """The per-query diagnostics of the last batch on the first context (fxjps_debug_qstat; FXJPS_QSTAT=1 must be in
        the environment before the first planning call of the process): -> uint64[nq, 4], per query start, end (100 MHz
        ticks), pops, wavefront (low 24 bits) | shader-clock cycles of the search << 24.  A query that was not searched
        has a zero row."""
        out = np.zeros((int(nq), 4), dtype=np.uint64)
        self._chk(self._L.fxjps_debug_qstat(self._h, _lib.ptr(out, C.c_uint64), int(nq)))
        return out

    def debug_counters(self):
        """The raw device counters of the last batch on the first context (fxjps_debug_counters): -> uint64[64].  [0] pops,
        [1] pushes, [2] far-tier refills, [3] slow pops in every build; the rest is filled by the diagnostic build
        (-DFXJPS_PROF) only and is zero otherwise: DBG_COUNT(k) of csrc/fxjps_kernels.hip.inc is [k]."""
        out = np.zeros(64, dtype=np.uint64)
        self._chk(self._L.fxjps_debug_counters(self._h, _lib.ptr(out, C.c_uint64)))
        return out

    def debug_nbmask(self):
        W, H = self.shape
        buf = np.empty((W + 2, H + 2), dtype=np.uint8)
        self._chk(self._L.fxjps_debug_read_nbmask(self._h, _lib.ptr(buf, C.c_uint8)))
        return buf


_default = None


def default_planner():
    """Process-wide planner on device 0 (what the jps1 shim uses)."""
    global _default
    if _default is None:
        _default = Planner([0])
    return _default


def plan(grid, start, goal, hchoice=2):
    """north_star call surface: plan(grid, start, goal) -> waypoint list."""
    p = default_planner()
    p.set_grid(grid)
    return p.plan(start, goal, hchoice)


def plan_batch(grid, starts, goals, hchoice=2, max_path_len=None):
    p = default_planner()
    p.set_grid(grid)
    return p.plan_batch(starts, goals, hchoice, max_path_len)
