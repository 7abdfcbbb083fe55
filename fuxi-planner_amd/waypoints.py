"""Waypoint selection after a plan: the step the reference's nodes run on the path that
jps1.method returned -- scripts/global_planner_st.py:292-327 and scripts/global_planner_ccst.py:487-526 (with
map_line_col, :258-283).  Thin wrappers over the C ABI (fxjps_waypoint_st / fxjps_waypoint_ccst); the functions are
host code and need no device.

    path1 = jps1.method(mapu, tuple(map_start), tuple(map_goal), 2)
    if path1[0] is not 0:
        wp, global_goal, ang_wp = waypoints.select_st(path1[0], map_start, map_reso, map_o, (px, py, pz), global_goal,
                                                      end_occu, prev_wp=wp)                          # st
        wp, kept, global_goal = waypoints.select_ccst(path1[0], mapu, map_reso, map_o, (px, py, pz), global_goal,
                                                      end_occu, return_goal=True)                  # ccst
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from .planner import as_occ


_HOST_LIB = None  # test hook: a library with the host-only entry points (e.g. the sanitizer build); None = libfxjps.so


def _L():
    return _HOST_LIB if _HOST_LIB is not None else _lib.load()


def _cells(path):
    c = np.ascontiguousarray(np.asarray(path, dtype=np.int32).reshape(-1, 2))
    if c.shape[0] < 1:
        raise ValueError("empty path")
    return c


def _vec(v, n):
    a = np.ascontiguousarray(np.asarray(v, dtype=np.float64).ravel())
    if a.shape[0] != n:
        raise ValueError("expected %d components" % n)
    return a


def select_st(path, map_start, map_reso, map_o, pos, global_goal, end_occu=0, prev_wp=None, dis_wp_tre=2.0,
              ang_wp_tre=math.pi / 4):
    """global_planner_st.py:292-327.  -> (wp ndarray of 2 or 3 components, global_goal ndarray[3], ang_wp)."""
    L = _L()
    c = _cells(path)
    ms = np.ascontiguousarray(np.asarray(map_start, dtype=np.int32).ravel())
    o, p, g = _vec(map_o, 2), _vec(pos, 3), _vec(global_goal, 3)
    pw = None if prev_wp is None else np.ascontiguousarray(np.asarray(prev_wp, dtype=np.float64).ravel())
    wp = np.zeros(3)
    gout = np.zeros(3)
    dim = C.c_int32(0)
    ang = C.c_double(0.0)
    rc = L.fxjps_waypoint_st(_lib.ptr(c, C.c_int32), c.shape[0], _lib.ptr(ms, C.c_int32), float(map_reso), _lib.ptr(o, C.c_double),
                             _lib.ptr(p, C.c_double), _lib.ptr(g, C.c_double), int(end_occu), float(dis_wp_tre), float(ang_wp_tre),
                             None if pw is None else _lib.ptr(pw, C.c_double), 0 if pw is None else int(pw.shape[0]),
                             _lib.ptr(wp, C.c_double), C.byref(dim), _lib.ptr(gout, C.c_double), C.byref(ang))
    if rc != 0:
        raise _lib.FxjpsError(rc, "fxjps_waypoint_st: bad argument")
    return wp[:dim.value].copy(), gout, ang.value


def select_ccst(path, mapu, map_reso, map_o, pos, global_goal, end_occu=0, return_goal=False):
    """global_planner_ccst.py:487-544.  -> (wp ndarray[3], kept cells int32[m, 2]) [+ global_goal ndarray[3] after the block
    when return_goal]."""
    L = _L()
    c = _cells(path)
    occ = as_occ(mapu)
    o, p, g = _vec(map_o, 2), _vec(pos, 3), _vec(global_goal, 3)
    wp = np.zeros(3)
    gout = np.zeros(3)
    kept = np.zeros((c.shape[0], 2), dtype=np.int32)
    nk = C.c_int32(0)
    rc = L.fxjps_waypoint_ccst(_lib.ptr(c, C.c_int32), c.shape[0], _lib.ptr(occ, C.c_uint8), occ.shape[0], occ.shape[1], float(map_reso),
                               _lib.ptr(o, C.c_double), _lib.ptr(p, C.c_double), _lib.ptr(g, C.c_double), int(end_occu),
                               _lib.ptr(wp, C.c_double), _lib.ptr(gout, C.c_double), _lib.ptr(kept, C.c_int32), C.byref(nk))
    if rc != 0:
        raise _lib.FxjpsError(rc, "fxjps_waypoint_ccst: bad argument")
    if return_goal:
        return wp, kept[:nk.value].copy(), gout
    return wp, kept[:nk.value].copy()


def check_path(path, occ, shift=None):
    """Does the grid still allow a kept path (fxjps_check_path, host code): every unit step of the jump-point path, moved by
    the integer `shift` (sx, sy) first, judged by blocked() of scripts/jps1.py:14-31 on occ -- the uint8 [W][H] bytes a slot
    holds (get_grid_slot), obstacle iff non-zero; an array of another type counts as != 0.  The path may be empty.
    -> (verdict, seg, (x, y)): _lib.PATH_VALID / PATH_EMPTY (seg -1, cell (-1, -1)), or PATH_BLOCKED / PATH_OUTSIDE /
    PATH_MALFORMED with the segment of the first failing step and that step's target cell in shifted coordinates
    (malformed: the segment's first cell)."""
    L = _L()
    c = np.ascontiguousarray(np.asarray(path, dtype=np.int32).reshape(-1, 2))
    g = np.asarray(occ)
    g = np.ascontiguousarray(g if g.dtype == np.uint8 else (g != 0).view(np.uint8))
    if g.ndim != 2:
        raise ValueError("grid must be 2-D")
    s = None if shift is None else np.ascontiguousarray(np.asarray(shift, dtype=np.int32).ravel())
    if s is not None and s.shape[0] != 2:
        raise ValueError("expected 2 components")
    verdict, seg = C.c_int32(0), C.c_int32(0)
    cell = np.zeros(2, dtype=np.int32)
    rc = L.fxjps_check_path(_lib.ptr(c, C.c_int32), c.shape[0], _lib.ptr(g, C.c_uint8), g.shape[0], g.shape[1],
                            None if s is None else _lib.ptr(s, C.c_int32), C.byref(verdict), C.byref(seg), _lib.ptr(cell, C.c_int32))
    if rc != 0:
        raise _lib.FxjpsError(rc, "fxjps_check_path: bad argument")
    return verdict.value, seg.value, (int(cell[0]), int(cell[1]))


def _batch_vec(v, n):
    a = np.asarray(v, dtype=np.float64)
    if a.ndim == 1:
        a = np.broadcast_to(a, (n, 3))
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != (n, 3):
        raise ValueError("expected %d x 3 values" % n)
    return a


def _batch_paths(planner, paths, n_hint):
    """paths: None (the planner's most recent batch, resident on the device) or (offsets, cells) as plan_batch returns;
    (offsets, None), where the caller says so: the resident paths again, with the offsets their batch returned."""
    if paths is None:
        return n_hint, None, None
    off = np.ascontiguousarray(paths[0], dtype=np.int64)
    if paths[1] is None:
        return len(off) - 1, off, None
    cells = np.ascontiguousarray(np.asarray(paths[1], dtype=np.int32).reshape(-1, 2))
    return len(off) - 1, off, cells


def select_ccst_batch(planner, nq, map_reso, map_o, pos, global_goal, end_occu=None, paths=None, return_kept=False):
    """global_planner_ccst.py:487-544 for every path of a batch, on the device, against the planner's resident grid
    (fxjps_waypoint_ccst_batch).  paths=None: the paths of the planner's last plan_batch / replan_frame (`nq` of them).
    pos / global_goal: one (x, y, z) for all, or nq x 3.  -> (wp float64[nq, 3], global_goal float64[nq, 3], n_kept int32[nq])
    [+ kept cells int32[total, 2], aligned with the offsets of the paths, when return_kept]."""
    nq, off, cells = _batch_paths(planner, paths, int(nq))
    o = _vec(map_o, 2)
    p, g = _batch_vec(pos, nq), _batch_vec(global_goal, nq)
    eo = None if end_occu is None else np.ascontiguousarray(np.broadcast_to(np.asarray(end_occu, dtype=np.int32), (nq,)))
    wp, gout, nk = np.zeros((nq, 3)), np.zeros((nq, 3)), np.zeros(nq, dtype=np.int32)
    kept = None
    cap = 0
    if return_kept:
        if off is None:
            raise ValueError("return_kept needs the paths (their offsets place the kept cells)")
        cap = int(off[-1])
        kept = np.zeros((max(cap, 1), 2), dtype=np.int32)
    planner._chk(planner._L.fxjps_waypoint_ccst_batch(
        planner._h, nq, None if off is None else _lib.ptr(off, C.c_int64), None if cells is None else _lib.ptr(cells, C.c_int32),
        float(map_reso), _lib.ptr(o, C.c_double), _lib.ptr(p, C.c_double), _lib.ptr(g, C.c_double),
        None if eo is None else _lib.ptr(eo, C.c_int32), _lib.ptr(wp, C.c_double), _lib.ptr(gout, C.c_double), _lib.ptr(nk, C.c_int32),
        None if kept is None else _lib.ptr(kept, C.c_int32), cap))
    if return_kept:
        return wp, gout, nk, kept[:cap]
    return wp, gout, nk


def select_st_batch(planner, nq, map_start, map_reso, map_o, pos, global_goal, end_occu=None, prev_wp=None, prev_dim=None, paths=None,
                    dis_wp_tre=2.0, ang_wp_tre=math.pi / 4, nthreads=0):
    """global_planner_st.py:292-327 for every path of a batch, one wavefront per path on the device (fxjps_waypoint_st_batch;
    the angles come out of a table of the host's own atan2, filled by `nthreads` host threads once per range of map_start).
    -> (wp float64[nq, 3], dim int32[nq] (2 or 3 valid components), global_goal float64[nq, 3], ang_wp float64[nq])"""
    nq, off, cells = _batch_paths(planner, paths, int(nq))
    o = _vec(map_o, 2)
    p, g = _batch_vec(pos, nq), _batch_vec(global_goal, nq)
    ms = np.ascontiguousarray(np.broadcast_to(np.asarray(map_start, dtype=np.int32), (nq, 2)))
    eo = None if end_occu is None else np.ascontiguousarray(np.broadcast_to(np.asarray(end_occu, dtype=np.int32), (nq,)))
    pw = pd = None
    if prev_wp is not None:
        pw = np.ascontiguousarray(np.asarray(prev_wp, dtype=np.float64).reshape(nq, 3))
        pd = np.ascontiguousarray(np.asarray(prev_dim, dtype=np.int32).reshape(nq))
    wp, gout, dim, ang = np.zeros((nq, 3)), np.zeros((nq, 3)), np.zeros(nq, dtype=np.int32), np.zeros(nq)
    planner._chk(planner._L.fxjps_waypoint_st_batch(
        planner._h, nq, None if off is None else _lib.ptr(off, C.c_int64), None if cells is None else _lib.ptr(cells, C.c_int32),
        _lib.ptr(ms, C.c_int32), float(map_reso), _lib.ptr(o, C.c_double), _lib.ptr(p, C.c_double), _lib.ptr(g, C.c_double),
        None if eo is None else _lib.ptr(eo, C.c_int32), float(dis_wp_tre), float(ang_wp_tre),
        None if pw is None else _lib.ptr(pw, C.c_double), None if pd is None else _lib.ptr(pd, C.c_int32),
        _lib.ptr(wp, C.c_double), _lib.ptr(dim, C.c_int32), _lib.ptr(gout, C.c_double), _lib.ptr(ang, C.c_double), int(nthreads)))
    return wp, dim, gout, ang


def select_slots_batch(planner, rule, map_start, map_reso, map_o, pos, global_goal, end_occu=None, prev_wp=None, prev_dim=None,
                       grid_ids=None, paths=None, return_kept=False, dis_wp_tre=2.0, ang_wp_tre=math.pi / 4, nthreads=0):
    """Both rules over a grid-slots batch in one call (fxjps_waypoint_slots_batch): query q is selected by rule[q] (0 / "st":
    global_planner_st.py:292-327; 1 / "ccst": global_planner_ccst.py:487-544 against the grid of slot grid_ids[q] as it is
    now) with its own map_start[q], map_reso[q] and map_o[q].  paths=None: the paths of the planner's last plan_batch_slots,
    resident on the device (len(rule) of them; grid_ids=None: the slots that batch named); else (offsets, cells), and
    grid_ids is needed as soon as one query uses the ccst rule; (offsets, None): the resident paths, `offsets` being what
    that plan_batch_slots returned (return_kept needs them to place the kept cells).  map_reso: a scalar or nq values; map_o: one pair or
    nq x 2; map_start: one pair or nq x 2 (None when no query uses the st rule); pos / global_goal: one (x, y, z) or nq x 3.
    -> (wp float64[nq, 3], dim int32[nq] (2 or 3 valid components; ccst: 3), global_goal float64[nq, 3], ang_wp float64[nq]
    (ccst: 0.0), n_kept int32[nq] (st: 0)) [+ kept cells int32[total, 2], aligned with the offsets of the paths, when
    return_kept]."""
    r = np.ascontiguousarray([{"st": 0, "ccst": 1}[x] if isinstance(x, str) else int(x) for x in np.asarray(rule, dtype=object).ravel()],
                             dtype=np.int32)  # (a number other than 0 / 1 goes through: the library refuses it and names the query)
    nq, off, cells = _batch_paths(planner, paths, len(r))
    if len(r) != nq:
        raise ValueError("%d rules for %d paths" % (len(r), nq))
    reso = np.ascontiguousarray(np.broadcast_to(np.asarray(map_reso, dtype=np.float64), (nq,)))
    o = np.ascontiguousarray(np.broadcast_to(np.asarray(map_o, dtype=np.float64), (nq, 2)))
    p, g = _batch_vec(pos, nq), _batch_vec(global_goal, nq)
    ms = None if map_start is None else np.ascontiguousarray(np.broadcast_to(np.asarray(map_start, dtype=np.int32), (nq, 2)))
    eo = None if end_occu is None else np.ascontiguousarray(np.broadcast_to(np.asarray(end_occu, dtype=np.int32), (nq,)))
    ids = None if grid_ids is None else np.ascontiguousarray(np.broadcast_to(np.asarray(grid_ids, dtype=np.int32), (nq,)))
    pw = pd = None
    if prev_wp is not None:
        pw = np.ascontiguousarray(np.asarray(prev_wp, dtype=np.float64).reshape(nq, 3))
        pd = np.ascontiguousarray(np.asarray(prev_dim, dtype=np.int32).reshape(nq))
    wp, gout, dim, ang, nk = np.zeros((nq, 3)), np.zeros((nq, 3)), np.zeros(nq, dtype=np.int32), np.zeros(nq), np.zeros(nq, dtype=np.int32)
    kept = None
    cap = 0
    if return_kept:
        if off is None:
            raise ValueError("return_kept needs the paths (their offsets place the kept cells)")
        cap = int(off[-1])
        kept = np.zeros((max(cap, 1), 2), dtype=np.int32)

    def opt(a, t):
        return None if a is None else _lib.ptr(a, t)
    planner._chk(planner._L.fxjps_waypoint_slots_batch(
        planner._h, nq, None if cells is None else _lib.ptr(off, C.c_int64), opt(cells, C.c_int32), opt(ids, C.c_int32), _lib.ptr(r, C.c_int32), opt(ms, C.c_int32),
        _lib.ptr(reso, C.c_double), _lib.ptr(o, C.c_double), _lib.ptr(p, C.c_double), _lib.ptr(g, C.c_double), opt(eo, C.c_int32),
        float(dis_wp_tre), float(ang_wp_tre), opt(pw, C.c_double), opt(pd, C.c_int32), _lib.ptr(wp, C.c_double), _lib.ptr(dim, C.c_int32),
        _lib.ptr(gout, C.c_double), _lib.ptr(ang, C.c_double), _lib.ptr(nk, C.c_int32), opt(kept, C.c_int32), cap, int(nthreads)))
    if return_kept:
        return wp, dim, gout, ang, nk, kept[:cap]
    return wp, dim, gout, ang, nk


def tick_outputs_slots(planner, rule, map_start, map_reso, map_o, pos, global_goal, home, end_occu=None, prev_wp=None, prev_dim=None,
                       grid_ids=None, paths=None, offsets=None, return_kept=False, dis_wp_tre=2.0, ang_wp_tre=math.pi / 4, nthreads=0):
    """What both nodes send out per tick, for every query of a grid-slots batch in one call (fxjps_tick_outputs_slots):
    select_slots_batch's selection, and from the same launch the Point of /goal_global (x, y of the waypoint, z by
    global_planner_st.py:335 or global_planner_ccst.py:559-562 with `home` = (xo, yo), one pair or nq x 2), /jps_path (path3,
    st:292-298 / ccst:487-494) and the ccst node's /direct_jps_path (path4 of ccst:495-521 with time_b 0; without a path the two
    poses [pos, wp] with time_b 100; st: empty).  The other arguments are select_slots_batch's.  With paths=None
    (the resident paths of the planner's last plan_batch_slots) `offsets` are the offsets that call returned: they place
    the triples.
    -> (wp, dim, goal_out, ang_wp, n_kept, point float64[nq, 3], paths, dir_paths, dir_back int32[nq]); paths and dir_paths
    are lists of nq float64 [m, 3] views [+ kept cells int32[total, 2], aligned with the offsets of the paths, when
    return_kept]."""
    r = np.ascontiguousarray([{"st": 0, "ccst": 1}[x] if isinstance(x, str) else int(x) for x in np.asarray(rule, dtype=object).ravel()],
                             dtype=np.int32)
    nq, off, cells = _batch_paths(planner, paths, len(r))
    if len(r) != nq:
        raise ValueError("%d rules for %d paths" % (len(r), nq))
    c_off = None if cells is None else off
    if off is None:
        if offsets is None:
            raise ValueError("resident paths need offsets= (what plan_batch_slots returned): they place the triples")
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        if len(off) != nq + 1:
            raise ValueError("%d offsets for %d paths" % (len(off), nq))
    reso = np.ascontiguousarray(np.broadcast_to(np.asarray(map_reso, dtype=np.float64), (nq,)))
    o = np.ascontiguousarray(np.broadcast_to(np.asarray(map_o, dtype=np.float64), (nq, 2)))
    p, g = _batch_vec(pos, nq), _batch_vec(global_goal, nq)
    hm = np.ascontiguousarray(np.broadcast_to(np.asarray(home, dtype=np.float64), (nq, 2)))
    ms = None if map_start is None else np.ascontiguousarray(np.broadcast_to(np.asarray(map_start, dtype=np.int32), (nq, 2)))
    eo = None if end_occu is None else np.ascontiguousarray(np.broadcast_to(np.asarray(end_occu, dtype=np.int32), (nq,)))
    ids = None if grid_ids is None else np.ascontiguousarray(np.broadcast_to(np.asarray(grid_ids, dtype=np.int32), (nq,)))
    pw = pd = None
    if prev_wp is not None:
        pw = np.ascontiguousarray(np.asarray(prev_wp, dtype=np.float64).reshape(nq, 3))
        pd = np.ascontiguousarray(np.asarray(prev_dim, dtype=np.int32).reshape(nq))
    wp, gout, dim, ang, nk = np.zeros((nq, 3)), np.zeros((nq, 3)), np.zeros(nq, dtype=np.int32), np.zeros(nq), np.zeros(nq, dtype=np.int32)
    total = int(off[-1]) if nq else 0
    point, dn, db = np.zeros((nq, 3)), np.zeros(nq, dtype=np.int32), np.zeros(nq, dtype=np.int32)
    pxyz, dxyz = np.zeros((max(total, 1), 3)), np.zeros((total + 2 * nq + 1, 3))
    kept = np.zeros((max(total, 1), 2), dtype=np.int32) if return_kept else None

    def opt(a, t):
        return None if a is None else _lib.ptr(a, t)
    planner._chk(planner._L.fxjps_tick_outputs_slots(
        planner._h, nq, opt(c_off, C.c_int64), opt(cells, C.c_int32), opt(ids, C.c_int32), _lib.ptr(r, C.c_int32), opt(ms, C.c_int32),
        _lib.ptr(reso, C.c_double), _lib.ptr(o, C.c_double), _lib.ptr(p, C.c_double), _lib.ptr(g, C.c_double), opt(eo, C.c_int32),
        float(dis_wp_tre), float(ang_wp_tre), opt(pw, C.c_double), opt(pd, C.c_int32), _lib.ptr(hm, C.c_double), _lib.ptr(wp, C.c_double),
        _lib.ptr(dim, C.c_int32), _lib.ptr(gout, C.c_double), _lib.ptr(ang, C.c_double), _lib.ptr(nk, C.c_int32), opt(kept, C.c_int32), total,
        _lib.ptr(point, C.c_double), _lib.ptr(pxyz, C.c_double), total, _lib.ptr(dxyz, C.c_double), _lib.ptr(dn, C.c_int32),
        _lib.ptr(db, C.c_int32), total + 2 * nq, int(nthreads)))
    paths_out = [pxyz[int(off[q]):int(off[q + 1])] for q in range(nq)]
    dir_out = [dxyz[int(off[q]) + 2 * q:int(off[q]) + 2 * q + int(dn[q])] for q in range(nq)]
    if return_kept:
        return wp, dim, gout, ang, nk, point, paths_out, dir_out, db, kept[:total]
    return wp, dim, gout, ang, nk, point, paths_out, dir_out, db
