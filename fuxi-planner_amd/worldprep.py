"""What each planner node does between the map callback and the grid preparation, per vehicle, in plain numpy: the ccst
node's crop of the map message to its occupied box (global_planner_ccst.py:36-63), the prior-map merge
(global_planner_st.py:210-225 / global_planner_ccst.py:395-409) and the world -> cell conversion (st:226-227 /
ccst:411-412).

This is the host form of Planner.prepare_slots_world for callers without a device, and what the tests compare the device
against: the same float64 operations in the same order, truncation toward zero where the reference's .astype(int) /
int() truncate, and a ValueError where the library refuses.  Pinned by tests/golden/worldprep.json, whose expected
values come from executing the reference's own lines (tests/golden/make_golden_worldprep.py).  crop_host is the host form
of Planner.prepare_slots_cropped in the same way, pinned by tests/golden/cropprep.json (make_golden_cropprep.py), and
absorb_host that of Planner.absorb_prior: the same slice assignment kept in the prior map, pinned by the canvases of
worldprep.json; grow_host is that of Planner.absorb_prior_grow: the whole canvas kept, pinned by the same canvases;
window_host and slide_host are those of Planner.absorb_prior_slide: the grow_host fold, then a slice of it.
"""
import math

import numpy as np

I32_LO, I32_HI = -2147483649.0, 2147483648.0  # a quotient strictly between them truncates to an int32


def matrix_from_msg(data, width, height):
    """The matrix map_callback (st:15-20) makes of a nav_msgs/OccupancyGrid: [x][y], 100 -> 1, -1 -> 0."""
    a = np.asarray(data, dtype=np.int8).reshape(-1)
    if a.size != width * height:
        raise ValueError("data has %d cells, expected %d" % (a.size, width * height))
    m = a.reshape(height, width).T.copy()
    m[m == 100] = 1
    m[m == -1] = 0
    return m


def prior_from_image(gray):
    """The loader convention of st:179-182 on a decoded 8-bit grey image (rows x cols): > 200 free, else occupied, the
    map is img[::-1].T.  -> uint8 [cols][rows]."""
    gray = np.asarray(gray, dtype=np.uint8)
    if gray.ndim != 2:
        raise ValueError("image must be 2-D (convert('L'))")
    return np.ascontiguousarray(np.where(gray > 200, 0, 1).astype(np.uint8)[::-1].T)


def map_top(map_o, extent, map_reso):
    """self.map_t as map_callback computes it (st:24)."""
    return [float(map_o[0]) + int(extent[0]) * float(map_reso), float(map_o[1]) + int(extent[1]) * float(map_reso)]


def _trunc(q, what):
    if not (I32_LO < q < I32_HI):  # (NaN and the infinities fail)
        raise ValueError("%s: the quotient %r does not truncate to an int32" % (what, q))
    return int(q)


def _pair(v, what):
    a, b = float(v[0]), float(v[1])
    if not (math.isfinite(a) and math.isfinite(b)):
        raise ValueError("%s is not finite" % what)
    return [a, b]


NOT_PLANNED, REFUSED = 1, -1  # crop_host's outcomes besides 0: FXJPS_JOB_NOT_PLANNED, FXJPS_E_ARG
I32_MAX = 2147483647


def crop_host(raw, map_o, map_reso, pos_xy, ifa):
    """remove_zero_rowscols (ccst:36-63, called at :349) and the node's decision whether to plan at all (ccst:351).  raw:
    the map MESSAGE as map_callback left it, a matrix [x][y] or (data, width, height) of an OccupancyGrid; map_o: the
    message's origin.  -> (record, outcome, window).  record: bbox (min x, min y, max x, max y of the non-zero cells;
    I32_MAX, I32_MAX, -1, -1: none, and lo = win = 0 then), start0 (the vehicle's cell in the message), lo (the window's
    low corner: min(first non-zero, vehicle's cell) per axis), win (map_c, map_r = bbox max - lo: the last non-zero row
    and column are EXCLUDED), map_o and map_t (the cropped ones) -- fxjps_crop_t field by field.  outcome: 0, the window
    X[lo_x:max_x, lo_y:max_y] goes on into merge_host with the record's win, map_o and map_t; NOT_PLANNED (no non-zero
    cell, width <= 2 * ifa, or win[0] * win[1] <= 0: the node does not plan on this tick); REFUSED (lo < 0 on an axis:
    the reference's slice counts from the end there, the library refuses the job).  window is None unless outcome is 0."""
    m = matrix_from_msg(*raw) if isinstance(raw, tuple) else np.asarray(raw)
    if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError("the map message must be 2-D and not empty")
    reso = float(map_reso)
    if not (math.isfinite(reso) and reso > 0.0):
        raise ValueError("map_reso %r must be finite and > 0" % (map_reso,))
    o = _pair(map_o, "map_o")
    pos = _pair(pos_xy, "pos_xy")
    start0 = [_trunc((pos[k] - o[k]) / reso, "the vehicle's cell in the message") for k in range(2)]   # ccst:47
    nz = m.nonzero()                                                                                   # ccst:42
    none = len(nz[0]) == 0
    bbox = [I32_MAX, I32_MAX, -1, -1] if none else [int(nz[0].min()), int(nz[1].min()), int(nz[0].max()), int(nz[1].max())]
    lo = [0, 0] if none else [min(bbox[k], start0[k]) for k in range(2)]                               # ccst:48-52
    win = [0, 0] if none else [bbox[2 + k] - lo[k] for k in range(2)]                                  # ccst:49-50
    o2 = [float(lo[k]) * reso + o[k] for k in range(2)]                                                # ccst:52
    t2 = [o2[k] + float(win[k]) * reso for k in range(2)]                                              # ccst:54
    if none or m.shape[0] <= 2 * int(ifa) or win[0] * win[1] <= 0:                                     # ccst:61-63, :351
        outcome = NOT_PLANNED
    elif lo[0] < 0 or lo[1] < 0:
        outcome = REFUSED
    else:
        outcome = 0
    window = m[lo[0]:bbox[2], lo[1]:bbox[3]] if outcome == 0 else None                                 # ccst:56, :60
    rec = {"bbox": bbox, "start0": start0, "lo": lo, "win": [min(w, I32_MAX) for w in win], "map_o": o2, "map_t": t2}
    return rec, outcome, window


ABSORB_MODES = ("overwrite", "occupied", "known")  # FXJPS_ABSORB_OVERWRITE, _OCCUPIED, _KNOWN


def absorb_host(prior, ori_pre, raw, map_o, map_reso, mode="overwrite", lo=None, win=None):
    """One job of Planner.absorb_prior on the host: the rectangle lo .. lo + win - 1 of raw (None: the whole map) pasted
    into the prior map, the slice assignment of st:219-220 kept.  prior: the prior's bytes [x][y] at world origin ori_pre;
    raw: a matrix [x][y] (> 0 = occupied; it has no unknown cells) or (data, width, height) of an OccupancyGrid (> 0 =
    occupied, -1 = unknown); map_o: the world origin of the RECTANGLE (a cropped job: the crop record's map_o).  The
    rectangle's cell (0, 0) lands on prior cell d = trunc((map_o - o1) / map_reso) - trunc((ori_pre - o1) / map_reso), o1 =
    min(map_o, ori_pre), per axis -- where merge_host's canvas puts the two (st:212-214); cells that fall outside the prior
    are dropped.  mode "overwrite": every covered cell becomes the rectangle's occupancy, 1 or 0 (unknown counts as free);
    "occupied": 1 where the rectangle is occupied, else the byte stays; "known": the occupancy where the rectangle is not
    unknown, else the byte stays.  A byte that is not decided stays as it is (a 255 stays 255).
    -> (new prior uint8, inside, outside, changed): the cells of the rectangle inside / outside the prior, and the cells
    whose occupancy (non-zero) flipped.  Several jobs: call it job by job on the result.  ValueError where the library
    refuses."""
    if mode not in ABSORB_MODES:
        raise ValueError("mode %r is not one of %r" % (mode, ABSORB_MODES))
    pre = np.asarray(prior)
    if pre.ndim != 2 or pre.shape[0] < 1 or pre.shape[1] < 1:
        raise ValueError("the prior map must be 2-D and not empty")
    if isinstance(raw, tuple):
        data, width, height = raw
        a = np.asarray(data, dtype=np.int8).reshape(-1)
        if a.size != width * height:
            raise ValueError("data has %d cells, expected %d" % (a.size, width * height))
        m = a.reshape(height, width).T
        unknown = m == -1
    else:
        m = np.asarray(raw)
        unknown = None
    if m.ndim != 2 or not (1 <= m.shape[0] <= 8190 and 1 <= m.shape[1] <= 8190):
        raise ValueError("raw must be 2-D and 1..8190 cells a side")
    occupied = m > 0
    lo = [0, 0] if lo is None else [int(lo[0]), int(lo[1])]
    win = [m.shape[k] - lo[k] for k in range(2)] if win is None else [int(win[0]), int(win[1])]
    for k in range(2):
        if win[k] < 1 or lo[k] < 0 or lo[k] + win[k] > m.shape[k]:
            raise ValueError("axis %d: the rectangle (%d + %d) is empty or does not lie inside raw's %d cells" % (k, lo[k], win[k], m.shape[k]))
    reso = float(map_reso)
    if not (math.isfinite(reso) and reso > 0.0):
        raise ValueError("map_reso %r must be finite and > 0" % (map_reso,))
    o = _pair(map_o, "map_o")
    op = _pair(ori_pre, "ori_pre")
    new = np.array(pre, dtype=np.uint8)
    a0, a1 = [0, 0], [0, 0]  # the rectangle clipped to the prior, in prior cells
    d = [0, 0]
    for k in range(2):
        o1 = min(o[k], op[k])                                                       # st:212
        d[k] = _trunc((o[k] - o1) / reso, "the detected map's index") - _trunc((op[k] - o1) / reso, "the prior's index")  # st:213-214
        a0[k] = max(d[k], 0)
        a1[k] = min(d[k] + win[k], int(pre.shape[k]))
    inside = max(a1[0] - a0[0], 0) * max(a1[1] - a0[1], 0)
    changed = 0
    if inside > 0:
        cut = tuple(slice(lo[k] + a0[k] - d[k], lo[k] + a1[k] - d[k]) for k in range(2))
        occ = occupied[cut]
        target = new[a0[0]:a1[0], a0[1]:a1[1]]
        before = target != 0
        if mode == "overwrite":
            target[...] = occ
        elif mode == "occupied":
            target[occ] = 1
        elif unknown is None:
            target[...] = occ
        else:
            known = ~unknown[cut]
            target[known] = occ[known]
        changed = int(np.count_nonzero((target != 0) != before))
    return new, inside, win[0] * win[1] - inside, changed


def grow_host(prior, ori_pre, raw, map_o, map_reso, mode="overwrite", lo=None, win=None, map_t=None, limit=(8190, 8190)):
    """One job of Planner.absorb_prior_grow on the host: absorb_host on a prior that GROWS to hold the rectangle -- the
    canvas of st:212-220, the union of the prior and the detected map, kept as the next prior.  Arguments as absorb_host
    takes them, and map_t, the rectangle's top (None: map_o + win * map_reso; a cropped job: the crop record's).  Per axis
        o1 = min(map_o, ori_pre);  at_raw = trunc((map_o - o1) / reso);  at_pre = trunc((ori_pre - o1) / reso)
        size = max(trunc((max(ori_pre + reso * W, map_t) - o1) / reso), at_pre + W, at_raw + win)
    in merge_host's float64 operations and order.  The new prior has size cells a side: the old bytes unchanged at at_pre
    (a 255 stays 255), the rectangle applied at at_raw under the mode's rule, every other cell 0.  size is the
    reference's canvas extent except where its slice assignment would raise or clip: there the prior still grows.
    -> (new prior uint8, new ori_pre [x, y] (o1), shift (at_pre: where old cell (0, 0) lies), at (at_raw: where rectangle
    cell (0, 0) lies), changed: the cells whose occupancy (non-zero) differs from the old byte at that place, 0 where the
    old prior had none).  Several jobs: call it job by job on the result (an earlier job's `at` then moves by every later
    job's shift).  limit: the largest side per axis (slide_host passes the call's, or int32's for a prior that is cut
    afterwards).  ValueError where the library refuses."""
    if mode not in ABSORB_MODES:
        raise ValueError("mode %r is not one of %r" % (mode, ABSORB_MODES))
    pre = np.asarray(prior)
    if pre.ndim != 2 or pre.shape[0] < 1 or pre.shape[1] < 1:
        raise ValueError("the prior map must be 2-D and not empty")
    if isinstance(raw, tuple):
        data, width, height = raw
        a = np.asarray(data, dtype=np.int8).reshape(-1)
        if a.size != width * height:
            raise ValueError("data has %d cells, expected %d" % (a.size, width * height))
        m = a.reshape(height, width).T
        unknown = m == -1
    else:
        m = np.asarray(raw)
        unknown = None
    if m.ndim != 2 or not (1 <= m.shape[0] <= 8190 and 1 <= m.shape[1] <= 8190):
        raise ValueError("raw must be 2-D and 1..8190 cells a side")
    occupied = m > 0
    lo = [0, 0] if lo is None else [int(lo[0]), int(lo[1])]
    win = [m.shape[k] - lo[k] for k in range(2)] if win is None else [int(win[0]), int(win[1])]
    for k in range(2):
        if win[k] < 1 or lo[k] < 0 or lo[k] + win[k] > m.shape[k]:
            raise ValueError("axis %d: the rectangle (%d + %d) is empty or does not lie inside raw's %d cells" % (k, lo[k], win[k], m.shape[k]))
    reso = float(map_reso)
    if not (math.isfinite(reso) and reso > 0.0):
        raise ValueError("map_reso %r must be finite and > 0" % (map_reso,))
    o = _pair(map_o, "map_o")
    op = _pair(ori_pre, "ori_pre")
    top = _pair(map_t, "map_t") if map_t is not None else map_top(o, win, reso)
    if not (math.isfinite(top[0]) and math.isfinite(top[1])):
        raise ValueError("map_t is not finite")
    ext = [int(pre.shape[0]), int(pre.shape[1])]
    o1, at_raw, at_pre, size = [0.0, 0.0], [0, 0], [0, 0], [0, 0]
    for k in range(2):
        t_pre = op[k] + reso * ext[k]                                            # st:187
        o1[k] = min(o[k], op[k])                                                 # st:212
        at_raw[k] = _trunc((o[k] - o1[k]) / reso, "the detected map's index")    # st:213
        at_pre[k] = _trunc((op[k] - o1[k]) / reso, "the prior's index")          # st:214
        ref = _trunc((max(t_pre, top[k]) - o1[k]) / reso, "the canvas extent")   # st:215-216
        size[k] = max(ref, at_pre[k] + ext[k], at_raw[k] + win[k])
        if size[k] > limit[k]:
            raise ValueError("axis %d: the prior would grow to %d cells, above %d" % (k, size[k], limit[k]))
    placed = np.zeros(size, dtype=np.uint8)
    placed[at_pre[0]:at_pre[0] + ext[0], at_pre[1]:at_pre[1] + ext[1]] = pre
    new = placed.copy()
    cut = tuple(slice(lo[k], lo[k] + win[k]) for k in range(2))
    occ = occupied[cut]
    target = new[at_raw[0]:at_raw[0] + win[0], at_raw[1]:at_raw[1] + win[1]]
    if mode == "overwrite" or (mode == "known" and unknown is None):
        target[...] = occ
    elif mode == "occupied":
        target[occ] = 1
    else:
        known = ~unknown[cut]
        target[known] = occ[known]
    changed = int(np.count_nonzero((new != 0) != (placed != 0)))
    return new, o1, at_pre, at_raw, changed


KEEP_USES = ("none", "always", "over_limit")  # FXJPS_KEEP_NONE, _ALWAYS, _OVER_LIMIT


def window_cells(extent, origin, map_reso, keep_lo, keep_hi):
    """The cells [k0, k1) per axis that a keep window (world metres; an infinite bound: no cut on that side) leaves of a
    prior of `extent` cells at `origin`, and the origin of the cut: per axis, in float64,
        k0 = clamp(trunc((keep_lo - origin) / reso), 0, extent);  k1 = clamp(trunc((keep_hi - origin) / reso), 0, extent)
        new origin = origin if k0 == 0 else origin + reso * k0
    with the clamp on the float before the conversion.  -> (k0, k1, new origin).  ValueError where the library refuses:
    NaN in a bound, lo > hi, a window that holds no cell (k1 <= k0)."""
    reso = float(map_reso)
    if not (math.isfinite(reso) and reso > 0.0):
        raise ValueError("map_reso %r must be finite and > 0" % (map_reso,))
    og = _pair(origin, "origin")
    k0, k1, new = [0, 0], [0, 0], [0.0, 0.0]
    for k in range(2):
        lo, hi, G = float(keep_lo[k]), float(keep_hi[k]), float(int(extent[k]))
        if math.isnan(lo) or math.isnan(hi):
            raise ValueError("axis %d: NaN in the keep window" % k)
        if lo > hi:
            raise ValueError("axis %d: the keep window's lo %r is above its hi %r" % (k, lo, hi))
        a, b = (lo - og[k]) / reso, (hi - og[k]) / reso
        a = a if math.isinf(a) else float(math.trunc(a))
        b = b if math.isinf(b) else float(math.trunc(b))
        k0[k] = int(min(max(a, 0.0), G))
        k1[k] = int(min(max(b, 0.0), G))
        if k1[k] <= k0[k]:
            raise ValueError("axis %d: the keep window holds no cell of the prior (cells %d .. %d of %d)" % (k, k0[k], k1[k], int(G)))
        new[k] = og[k] if k0[k] == 0 else og[k] + reso * float(k0[k])
    return k0, k1, new


def window_host(prior, origin, map_reso, keep_lo, keep_hi):
    """The cut of Planner.absorb_prior_slide on the host: -> (prior[k0[0]:k1[0], k0[1]:k1[1]] (a copy), new origin, cut_lo =
    k0, cut_hi = extent - k1) with window_cells' arithmetic.  ValueError where the library refuses."""
    pre = np.asarray(prior)
    if pre.ndim != 2 or pre.shape[0] < 1 or pre.shape[1] < 1:
        raise ValueError("the prior map must be 2-D and not empty")
    k0, k1, new = window_cells(pre.shape, origin, map_reso, keep_lo, keep_hi)
    return pre[k0[0]:k1[0], k0[1]:k1[1]].copy(), new, k0, [pre.shape[k] - k1[k] for k in range(2)]


def slide_host(before, jobs, mode="overwrite", crops=None, limit=None, keep=None, use="over_limit"):
    """Planner.absorb_prior_slide on the host, and the yardstick of its GPU tests: the grow_host fold job by job, then
    window_host under the use / limit rule.  before: {prior: bytes [x][y]}; jobs, crops, mode, limit, keep ({prior: (lo_xy,
    hi_xy)}) and use (one of KEEP_USES, or {prior: use}) as absorb_prior_slide takes them, every job's ori_pre the prior's
    origin BEFORE the call.  A prior with a keep window is not held to the limit job after job (only to int32); its window is
    applied under "always", under "over_limit" if and only if a grown side exceeds the limit; a side above the limit after
    the cut is refused.  -> (after {prior: bytes}, records {named prior: {"W", "H", "shift", "origin", "changed", "trimmed",
    "grown_wh", "cut_lo", "cut_hi"}}, [(at, inside, outside) per job]).  The host form materialises the grown frame, which
    the library never does.  ValueError where the library refuses."""
    jobs = list(jobs)
    lim = [8190, 8190] if limit is None else [int(limit), int(limit)] if np.isscalar(limit) else [int(limit[0]), int(limit[1])]
    if not all(1 <= x <= 8190 for x in lim):
        raise ValueError("the limit %r is not in 1 .. 8190" % (lim,))
    keep = {} if keep is None else {int(p): w for p, w in keep.items()}
    uses = {p: (use.get(p, "none") if isinstance(use, dict) else use) for p in keep}
    for p, u in uses.items():
        if u not in KEEP_USES:
            raise ValueError("prior %d: use %r is not one of %r" % (p, u, KEEP_USES))
        if u != "none":
            for k in range(2):
                lo, hi = float(keep[p][0][k]), float(keep[p][1][k])
                if math.isnan(lo) or math.isnan(hi) or lo > hi:
                    raise ValueError("prior %d: axis %d: a NaN in the keep window, or lo above hi" % (p, k))
    cur = {int(k): np.array(v, dtype=np.uint8) for k, v in before.items()}
    origin, shift, at, first = {}, {}, [], {}
    for v, wj in enumerate(jobs):
        raw, map_o, reso, prior, ori_pre = wj[1], wj[2], wj[3], int(wj[8]), wj[9]
        map_t = wj[10] if len(wj) > 10 else None
        rec = crops[v] if crops is not None else None
        lo, win = (None, None) if rec is None else (rec["lo"], rec["win"])
        if rec is not None:
            map_o, map_t = rec["map_o"], rec["map_t"]
        if prior not in cur:
            raise ValueError("job %d: prior %d is not set" % (v, prior))
        if prior in first and (tuple(float(x) for x in ori_pre), float(reso)) != first[prior]:
            raise ValueError("job %d: ori_pre / map_reso differ from those of an earlier job on prior %d" % (v, prior))
        first.setdefault(prior, (tuple(float(x) for x in ori_pre), float(reso)))
        held = uses.get(prior, "none") == "none"
        new, o1, sh, a, _ = grow_host(cur[prior], origin.get(prior, ori_pre), raw, map_o, reso, mode, lo=lo, win=win, map_t=map_t,
                                      limit=lim if held else (I32_MAX, I32_MAX))
        for i, earlier in enumerate(jobs[:v]):  # (the earlier rectangles move with the old prior)
            if int(earlier[8]) == prior:
                at[i][0] = (at[i][0][0] + sh[0], at[i][0][1] + sh[1])
        s = shift.get(prior, (0, 0))
        shift[prior] = (s[0] + sh[0], s[1] + sh[1])
        cur[prior], origin[prior] = new, [float(o1[0]), float(o1[1])]
        size = win if win is not None else (raw[1], raw[2]) if isinstance(raw, tuple) else np.asarray(raw).shape
        at.append([(a[0], a[1]), (int(size[0]), int(size[1])), prior])
    for p, u in uses.items():
        if u != "none" and p not in origin:
            raise ValueError("prior %d: a keep window for a prior that no job names" % p)
    records, k0s = {}, {}
    for p in origin:
        grown = cur[p]
        old = np.zeros(grown.shape, dtype=np.uint8)
        w, h = before[p].shape
        old[shift[p][0]:shift[p][0] + w, shift[p][1]:shift[p][1] + h] = before[p]
        u = uses.get(p, "none")
        G = [int(grown.shape[0]), int(grown.shape[1])]
        k0, k1, o = [0, 0], G, origin[p]
        trimmed = u == "always" or (u == "over_limit" and (G[0] > lim[0] or G[1] > lim[1]))
        if trimmed:
            k0, k1, o = window_cells(G, origin[p], first[p][1], keep[p][0], keep[p][1])
            for k in range(2):
                if k1[k] - k0[k] > lim[k]:
                    raise ValueError("prior %d: axis %d: the keep window of %d cells is above the limit of %d" % (p, k, k1[k] - k0[k], lim[k]))
        cut = (slice(k0[0], k1[0]), slice(k0[1], k1[1]))
        cur[p] = grown[cut].copy()
        k0s[p] = k0
        records[p] = {"W": k1[0] - k0[0], "H": k1[1] - k0[1], "shift": (shift[p][0] - k0[0], shift[p][1] - k0[1]), "origin": [float(o[0]), float(o[1])],
                      "changed": int(np.count_nonzero((grown[cut] != 0) != (old[cut] != 0))), "trimmed": bool(trimmed), "grown_wh": (G[0], G[1]),
                      "cut_lo": (k0[0], k0[1]), "cut_hi": (G[0] - k1[0], G[1] - k1[1])}
    per_job = []
    for a, win, p in at:
        k0, ext = k0s[p], (records[p]["W"], records[p]["H"])
        where = (a[0] - k0[0], a[1] - k0[1])
        inside = 1
        for k in range(2):
            inside *= max(0, min(where[k] + win[k], ext[k]) - max(where[k], 0))
        per_job.append((where, inside, win[0] * win[1] - inside))
    return cur, records, per_job


def merge_host(raw, map_o, map_reso, pos_xy, goal_xy, prior=None, ori_pre=(-15, -15), map_t=None):
    """raw: the detected map, a matrix [x][y] (> 0 = occupied) or (data, width, height) of an OccupancyGrid; prior: the
    prior map as a matrix [x][y] (> 0 = occupied) at world origin ori_pre, or None; map_t None: map_o + extent * map_reso.
    -> (canvas uint8 [W][H] of 0 / 1, (W, H), canvas_o [x, y], start (x, y), goal (x, y)): the merged map, its origin and
    the vehicle's and the goal's cell in it -- what Planner.prepare_slots / oracle-style preparation take as raw, start
    and goal.  The detected map OVERWRITES the prior (a free detected cell clears an occupied prior cell)."""
    m = matrix_from_msg(*raw) if isinstance(raw, tuple) else np.asarray(raw)
    if m.ndim != 2 or m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError("the detected map must be 2-D and not empty")
    ext = [int(m.shape[0]), int(m.shape[1])]
    reso = float(map_reso)
    if not (math.isfinite(reso) and reso > 0.0):
        raise ValueError("map_reso %r must be finite and > 0" % (map_reso,))
    o = _pair(map_o, "map_o")
    pos = _pair(pos_xy, "pos_xy")
    goal = _pair(goal_xy, "goal_xy")
    canvas = np.ascontiguousarray(m > 0, dtype=np.uint8)
    if prior is not None:
        pre = np.asarray(prior)
        if pre.ndim != 2 or pre.shape[0] < 1 or pre.shape[1] < 1:
            raise ValueError("the prior map must be 2-D and not empty")
        op = _pair(ori_pre, "ori_pre")
        top = _pair(map_t, "map_t") if map_t is not None else map_top(o, ext, reso)
        if not (math.isfinite(top[0]) and math.isfinite(top[1])):
            raise ValueError("map_t is not finite")
        o1, at_raw, at_pre, size = [0.0, 0.0], [0, 0], [0, 0], [0, 0]
        for k in range(2):
            t_pre = op[k] + reso * int(pre.shape[k])            # st:187
            o1[k] = min(o[k], op[k])                            # st:212
            at_raw[k] = _trunc((o[k] - o1[k]) / reso, "the detected map's index")   # st:213
            at_pre[k] = _trunc((op[k] - o1[k]) / reso, "the prior's index")         # st:214
            size[k] = _trunc((max(t_pre, top[k]) - o1[k]) / reso, "the canvas extent")  # st:215-216
            # the reference's slice assignment raises when a rectangle is clipped (st:219-220); a side of 1 clipped to 0
            # would broadcast there: refused here as well, like the library
            if size[k] < 1 or at_raw[k] < 0 or at_pre[k] < 0 or at_raw[k] + ext[k] > size[k] or at_pre[k] + int(pre.shape[k]) > size[k]:
                raise ValueError("axis %d: the detected map (%d + %d) or the prior (%d + %d) sticks out of the canvas of %d cells"
                                 % (k, at_raw[k], ext[k], at_pre[k], pre.shape[k], size[k]))
        merged = np.zeros(size, dtype=np.uint8)
        merged[at_pre[0]:at_pre[0] + pre.shape[0], at_pre[1]:at_pre[1] + pre.shape[1]] = pre > 0
        merged[at_raw[0]:at_raw[0] + ext[0], at_raw[1]:at_raw[1] + ext[1]] = canvas
        canvas, o = merged, o1
    g = tuple(_trunc((goal[k] - o[k]) / reso, "the goal's cell") for k in range(2))   # st:226
    s = tuple(_trunc((pos[k] - o[k]) / reso, "the start's cell") for k in range(2))   # st:227
    return canvas, (int(canvas.shape[0]), int(canvas.shape[1])), o, s, g
