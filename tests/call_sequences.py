"""Random call sequences on ONE handle against a stateless host model -- a helper module, not collected as a test.

The suite pins each call family on its own; what lives ACROSS calls on a handle (the stale-map flags, the deferred updates,
the stored results of replan_frame and replan_slots, the slot generations, the resident paths, Planner's memory of the
matrix set_grid uploaded) is pinned here: `generate` draws a list of plain op records from the model alone, `run` applies
each op to the library and to the model and compares every output with what the host references give on the model's
current bytes.  The model holds bytes and the bookkeeping the header documents; it never keeps a result.

    ops = generate(seed, n_steps, profile)      # the same list with and without a GPU
    run(planner, ops, oracle)                   # raises AssertionError naming seed, step and the ops so far

A failure message carries the ops up to the failing step as Python literals: run(planner, <that list>, oracle) replays it.

Op records are dicts of ints, floats, strings and lists.  A grid is a recipe {"W", "H", "seed", "p", "set"}: random bytes of
density p from numpy's RandomState(seed), then the listed [x, y, value] cells; `grid_of` expands it.

The profiles `world` and `world_two_contexts` have a generator of their own (_WorldGen, with its own draws: the op lists
of the four earlier profiles are what they were, pinned by digest in the host test).  Their state is the shared prior
maps: Model.prior is {index: bytes, the origin they lie at now, the origin they were uploaded with, whether a grow or slide
has moved them since}, written by set_prior_map / set_prior_image / clear_prior_map and by absorb_prior / absorb_prior_grow /
absorb_prior_slide (the named priors only; no slot, generation, stored result or resident path), read by every world-frame
and cropped job -- which carries the prior's index and the origin the model holds when it is drawn, now and then the
upload's origin after a grow.  Expected outputs are worldprep's host references (absorb_host, slide_host -- the grow_host
fold --, crop_host, merge_host) and, for check_paths_slots on the last slots batch's paths, waypoints.check_path on the
slots as they are now.  After every op that writes a prior or is refused on one, and on every 8th step, every set prior
is read back; prior_origin is compared after every op that names a prior.  A world job is {"slot", "raw", "msg" (handed in
as an OccupancyGrid message with -1 cells), "start", "goal", "ifa", "variant", "prior" (an index or None), "at" (the raw's
origin in cells from ORI_PRE), "ori" (the prior's origin it carries)}; a fold's job is {"prior", "raw", "msg", "at", "ori"[,
"crop": the vehicle's cell -- the job is absorbed through worldprep.crop_host's record]}; a keep window is [lo_xy, hi_xy]
with None for an infinite bound.
"""
import contextlib
import io

import numpy as np

from oracle import adapters, gridprep
from oracle import derived_maps as dm

R = 0.25                 # the resolution of every world job and waypoint call: origins lie on its grid, quotients are exact
ORI_PRE = (-3.0, 2.0)    # the world origin of prior map 0
E_ARG, E_NOGRID = -1, -4
Q_BAD_START = -2
PROFILES = ("single", "tiles", "two_contexts", "shim")
WORLD_PROFILES = ("world", "world_two_contexts")  # the shared prior maps, the cropped prepares, the path checks: their own draws
ALL_PROFILES = PROFILES + WORLD_PROFILES
SEEDS = (0, 1, 2, 3)     # the sequences the CPU and the GPU suites run per profile
STEPS = 120              # ... and their length before the closing round
MPLS = (6, 400)          # max_path_len of the stored and the slot batches: 6 cuts some paths (PATH_TOO_LONG)


# ------------------------------------------------------------------ recipes
def grid_of(spec):
    g = (np.random.RandomState(spec["seed"]).random_sample((spec["W"], spec["H"])) < spec["p"]).astype(np.uint8)
    for x, y, v in spec.get("set", ()):
        g[x, y] = v
    return g


def msg_of(spec):
    """The OccupancyGrid data[] of a raw recipe: 100 occupied, a tenth of the free cells unknown (-1)."""
    raw = grid_of(spec)
    unknown = np.random.RandomState(spec["seed"] + 1).random_sample((spec["H"], spec["W"])) < 0.1
    return np.where(raw.T > 0, 100, np.where(unknown, -1, 0)).astype(np.int8).reshape(-1)


def gray_of(spec):
    return np.random.RandomState(spec["seed"]).randint(0, 256, (spec["rows"], spec["cols"])).astype(np.uint8)


def truth(g):
    return np.ascontiguousarray(np.asarray(g) != 0, dtype=np.uint8)


def world_job(j):
    """A world-job record -> the tuple Planner.prepare_slots_world takes."""
    raw = grid_of(j["raw"])
    map_o = (ORI_PRE[0] + j["at"][0] * R, ORI_PRE[1] + j["at"][1] * R)
    pos = (map_o[0] + (j["start"][0] + 0.5) * R, map_o[1] + (j["start"][1] + 0.5) * R)
    goal = (map_o[0] + (j["goal"][0] + 0.5) * R, map_o[1] + (j["goal"][1] + 0.5) * R)
    if j.get("msg"):
        raw = (msg_of(j["raw"]), j["raw"]["W"], j["raw"]["H"])
    t = (j["slot"], raw, map_o, R, pos, goal, j["ifa"], j["variant"])
    if "ori" in j:  # (the world profiles: a prior index or None, and the origin the job carries)
        return t + (j["prior"], tuple(j["ori"]) if j["ori"] is not None else (-15.0, -15.0))
    return t + (0, ORI_PRE) if j["prior"] else t


def prior_job(j):
    """An absorb / grow / slide job record -> the tuple Planner.absorb_prior takes (a world job whose slot, position, goal,
    ifa and variant are not read)."""
    return world_job(dict(j, slot=0, start=[0, 0], goal=[0, 0], ifa=0, variant=0))


def slot_job(j):
    return (j["slot"], grid_of(j["raw"]), tuple(j["start"]), tuple(j["goal"]), j["ifa"], j["variant"])


# ------------------------------------------------------------------ host references
def csr(oracle, grids, s, g, hchoice, max_len):
    """The oracle's answer as the library returns a batch: -> (offsets int64[n+1], cells int32[total, 2], cost, status).
    grids: one grid for all queries, or one per query."""
    s = np.asarray(s, np.int32).reshape(-1, 2)
    g = np.asarray(g, np.int32).reshape(-1, 2)
    n = len(s)
    status, cost, parts = np.zeros(n, np.int32), np.zeros(n, np.float64), []
    if isinstance(grids, np.ndarray):
        if n:
            c, status, cost, _ = oracle.plan_batch(truth(grids), s, g, hchoice, literal=False, max_len=max_len)
            parts = [c[q, :max(int(status[q]), 0)] for q in range(n)]
    else:
        for q in range(n):
            c, l, k, _ = oracle.plan_batch(truth(grids[q]), s[q:q + 1], g[q:q + 1], hchoice, literal=False, max_len=max_len)
            status[q], cost[q] = l[0], k[0]
            parts.append(c[0, :max(int(l[0]), 0)])
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(np.maximum(status, 0))
    cells = np.concatenate(parts).astype(np.int32).reshape(-1, 2) if parts else np.zeros((0, 2), np.int32)
    return off, cells, cost, status


def prepared(raw, start, goal, ifa, variant):
    """-> (grid, Planner.prepare_grid's tuple) by oracle/gridprep.py."""
    grid, s, g, d, eo = gridprep.prepare_full(np.asarray(raw) > 0, start, goal, ifa, variant)
    return grid, (tuple(int(v) for v in s), tuple(int(v) for v in g), tuple(int(v) for v in d), grid.shape, int(eo))


def world_prepared(job, prior):
    """A world job (Planner's tuple) -> (grid, prepare_slots_world's tuple without ok / kept, the three world outputs)."""
    from fuxi_planner_amd import worldprep
    slot, raw, map_o, reso, pos, goal, ifa, variant = job[:8]
    canvas, shape, co, s, g = worldprep.merge_host(raw, map_o, reso, pos, goal, prior=prior if len(job) > 8 else None,
                                                   ori_pre=job[9] if len(job) > 9 else (-15, -15), map_t=job[10] if len(job) > 10 else None)
    grid, out = prepared(canvas, s, g, ifa, variant)
    origin = list(-np.asarray(out[2]) * reso + np.asarray(co, dtype=np.float64))
    return grid, out, (origin, tuple(shape), [float(co[0]), float(co[1])])


def named_prior(priors, job):
    """The bytes of the prior a world job (Planner's tuple) names out of priors {index: bytes}; None for a job without one;
    a ValueError -- the call is refused -- for one that is not set."""
    p = job[8] if len(job) > 8 else None
    if p is None:
        return None
    if p not in priors:
        raise ValueError("prior %d is not set" % p)
    return priors[p]


def refusing(fn, *args):
    """fn(*args); the ValueError with which a host reference refuses becomes the model's Refused (FXJPS_E_ARG)."""
    try:
        return fn(*args)
    except ValueError:
        raise Refused("FxjpsError", E_ARG)


NO_OUT = ((0, 0), (0, 0), (0, 0), (0, 0), 0, False)  # what a cropped job that takes no part in the call reports: ok False ...
NO_WORLD = ([0.0, 0.0], (0, 0), [0.0, 0.0])           # ... and no origin, canvas extents or canvas origin


def crop_prepared(job, priors):
    """A cropped job (Planner's tuple) by worldprep.crop_host and world_prepared -> (grid, prepare's tuple, the three world
    outputs, (status, crop record)).  grid None: the job is not planned or refused on its own (fxjps.h: the cases 1 and 2),
    its outputs are 0 and its slot is left empty."""
    from fuxi_planner_amd import worldprep
    raw = job[1] if isinstance(job[1], tuple) else (np.asarray(job[1]) > 0).astype(np.uint8)  # (the binding hands a matrix in as 0 / 1)
    rec, outcome, window = worldprep.crop_host(raw, job[2], job[3], job[4], job[6])
    prior = named_prior(priors, job)  # (a prior that is not set refuses the whole call, whatever the crop says)
    if outcome != 0:
        return None, NO_OUT, NO_WORLD, (outcome, rec)
    wj = (job[0], window, rec["map_o"]) + tuple(job[3:8]) + (job[8] if len(job) > 8 else None, job[9] if len(job) > 9 else (-15, -15), rec["map_t"])
    grid, out, w = world_prepared(wj, prior)
    return grid, out, w, (0, rec)


def keep_of(op):
    """The keep windows of a slide record ({prior: [lo_xy, hi_xy]}, None for an infinite bound) as Planner takes them."""
    inf = float("inf")
    return {int(p): ([-inf if v is None else v for v in w[0]], [inf if v is None else v for v in w[1]]) for p, w in op["keep"].items()}


def crops_of(jobs):
    """The crop records of a fold's job records, as Planner's crops= takes them: None for a job absorbed whole; for a job
    with a "crop" cell worldprep.crop_host's record of the message with the vehicle in the middle of that cell -- the
    rectangle absorbed is then the record's window.  None if no job has one."""
    from fuxi_planner_amd import worldprep
    out = []
    for j in jobs:
        if j.get("crop") is None:
            out.append(None)
            continue
        wj = world_job(dict(j, slot=0, start=j["crop"], goal=[0, 0], ifa=0, variant=0))
        raw = wj[1] if isinstance(wj[1], tuple) else (np.asarray(wj[1]) > 0).astype(np.uint8)
        rec, outcome, window = worldprep.crop_host(raw, wj[2], wj[3], wj[4], 0)
        if outcome != 0:
            raise ValueError("a message without a window cannot be absorbed through its crop record")
        out.append(rec)
    return out if any(r is not None for r in out) else None


def fold_of(before, op):
    """prior_fold of a fold's op record."""
    return prior_fold(before, [prior_job(j) for j in op["jobs"]], op, crops_of(op["jobs"]))


def prior_fold(before, jobs, op, crops=None):
    """An absorb_prior / absorb_prior_grow / absorb_prior_slide record on the priors `before` ({index: bytes}), by
    worldprep.absorb_host job by job and worldprep.slide_host (without windows: the grow_host fold).  jobs and crops as
    Planner's call takes them.  -> (the named priors' bytes afterwards, the new origins of those that grew or slid, what
    Planner's call returns).  ValueError where the library refuses."""
    from fuxi_planner_amd import worldprep
    for v, wj in enumerate(jobs):
        if wj[8] not in before:
            raise ValueError("job %d: prior %d is not set" % (v, wj[8]))
    named = sorted({wj[8] for wj in jobs})
    if op["op"] == "absorb_prior":
        cur, counts = dict(before), []
        for v, wj in enumerate(jobs):
            rec = crops[v] if crops is not None else None
            lo, win = (None, None) if rec is None else (rec["lo"], rec["win"])
            cur[wj[8]], inside, outside, _ = worldprep.absorb_host(cur[wj[8]], wj[9], wj[1], wj[2] if rec is None else rec["map_o"], wj[3], op["mode"],
                                                                   lo=lo, win=win)
            counts.append((inside, outside))
        return {p: cur[p] for p in named}, {}, (counts, {p: int(np.count_nonzero((cur[p] != 0) != (before[p] != 0))) for p in named})
    slide = op["op"] == "absorb_prior_slide"
    cur, records, per_job = worldprep.slide_host(before, jobs, op["mode"], crops, op["limit"], keep_of(op) if slide else None,
                                                 op["use"] if slide else "none")
    if slide:
        ret = ([(tuple(a), i, o) for a, i, o in per_job], records)
    else:
        ret = ([tuple(a) for a, i, o in per_job], {p: {f: r[f] for f in ("W", "H", "shift", "origin", "changed")} for p, r in records.items()})
    return {p: cur[p] for p in named}, {p: records[p]["origin"] for p in named}, ret


def default_mpl(W, H):
    return int(min(W * H + 1, max(256, 4 * max(W, H))))


def same(a, b):
    """Equal values: tuples and lists item by item, arrays by shape and by value -- floats by their bytes, so a NaN has to
    be the same NaN.  None equals None only."""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, dict) or isinstance(b, dict):
        return isinstance(a, dict) and isinstance(b, dict) and sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)) and isinstance(b, (tuple, list)) and (any(isinstance(v, (tuple, list, np.ndarray)) or v is None for v in a)
                                                                           or any(isinstance(v, (tuple, list, np.ndarray)) or v is None for v in b)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    x, y = np.asarray(a), np.asarray(b)
    if x.shape != y.shape:
        return False
    if x.dtype.kind == "f" or y.dtype.kind == "f":
        return np.ascontiguousarray(x, np.float64).tobytes() == np.ascontiguousarray(y, np.float64).tobytes()
    return bool(np.array_equal(x, y))


# ------------------------------------------------------------------ the model
class Refused(Exception):
    """What the model expects of an op the library must refuse: the exception's class name and, for FxjpsError, the code."""

    def __init__(self, kind, code=None):
        Exception.__init__(self, kind, code)
        self.kind, self.code = kind, code


class Model(object):
    def __init__(self, contexts=1):
        self.contexts = contexts
        self.grid = None       # the resident grid's bytes
        self.memo = False      # the resident grid is the matrix the last set_grid uploaded: Planner.set_grid skips an equal one
        self.ever_free = None  # cells free at some time since the component forest was last built whole
        self.whole = True      # ... and whether nothing but whole builds made the resident maps
        self.queries = None    # (starts, goals, hchoice, max_path_len) of set_queries
        self.slots = {}        # slot -> bytes
        self.gen = {}          # slot -> generation (fxjps.h: the set and prepare calls bump every slot they name, the refresh calls those not kept)
        self.prior = {}        # index -> {"bytes": uint8 [W][H], "origin": where it lies now, "upload": where it was uploaded,
        #                        "moved": a grow or slide has run since the upload (Planner.prior_origin is the origin then)}
        self.mode = 0
        self.prev = None       # the previous replan_slots while its stored results stand: ids, s, g, hchoice, mpl, gen, status
        self.last = None       # the last batch: kind "resident" / "slots", nq, ids, shapes, and (from run) off, cells

    # -- what the calls do to the state
    def _bump(self, slot):
        self.gen[slot] = self.gen.get(slot, 0) + 1

    def write_resident(self, grid, memo=False, partial=False):
        """Any change of the resident grid: the stored results of replan_frame and replan_slots are void."""
        grid = np.ascontiguousarray(grid, dtype=np.uint8)
        if partial and self.ever_free is not None and self.grid is not None and self.grid.shape == grid.shape:
            self.ever_free = self.ever_free | (grid == 0)
            self.whole = False
        else:
            self.ever_free = grid == 0
            self.whole = True
        self.grid = grid
        self.memo = memo
        self.prev = None

    def batch(self, kind, nq, ids=None):
        self.last = {"kind": kind, "nq": nq, "ids": ids, "off": None, "cells": None,
                     "shapes": [self.slots[i].shape for i in ids] if ids is not None else self.grid.shape}

    def update(self, xy, val):
        g = self.grid.copy()
        W, H = g.shape
        for (x, y), v in zip(xy, val):  # (in order: the last entry of a cell named twice wins; cells off the grid are ignored)
            if 0 <= x < W and 0 <= y < H:
                g[x, y] = 1 if v else 0  # (0 free / non-zero obstacle: the cell update writes 0 or 1)
        self.write_resident(g, partial=True)

    def slot_set(self, slot, grid):
        self.slots[slot] = np.ascontiguousarray(grid, dtype=np.uint8)
        self._bump(slot)

    def slot_empty(self, slot):
        """A cropped job that is not planned or refused: the slot is left empty and its generation moves."""
        self.slots.pop(slot, None)
        self._bump(slot)

    def prior_set(self, p, occ, origin):
        self.prior[p] = {"bytes": np.ascontiguousarray(occ, dtype=np.uint8), "origin": tuple(origin), "upload": tuple(origin), "moved": False}

    def prior_bytes(self):
        return {p: d["bytes"] for p, d in self.prior.items()}

    def slot_refresh(self, slot, grid):
        """-> kept, by the header's rule: the slot holds a grid of the same extents and bytes."""
        old = self.slots.get(slot)
        kept = old is not None and old.shape == grid.shape and np.array_equal(old, grid)
        if not kept:
            self.slot_set(slot, grid)
        return kept

    def predict_reused(self, ids, s, g, hchoice, mpl):
        """out_reused of a replan_slots under the generation rule (fxjps.h: the iff of fxjps_replan_slots)."""
        p = self.prev
        n = len(ids)
        if self.contexts > 1 or p is None or len(p["ids"]) != n or p["hchoice"] != hchoice or p["mpl"] != mpl:
            return [0] * n
        return [int(p["ids"][q] == ids[q] and list(p["s"][q]) == list(s[q]) and list(p["g"][q]) == list(g[q])
                    and p["gen"][q] == self.gen.get(ids[q], 0)) for q in range(n)]

    def same_args(self, q, ids, s, g, hchoice, mpl):
        p = self.prev
        return (p is not None and len(p["ids"]) == len(ids) and p["hchoice"] == hchoice and p["mpl"] == mpl and p["ids"][q] == ids[q]
                and list(p["s"][q]) == list(s[q]) and list(p["g"][q]) == list(g[q]))

    def replanned(self, ids, s, g, hchoice, mpl):
        self.batch("slots", len(ids), list(ids))
        self.prev = None if self.contexts > 1 else {"ids": list(ids), "s": [list(v) for v in s], "g": [list(v) for v in g], "hchoice": hchoice,
                                                    "mpl": mpl, "gen": [self.gen.get(i, 0) for i in ids], "status": None}


# ------------------------------------------------------------------ one op on the model: the state afterwards, and what to expect
def expect(m, op, oracle=None):
    """Apply `op` to model m.  -> a dict of what the call must return (keys depend on the op; "csr" needs the oracle and is
    left out without one).  Raises Refused for an op the library must refuse; the model is unchanged then."""
    k = op["op"]
    e = {}

    def plan_on(grid, s, g, h, mpl):
        if oracle is not None:
            e["csr"] = csr(oracle, grid, s, g, h, mpl)

    def need_grid():
        if m.grid is None:
            raise Refused("FxjpsError", E_NOGRID)

    if k == "set_grid":
        mat = grid_of(op["g"])
        occ = (mat == 1).astype(np.uint8)
        e["skipped"] = m.memo and m.grid is not None and m.grid.shape == occ.shape and np.array_equal(m.grid, occ)
        if not e["skipped"]:
            m.write_resident(occ, memo=True)
    elif k == "set_grid_occ":
        m.write_resident(grid_of(op["g"]))
    elif k == "set_grid_image":
        m.write_resident(adapters.load_image(gray_of(op["gray"])))
    elif k in ("prepare_grid", "prepare_occupancy_msg", "refresh_grid"):
        raw = grid_of(op["raw"])
        grid, e["out"] = prepared(raw, op["start"], op["goal"], op["ifa"], op["variant"])
        if k == "refresh_grid":
            if m.grid is not None and m.grid.shape == grid.shape:
                diff = np.argwhere(m.grid != grid)
                e["diff"] = (diff.astype(np.int32), grid[diff[:, 0], diff[:, 1]])
                e["mode0"] = len(diff) == 0
                m.write_resident(grid, partial=True)
            else:
                e["diff"], e["mode0"] = None, False
                m.write_resident(grid)
        else:
            m.write_resident(grid)
    elif k == "update_cells":
        need_grid()
        m.update(op["xy"], op["val"])
    elif k in ("get_grid", "publish_map", "snapshot_image"):
        need_grid()
    elif k == "plan_batch":
        if op["hchoice"] not in (1, 2):
            raise Refused("TypeError")
        need_grid()
        W, H = m.grid.shape
        plan_on(m.grid, op["s"], op["g"], op["hchoice"], op["mpl"] if op["mpl"] is not None else W * H + 1)
        m.prev = None
        m.batch("resident", len(op["s"]))
    elif k in ("plan_one", "plan", "jps1_method"):
        if k == "jps1_method":  # (set_grid, then plan_one; the record's "g" is the matrix, "g2" the goal)
            expect(m, {"op": "set_grid", "g": op["g"]})
        need_grid()
        W, H = m.grid.shape
        plan_on(m.grid, [op["s"]], [op["g2"] if k == "jps1_method" else op["g"]], op["hchoice"], W * H + 1)
        m.prev = None
        m.batch("resident", 1)
    elif k == "set_queries":
        need_grid()
        m.queries = ([list(v) for v in op["s"]], [list(v) for v in op["g"]], op["hchoice"], op["mpl"])
        m.prev = None  # (the call drops the stored results of both replan calls)
    elif k == "replan_frame":
        if m.queries is None:
            raise Refused("FxjpsError", E_ARG)
        need_grid()
        m.update(op["xy"], op["val"])
        s, g, h, mpl = m.queries
        plan_on(m.grid, s, g, h, mpl)
        m.batch("resident", len(s))
    elif k == "replan_frame_raw":
        m.memo = False  # (Planner forgets the matrix set_grid uploaded before it makes this call, whatever becomes of it)
        raw = grid_of(op["raw"])
        grid, e["out"] = prepared(raw, op["start"], op["goal"], op["ifa"], op["variant"])
        if m.queries is None or m.grid is None or m.grid.shape != grid.shape:
            raise Refused("FxjpsError", E_ARG)
        diff = np.argwhere(m.grid != grid)
        e["diff"], e["mode0"] = (diff.astype(np.int32), grid[diff[:, 0], diff[:, 1]]), len(diff) == 0
        m.write_resident(grid, partial=True)
        s, g, h, mpl = m.queries
        plan_on(m.grid, s, g, h, mpl)
        m.batch("resident", len(s))
    elif k == "set_grid_slot":
        m.slot_set(op["slot"], (grid_of(op["g"]) == 1).astype(np.uint8))
    elif k == "clear_grid_slot":
        m.slots.pop(op["slot"], None)
        m._bump(op["slot"])
    elif k == "set_grid_slots":
        for slot, g in op["jobs"]:
            m.slot_set(slot, (grid_of(g) == 1).astype(np.uint8))
    elif k == "refresh_grid_slots":
        e["kept"] = [m.slot_refresh(slot, (grid_of(g) == 1).astype(np.uint8)) for slot, g in op["jobs"]]
    elif k in ("prepare_slots", "refresh_slots", "prepare_slots_world", "refresh_slots_world", "prepare_slots_cropped", "refresh_slots_cropped"):
        done = []  # (every job is computed before a slot is written: a whole-call refusal leaves the model as it was)
        for j in op["jobs"]:
            tail = ()
            if k.endswith("_cropped"):
                grid, out, w, tail = refusing(crop_prepared, world_job(j), m.prior_bytes())
            elif k.endswith("_world"):
                wj = world_job(j)
                grid, out, w = refusing(lambda: world_prepared(wj, named_prior(m.prior_bytes(), wj)))
            else:
                grid, out = prepared(grid_of(j["raw"]), j["start"], j["goal"], j["ifa"], j["variant"])
                w = ()
            done.append((grid, out, w, tail))
        outs = []
        for j, (grid, out, w, tail) in zip(op["jobs"], done):
            if grid is None:  # (a cropped job that is not planned, or refused on its own: fxjps.h, the cases 1 and 2)
                m.slot_empty(j["slot"])
                outs.append(out + ((False,) if k.startswith("refresh") else ()) + w + tail)
            elif k.startswith("refresh"):
                outs.append(out + (True, m.slot_refresh(j["slot"], grid)) + w + tail)
            else:
                m.slot_set(j["slot"], grid)
                outs.append(out + (True,) + w + tail)
        e["outs"] = outs
    elif k in ("set_prior_map", "set_prior_image"):
        from fuxi_planner_amd import worldprep
        occ = grid_of(op["g"]) > 0 if k == "set_prior_map" else worldprep.prior_from_image(gray_of(op["gray"]))
        m.prior_set(op["prior"], occ, op.get("origin", ORI_PRE))  # (the moved origin is forgotten with the old entry)
    elif k == "clear_prior_map":
        m.prior.pop(op["prior"], None)
    elif k in ("get_prior_map", "prior_origin"):
        if k == "get_prior_map" and op["prior"] not in m.prior:
            raise Refused("FxjpsError", E_ARG)
    elif k in ("absorb_prior", "absorb_prior_grow", "absorb_prior_slide"):
        # (only the named priors are written: no slot, no generation, no stored result, not the resident grid, not m.last)
        after, origin, e["ret"] = refusing(fold_of, m.prior_bytes(), op)
        for p, b in after.items():
            m.prior[p] = dict(m.prior[p], bytes=b)
            if p in origin:
                m.prior[p].update(origin=tuple(origin[p]), moved=True)
    elif k == "check_paths_slots":
        L = m.last
        if L is None or L["kind"] != "slots" or any(i not in m.slots for i in L["ids"]):
            raise Refused("FxjpsError", E_ARG)
        if L["off"] is not None:  # (the slots as they are NOW: they may have been rewritten since the batch)
            from fuxi_planner_amd import waypoints
            e["checks"] = [waypoints.check_path(L["cells"][L["off"][q]:L["off"][q + 1]], m.slots[L["ids"][q]], op["shift"]) for q in range(L["nq"])]
    elif k in ("plan_batch_slots", "replan_slots", "jps1_method_many"):
        if k == "jps1_method_many":
            expect(m, {"op": "refresh_grid_slots", "jobs": [[v, c[0]] for v, c in enumerate(op["calls"])]})
            ids, s, g = list(range(len(op["calls"]))), [c[1] for c in op["calls"]], [c[2] for c in op["calls"]]
            h, mpl = op["hchoice"], max(default_mpl(*m.slots[i].shape) for i in ids)
        else:
            ids, s, g, h, mpl = op["ids"], op["s"], op["g"], op["hchoice"], op["mpl"]
        if h not in (1, 2):
            raise Refused("TypeError")
        if any(i not in m.slots for i in ids):
            raise Refused("FxjpsError", E_ARG)
        plan_on([m.slots[i] for i in ids], s, g, h, mpl)
        if k == "plan_batch_slots":
            m.prev = None
            m.batch("slots", len(ids), list(ids))
        else:
            e["reused"] = m.predict_reused(ids, s, g, h, mpl)
            e["same"] = [m.same_args(q, ids, s, g, h, mpl) for q in range(len(ids))]
            e["stored"] = None if m.prev is None else m.prev["status"]
            m.replanned(ids, s, g, h, mpl)
    elif k == "set_slot_reuse":
        new = {"generation": 0, "tiles": 1}[op["mode"]]
        if new != m.mode:
            m.mode, m.prev = new, None
    elif k in ("publish_slots", "get_grid_slot"):
        for s_ in (op["slots"] if k == "publish_slots" else [op["slot"]]):
            if s_ not in m.slots:
                raise Refused("FxjpsError", E_ARG)
    elif k in ("select_st_batch", "select_ccst_batch", "select_slots_batch", "tick_outputs_slots"):
        L = m.last
        slots_form = k in ("select_slots_batch", "tick_outputs_slots")
        if L is None or op["nq"] != L["nq"] or (slots_form and L["kind"] != "slots") or (k == "select_ccst_batch" and L["kind"] != "resident"):
            raise Refused("FxjpsError", E_ARG)
    elif k == "fresh_set_queries":
        pass  # (another handle: refused there, nothing here)
    else:
        raise ValueError("unknown op %r" % (k,))
    if "csr" in e:  # (the paths the batch leaves resident: what the waypoint calls and check_paths_slots run on)
        m.last["off"], m.last["cells"] = e["csr"][0], e["csr"][1]
    return e


# ------------------------------------------------------------------ the generator
GRID_WRITERS = ("set_grid", "set_grid_occ", "set_grid_image", "prepare_grid", "prepare_occupancy_msg", "refresh_grid")
INVALIDATORS = ("set_grid", "set_grid_occ", "set_grid_image", "prepare_grid", "prepare_occupancy_msg", "refresh_grid", "update_cells",
                "plan_batch", "plan_one", "plan", "set_queries")
KINDS = GRID_WRITERS + ("update_cells", "get_grid", "publish_map", "snapshot_image", "plan_batch", "plan_one", "plan", "set_queries",
                        "replan_frame", "replan_frame_raw", "set_grid_slot", "clear_grid_slot", "set_grid_slots", "refresh_grid_slots",
                        "prepare_slots", "refresh_slots", "prepare_slots_world", "refresh_slots_world", "plan_batch_slots", "replan_slots",
                        "set_slot_reuse", "publish_slots", "get_grid_slot", "select_st_batch", "select_ccst_batch", "select_slots_batch",
                        "tick_outputs_slots", "fresh_set_queries")
FRAME_DROPPERS = INVALIDATORS + ("plan_batch_slots", "replan_slots")                   # between two replan_frame calls
SLOT_DROPPERS = INVALIDATORS + ("plan_batch_slots", "replan_frame", "replan_frame_raw")  # between two replan_slots calls ("tiles": and set_slot_reuse)
REFUSALS = ("bad_hchoice", "empty_slot", "raw_other_extents", "wrong_nq")
NSLOTS = 6                    # the sequences write slots 0 .. 5
EMPTY_SLOTS = (253, 254, 255)  # ... and name these, which nothing writes, where a batch must be refused


class _Gen(object):
    def __init__(self, seed, profile):
        self.rs = np.random.RandomState(1000003 * (ALL_PROFILES.index(profile) + 1) + seed)
        self.profile, self.seed = profile, seed
        self.m = Model(2 if profile in ("two_contexts", "world_two_contexts") else 1)
        self.ops = []
        self.count = {}
        self.raw = None      # the recipe and arguments of the last prepare / refresh of the resident grid
        self.slot_raw = {}   # slot -> the job record that prepared it last
        self.slot_spec = {}  # slot -> the recipe set_grid_slot(s) wrote last
        self.seeds = 0

    def ri(self, lo, hi):
        return int(self.rs.randint(lo, hi + 1))

    def side(self, big=None):
        r = self.rs.random_sample()
        if big is True:
            return self.ri(65, 140)
        if r < 0.04:
            return 1
        if r < 0.60:
            return self.ri(2, 24)
        if r < 0.88:
            return self.ri(25, 64)
        return self.ri(65, 140)

    def spec(self, W=None, H=None, p=None):
        self.seeds += 1
        return {"W": W or self.side(), "H": H or self.side(), "seed": self.ri(0, 2 ** 30) ^ self.seeds,
                "p": float(self.rs.choice([0.0, 0.05, 0.2, 0.35])) if p is None else p, "set": []}

    def changed(self, spec, n, values=(0, 1)):
        """The recipe with n more cells set."""
        out = dict(spec, set=[list(c) for c in spec["set"]])
        for _ in range(n):
            out["set"].append([self.ri(0, spec["W"] - 1), self.ri(0, spec["H"] - 1), int(self.rs.choice(values))])
        return out

    def cell(self, grid, free=True):
        W, H = grid.shape
        r = self.rs.random_sample()
        if r < 0.08:  # off the grid, on any side
            return [self.ri(-2, W + 1), self.ri(-2, H + 1)]
        if free and r < 0.9:
            c = np.argwhere(grid == 0)
            if len(c):
                x, y = c[self.ri(0, len(c) - 1)]
                return [int(x), int(y)]
        return [self.ri(0, W - 1), self.ri(0, H - 1)]

    def queries(self, grids, n):
        """n (start, goal) pairs, query q on grids[q]: mostly free cells, some occupied, some off the grid."""
        return [self.cell(grids[q]) for q in range(n)], [self.cell(grids[q], free=self.rs.random_sample() < 0.8) for q in range(n)]

    def emit(self, op):
        try:
            e = expect(self.m, op)
        except Refused:
            e = None
        self.ops.append(op)
        self.count[op["op"]] = self.count.get(op["op"], 0) + 1
        return e

    # -- resident grid
    def prep_args(self, spec=None, ifa=None, variant=None):
        """A raw recipe with start and goal whose preparation neither raises on the host nor is refused: both cells come
        out inside the prepared grid."""
        for _ in range(50):
            sp = spec or self.spec(W=min(self.side(), 90), H=min(self.side(), 90), p=float(self.rs.choice([0.0, 0.05, 0.2])))
            raw = grid_of(sp)
            i = self.ri(0, 2) if ifa is None else ifa
            v = self.ri(0, 1) if variant is None else variant
            s = [self.ri(-2, sp["W"] + 1), self.ri(-2, sp["H"] + 1)]
            g = [self.ri(-2, sp["W"] + 1), self.ri(-2, sp["H"] + 1)]
            try:
                grid, out = prepared(raw, s, g, i, v)
            except (IndexError, ValueError):
                continue
            if all(0 <= out[a][b] < grid.shape[b] for a in (0, 1) for b in (0, 1)) and max(grid.shape) <= 160:
                return {"raw": sp, "start": s, "goal": g, "ifa": i, "variant": v}
        raise AssertionError("no preparable job drawn")

    def op_grid(self, kind=None, like=None, other=False):
        """A call that makes a grid resident.  like: of the extents of the resident one; other: of other extents."""
        kind = kind or str(self.rs.choice(GRID_WRITERS))
        cur = self.m.grid
        if kind in ("set_grid", "set_grid_occ"):
            if like and cur is not None:
                sp = self.spec(W=cur.shape[0], H=cur.shape[1])
            else:
                sp = self.spec()
                while other and cur is not None and (sp["W"], sp["H"]) == cur.shape:
                    sp = self.spec()
            if kind == "set_grid":
                sp = self.changed(sp, 3, (1, 100))  # (a 100 is free for jps1.py: only == 1 is an obstacle)
                self.last_set = sp
            else:
                sp = self.changed(sp, 3, (7, 100, 255, 0))  # (bytes other than 0 / 1: every one an obstacle)
            return self.emit({"op": kind, "g": sp})
        if kind == "set_grid_image":
            rows, cols = (cur.shape[1], cur.shape[0]) if like and cur is not None else (self.side(), self.side())
            return self.emit({"op": kind, "gray": {"rows": rows, "cols": cols, "seed": self.ri(0, 2 ** 30)}})
        a = self.prep_args()
        self.raw = a
        return self.emit(dict(a, op=kind))

    def op_set_grid_again(self):
        """set_grid of the matrix uploaded last: skipped while nothing else wrote the grid, uploaded otherwise."""
        sp = getattr(self, "last_set", None)
        if sp is None:
            return self.op_grid("set_grid")
        return self.emit({"op": "set_grid", "g": sp})

    def op_refresh(self):
        """refresh_grid: the same raw, a few cells changed, or other extents."""
        r = self.rs.random_sample()
        if self.raw is None or r < 0.2:
            a = self.prep_args()
        elif r < 0.5:
            a = dict(self.raw)
        else:
            a = dict(self.raw, raw=self.changed(self.raw["raw"], self.ri(1, 4)))
            try:
                grid, out = prepared(grid_of(a["raw"]), a["start"], a["goal"], a["ifa"], a["variant"])
            except (IndexError, ValueError):
                a = dict(self.raw)
        self.raw = a
        return self.emit(dict(a, op="refresh_grid"))

    def blob(self, grid, at, v):
        W, H = grid.shape
        r = self.ri(0, 2)
        return [[x, y] for x in range(at[0] - r, at[0] + r + 1) for y in range(at[1] - r, at[1] + r + 1)], v

    def cells_update(self):
        """A cell list for update_cells / replan_frame: random cells, some named twice, some off the grid, and a blob set
        or cleared between the start and the goal of a stored query (what a stale stored path would miss)."""
        g = self.m.grid
        W, H = g.shape
        xy, val = [], []
        for _ in range(self.ri(0, 6)):
            xy.append([self.ri(-1, W), self.ri(-1, H)])
            val.append(int(self.rs.choice([0, 1, 1, 3])))
        if xy and self.rs.random_sample() < 0.5:
            xy.append(list(xy[0]))
            val.append(1 - min(val[0], 1))
        if self.m.queries is not None and self.rs.random_sample() < 0.7:
            s, go = self.m.queries[0], self.m.queries[1]
            q = self.ri(0, len(s) - 1)
            t = self.rs.random_sample()
            at = [int(s[q][0] + t * (go[q][0] - s[q][0])), int(s[q][1] + t * (go[q][1] - s[q][1]))]
            b, v = self.blob(g, at, self.ri(0, 1))
            xy += b
            val += [v] * len(b)
        return xy, val

    def op_update(self):
        xy, val = self.cells_update()
        return self.emit({"op": "update_cells", "xy": xy, "val": val, "rebuild": bool(self.rs.random_sample() < 0.5)})

    # -- planning on the resident grid
    def op_plan_batch(self, n=None):
        n = int(self.rs.choice([0, 1, 1, 2, 7, 20, 48])) if n is None else n
        s, g = self.queries([self.m.grid] * n, n)
        return self.emit({"op": "plan_batch", "s": s, "g": g, "hchoice": self.ri(1, 2), "mpl": [None, 6, 400][self.ri(0, 2)]})

    def op_plan_one(self, kind):
        s, g = self.queries([self.m.grid], 1)
        return self.emit({"op": kind, "s": s[0], "g": g[0], "hchoice": self.ri(1, 2)})

    def op_set_queries(self):
        n = int(self.rs.choice([1, 3, 9, 24]))
        s, g = self.queries([self.m.grid] * n, n)
        return self.emit({"op": "set_queries", "s": s, "g": g, "hchoice": self.ri(1, 2), "mpl": MPLS[self.ri(0, 1)]})

    def op_replan_frame(self):
        if self.m.queries is None:
            self.op_set_queries()
        xy, val = ([], []) if self.rs.random_sample() < 0.4 else self.cells_update()
        return self.emit({"op": "replan_frame", "xy": xy, "val": val})

    def op_replan_frame_raw(self):
        """On a prepared resident grid with stored queries: the same raw or a few cells changed, under the same arguments."""
        if self.raw is None or self.m.grid is None or prepared(grid_of(self.raw["raw"]), self.raw["start"], self.raw["goal"], self.raw["ifa"],
                                                               self.raw["variant"])[0].shape != self.m.grid.shape:
            self.op_grid("prepare_grid")
        if self.m.queries is None:
            self.op_set_queries()
        a = dict(self.raw)
        if self.rs.random_sample() < 0.6:
            b = dict(a, raw=self.changed(a["raw"], self.ri(1, 4)))
            try:
                if prepared(grid_of(b["raw"]), b["start"], b["goal"], b["ifa"], b["variant"])[0].shape == self.m.grid.shape:
                    a = b
            except (IndexError, ValueError):
                pass
        self.raw = a
        return self.emit(dict(a, op="replan_frame_raw"))

    # -- slots
    def slot_job(self, slot, world=False):
        old = self.slot_raw.get(slot)
        r = self.rs.random_sample()
        if old is not None and ("at" in old) == world and r < 0.75:
            j = dict(old)
            if r < 0.35:
                j["raw"] = self.changed(old["raw"], self.ri(1, 3))
            try:
                self.check_job(j, world)
                return j
            except (IndexError, ValueError, AssertionError):
                pass
        for _ in range(50):
            a = self.prep_args(self.spec(W=min(self.side(), 60), H=min(self.side(), 60), p=float(self.rs.choice([0.0, 0.05, 0.2]))))
            j = dict(a, slot=slot)
            if world:
                j["start"] = [max(a["start"][0], 0), max(a["start"][1], 0)]
                j["goal"] = [max(a["goal"][0], 0), max(a["goal"][1], 0)]
                j["prior"] = bool(self.rs.random_sample() < 0.7)
                j["at"] = [self.ri(-6, 10), self.ri(-6, 10)]
            try:
                self.check_job(j, world)
                return j
            except (IndexError, ValueError, AssertionError):
                continue
        raise AssertionError("no preparable slot job drawn")

    def check_job(self, j, world):
        if world:
            grid, out, w = world_prepared(world_job(j), self.m.prior[0]["bytes"] if j["prior"] else None)
        else:
            grid, out = prepared(grid_of(j["raw"]), j["start"], j["goal"], j["ifa"], j["variant"])
        assert all(0 <= out[a][b] < grid.shape[b] for a in (0, 1) for b in (0, 1)) and max(grid.shape) <= 160

    def op_slot_jobs(self, kind):
        world = kind.endswith("_world")
        if world and 0 not in self.m.prior:
            self.emit({"op": "set_prior_map", "prior": 0, "g": self.spec(W=self.ri(5, 40), H=self.ri(5, 40), p=0.1)})
        slots = sorted(self.rs.choice(NSLOTS, self.ri(1, 3), replace=False).tolist())
        jobs = [self.slot_job(s, world) for s in slots]
        for j in jobs:
            self.slot_raw[j["slot"]] = j
            self.slot_spec.pop(j["slot"], None)
        return self.emit({"op": kind, "jobs": jobs})

    def slot_grid(self, slot, equal=None):
        """A recipe for set_grid_slot(s) / refresh_grid_slots: the one written last (equal bytes), that with cells changed,
        or a new one."""
        old = self.slot_spec.get(slot)
        r = self.rs.random_sample() if equal is None else (0.0 if equal else 0.5)
        if old is not None and r < 0.4:
            sp = old
        elif old is not None and r < 0.7:
            sp = self.changed(old, self.ri(1, 3))
        else:
            sp = self.changed(self.spec(), 2, (1, 100))
        return sp

    def op_grid_slots(self, kind, slots=None, equal=None):
        if kind == "set_grid_slot":
            slot = self.ri(0, NSLOTS - 1) if slots is None else slots[0]
            sp = self.slot_grid(slot, equal)
            self.slot_spec[slot] = sp
            self.slot_raw.pop(slot, None)
            return self.emit({"op": kind, "slot": slot, "g": sp})
        slots = sorted(self.rs.choice(NSLOTS, self.ri(1, 4), replace=False).tolist()) if slots is None else slots
        jobs = []
        for s in slots:
            sp = self.slot_grid(s, equal)
            self.slot_spec[s] = sp
            self.slot_raw.pop(s, None)
            jobs.append([s, sp])
        return self.emit({"op": kind, "jobs": jobs})

    def op_clear_slot(self):
        live = sorted(self.m.slots)
        if len(live) <= 3:
            return self.op_grid_slots("set_grid_slots")
        slot = live[self.ri(0, len(live) - 1)]
        self.slot_spec.pop(slot, None)
        self.slot_raw.pop(slot, None)
        return self.emit({"op": "clear_grid_slot", "slot": slot})

    def slots_batch(self):
        live = sorted(self.m.slots)
        n = int(self.rs.choice([1, 2, 5, 12, 30, 48]))
        ids = [live[self.ri(0, len(live) - 1)] for _ in range(n)]
        s, g = self.queries([self.m.slots[i] for i in ids], n)
        return {"ids": ids, "s": s, "g": g, "hchoice": self.ri(1, 2), "mpl": MPLS[self.ri(0, 1) if self.rs.random_sample() < 0.3 else 1]}

    def op_plan_batch_slots(self):
        return self.emit(dict(self.slots_batch(), op="plan_batch_slots"))

    def op_replan_slots(self, fresh=None, move=0.4):
        """The previous replan_slots again -- verbatim, or with one query moved -- unless it named a slot that is empty now."""
        last = getattr(self, "last_replan", None)
        if fresh is None or last is None or any(i not in self.m.slots for i in last["ids"]):
            fresh = last is None or any(i not in self.m.slots for i in last["ids"]) or self.rs.random_sample() < 0.2
        if fresh:
            b = self.slots_batch()
        else:
            b = {k: (list(v) if isinstance(v, list) else v) for k, v in last.items() if k != "op"}
            if self.rs.random_sample() < move:
                q = self.ri(0, len(b["ids"]) - 1)
                b["s"] = [list(v) for v in b["s"]]
                b["s"][q] = self.cell(self.m.slots[b["ids"][q]])
        self.last_replan = dict(b)
        return self.emit(dict(b, op="replan_slots"))

    def rewrite_slot_of_replan(self, equal):
        """One slot the last replan_slots named, written again: with equal bytes (refresh keeps it: its queries are handed
        back; set bumps it: they are searched) or with other bytes."""
        last = getattr(self, "last_replan", None)
        if last is None:
            return self.op_grid_slots("refresh_grid_slots")
        slot = last["ids"][self.ri(0, len(last["ids"]) - 1)]
        cur = self.m.slots.get(slot)
        if cur is None:
            return self.op_grid_slots("refresh_grid_slots")
        kind = str(self.rs.choice(["refresh_grid_slots", "set_grid_slot", "set_grid_slots"]))
        # the slot's present bytes as a recipe: all of them listed (the slot may have been prepared from a raw map)
        sp = self.slot_spec.get(slot)
        if sp is None:
            ones = np.argwhere(cur != 0)
            sp = {"W": cur.shape[0], "H": cur.shape[1], "seed": 0, "p": 0.0, "set": [[int(x), int(y), 1] for x, y in ones]}
        if not equal:
            for _ in range(20):
                sp2 = self.changed(sp, self.ri(1, 3))
                if not np.array_equal((grid_of(sp2) == 1), cur != 0):
                    sp = sp2
                    break
        self.slot_spec[slot] = sp
        self.slot_raw.pop(slot, None)
        if kind == "set_grid_slot":
            return self.emit({"op": kind, "slot": slot, "g": sp})
        return self.emit({"op": kind, "jobs": [[slot, sp]]})

    def op_readback(self, kind):
        live = sorted(self.m.slots)
        if kind == "get_grid_slot":
            return self.emit({"op": kind, "slot": live[self.ri(0, len(live) - 1)]})
        if kind == "publish_slots":
            n = self.ri(1, 4)
            return self.emit({"op": kind, "slots": [live[self.ri(0, len(live) - 1)] for _ in range(n)], "msg": bool(self.ri(0, 1)),
                              "channels": [None, 1, 3][self.ri(0, 2)]})
        if kind == "snapshot_image":
            return self.emit({"op": kind, "channels": [1, 3][self.ri(0, 1)]})
        return self.emit({"op": kind})

    # -- the resident-path forms
    def wp_args(self, nq, slots_form):
        L = self.m.last
        a = {"nq": nq, "seed": self.ri(0, 2 ** 30), "end_occu": bool(self.ri(0, 1)), "prev": bool(self.ri(0, 1))}
        if slots_form:
            a["form"] = "none"  # the resident paths as paths=None, or as (offsets, None): op_wp takes them in turn
            ok = L is not None and L["kind"] == "slots" and all(i in self.m.slots for i in L["ids"])
            # (the ccst rule reads the slot as it is now, other extents included; a ccst query on an empty slot is refused)
            a["rule"] = [self.ri(0, 1) if ok else 0 for _ in range(nq)]
        return a

    def op_wp(self, kind, wrong=False):
        L = self.m.last
        slots_form = kind in ("select_slots_batch", "tick_outputs_slots")
        want = "slots" if slots_form else "resident"
        if L is None or L["nq"] < 1 or (L["kind"] != want and kind != "select_st_batch"):
            if slots_form:
                self.op_plan_batch_slots() if self.rs.random_sample() < 0.5 else self.op_replan_slots()
            else:
                self.op_plan_batch()
            L = self.m.last
            if L["nq"] < 1:
                self.emit({"op": "plan_batch", "s": [[0, 0]], "g": [[0, 0]], "hchoice": 2, "mpl": None})
                L = self.m.last
        a = self.wp_args(L["nq"] + (1 if wrong else 0), slots_form)
        if slots_form and not wrong:
            self.count["form: " + kind] = self.count.get("form: " + kind, 0) + 1
            a["form"] = ("none", "offsets")[self.count["form: " + kind] % 2]
        return self.emit(dict(a, op=kind))

    # -- refusals
    def op_refusal(self, which):
        self.count["refused: " + which] = self.count.get("refused: " + which, 0) + 1
        if which == "bad_hchoice":
            if self.rs.random_sample() < 0.5:
                return self.emit({"op": "plan_batch", "s": [[0, 0]], "g": [[0, 0]], "hchoice": 3, "mpl": None})
            return self.emit(dict(self.slots_batch(), hchoice=3, op="replan_slots"))
        if which == "empty_slot":
            b = self.slots_batch()
            b["ids"][self.ri(0, len(b["ids"]) - 1)] = EMPTY_SLOTS[self.ri(0, 2)]  # (never written)
            return self.emit(dict(b, op=str(self.rs.choice(["plan_batch_slots", "replan_slots"]))))
        if which == "raw_other_extents":
            if self.m.queries is None:
                self.op_set_queries()
            for _ in range(50):
                a = self.prep_args()
                if prepared(grid_of(a["raw"]), a["start"], a["goal"], a["ifa"], a["variant"])[0].shape != self.m.grid.shape:
                    return self.emit(dict(a, op="replan_frame_raw"))
            raise AssertionError("no raw of other extents drawn")
        kind = str(self.rs.choice(["select_st_batch", "select_ccst_batch", "select_slots_batch", "tick_outputs_slots"]))
        return self.op_wp(kind, wrong=True)

    # -- the sequence
    def forced(self):
        """What every sequence holds whatever is drawn: a 1-wide resident grid, one with a side of 65 .. 140 whose H is no
        multiple of 64, two resident grids of equal extents in a row and two of different extents, four slots of different
        shapes -- one 1-wide, one with a long side."""
        if self.ri(0, 1):  # (half of the sequences begin small: what a first call sizes for its grid is then too small later)
            self.emit({"op": "set_grid_occ", "g": self.changed(self.spec(W=self.ri(3, 24), H=self.ri(3, 24), p=0.2), 3, (7, 255))})
        else:
            self.big_grid()
        self.op_set_queries()
        self.emit({"op": "replan_frame", "xy": [], "val": []})
        self.emit({"op": "set_grid_slots", "jobs": [[0, self.spec(W=1, H=self.ri(2, 70))], [1, self.spec(W=self.ri(65, 140), H=self.ri(3, 40), p=0.2)],
                                                    [2, self.spec(W=self.ri(2, 30), H=self.ri(65, 130), p=0.05)], [3, self.spec(W=self.ri(5, 40), H=self.ri(5, 40), p=0.35)]]})
        for s, j in enumerate(self.ops[-1]["jobs"]):
            self.slot_spec[j[0]] = j[1]
        self.op_replan_slots(fresh=True)

    def big_grid(self):
        H = self.ri(65, 140)
        H += 1 if H % 64 == 0 else 0
        self.emit({"op": "set_grid_occ", "g": self.changed(self.spec(W=self.ri(66, 140), H=H, p=0.2), 3, (7, 255))})

    def forced_later(self, which):
        if which == 0:  # a grid whose lines cross a 64-bit word, a 1-wide one, then one of other extents
            self.big_grid()
            self.op_plan_batch(0)
            self.emit({"op": "set_grid_occ", "g": self.spec(W=1, H=self.ri(2, 80), p=0.05)})
            self.op_plan_batch(1)
            self.op_grid("set_grid", other=True)
        elif which == 1:  # two grids of equal extents in a row: the owner / changed marks are kept
            self.op_grid("set_grid_occ")
            self.op_update()
            self.op_grid(str(self.rs.choice(["set_grid", "set_grid_occ", "set_grid_image"])), like=True)
        elif which == 2:  # an equal matrix: skipped (the stored slot results stand: out_reused shows it), uploaded again after an update
            self.op_grid("set_grid")
            self.op_replan_slots(fresh=False if getattr(self, "last_replan", None) is not None else None, move=0.0)
            self.op_set_grid_again()
            self.op_replan_slots(fresh=False, move=0.0)
            self.op_update()
            self.op_set_grid_again()
        elif which == 3:  # a refusal in the middle of a tick: the resident paths and the stored results stay
            self.op_slot_jobs("refresh_slots")
            self.op_replan_slots()
            self.op_refusal("empty_slot")
            self.op_wp("select_slots_batch")
            self.op_replan_slots(fresh=False)
        elif which < 8:  # four of the calls that drop stored frame results, in turn over the seeds of a profile
            self.frame_tick(FRAME_DROPPERS[(4 * self.seed + which - 4) % len(FRAME_DROPPERS)])
        elif which < 12:  # ... and of those that drop stored slot results
            kinds = SLOT_DROPPERS + (("set_slot_reuse",) if self.profile == "tiles" else ())
            self.slots_drop_tick(kinds[(4 * self.seed + which - 8) % len(kinds)])

    def do_kind(self, kind):
        """One op of `kind`, of those that must drop stored results."""
        if kind in ("set_grid", "set_grid_occ", "set_grid_image"):
            return self.op_grid(kind, like=True)
        if kind in ("prepare_grid", "prepare_occupancy_msg"):
            return self.op_grid(kind)
        if kind == "update_cells" and self.m.queries is not None:
            # (the goals of the stored queries change sides: every path to one of them ends, or begins to exist)
            g0 = self.m.grid
            goals = [c for c in self.m.queries[1] if 0 <= c[0] < g0.shape[0] and 0 <= c[1] < g0.shape[1]]
            return self.emit({"op": "update_cells", "xy": [list(c) for c in goals], "val": [int(g0[c[0], c[1]] == 0) for c in goals],
                              "rebuild": bool(self.ri(0, 1))})
        if kind == "set_slot_reuse":
            return self.emit({"op": kind, "mode": "generation" if self.m.mode else "tiles"})
        return {"refresh_grid": self.op_refresh, "update_cells": self.op_update, "plan_batch": self.op_plan_batch,
                "plan_one": lambda: self.op_plan_one("plan_one"), "plan": lambda: self.op_plan_one("plan"), "set_queries": self.op_set_queries,
                "plan_batch_slots": self.op_plan_batch_slots, "replan_slots": self.op_replan_slots, "replan_frame": self.op_replan_frame,
                "replan_frame_raw": self.op_replan_frame_raw}[kind]()

    def before_kind(self, kind):
        """What an op of `kind` needs in place, made before the stored results it is to drop."""
        if kind in ("replan_frame", "replan_frame_raw") and self.m.queries is None:
            self.op_set_queries()
        if kind == "replan_frame_raw" and (self.raw is None or prepared(grid_of(self.raw["raw"]), self.raw["start"], self.raw["goal"], self.raw["ifa"],
                                                                        self.raw["variant"])[0].shape != self.m.grid.shape):
            self.op_grid("prepare_grid")

    def frame_tick(self, kind=None):
        """Stored frame results, one call that must drop them, the frame again with nothing to apply."""
        kind = kind or FRAME_DROPPERS[self.ri(0, len(FRAME_DROPPERS) - 1)]
        self.before_kind(kind)
        g0 = self.m.grid
        if self.m.queries is None or self.rs.random_sample() < 0.7 or not all(0 <= c[0] < g0.shape[0] and 0 <= c[1] < g0.shape[1]
                                                                               for c in self.m.queries[0]):
            self.op_set_queries()  # (queries of this grid: stored ones may lie off it, and nothing could go stale)
        self.op_replan_frame()
        self.do_kind(kind)
        return self.emit({"op": "replan_frame", "xy": [], "val": []})

    def slots_drop_tick(self, kind=None):
        """Stored slot results, one call that must drop them, the same batch again."""
        kind = kind or SLOT_DROPPERS[self.ri(0, len(SLOT_DROPPERS) - 1)]
        self.before_kind(kind)
        again = False if getattr(self, "last_replan", None) is not None else None
        self.op_replan_slots(fresh=again, move=0.0)
        self.do_kind(kind)
        return self.op_replan_slots(fresh=False, move=0.0)

    def slots_tick(self):
        """Fleet ticks in a row: one or two of the slots the last replan_slots named are written again -- with the bytes
        they hold or with others -- a call that touches no stored result may follow, and the batch is replanned as it was."""
        if self.m.prev is None:
            self.op_replan_slots(fresh=False if getattr(self, "last_replan", None) is not None else None, move=0.0)
        for _ in range(self.ri(3, 4)):
            for _ in range(self.ri(1, 2)):
                self.rewrite_slot_of_replan(equal=bool(self.rs.random_sample() < 0.35))
            r = self.rs.random_sample()
            if r < 0.2:
                self.op_readback(str(self.rs.choice(["publish_slots", "get_grid_slot", "get_grid", "publish_map"])))
            elif r < 0.4:
                self.op_wp(str(self.rs.choice(["select_slots_batch", "tick_outputs_slots", "select_st_batch"])))
            self.op_replan_slots(fresh=False, move=0.15)

    def step(self):
        m = self.m
        r = self.rs.random_sample()
        if r < 0.07:
            return self.op_refusal(REFUSALS[self.ri(0, len(REFUSALS) - 1)])
        if r < 0.10:
            return self.emit({"op": "fresh_set_queries", "s": [[0, 0]], "g": [[1, 1]], "hchoice": 2, "mpl": 400})
        if r < 0.17:
            return self.op_grid()
        if r < 0.20:
            return self.op_set_grid_again()
        if r < 0.24:
            return self.op_refresh()
        if r < 0.29:
            return self.op_update()
        if r < 0.33:
            return self.op_readback(str(self.rs.choice(["get_grid", "publish_map", "snapshot_image"])))
        if r < 0.37:
            return self.op_plan_batch()
        if r < 0.41:
            return self.op_plan_one(str(self.rs.choice(["plan_one", "plan"])))
        if r < 0.44:
            return self.op_set_queries()
        if r < 0.50:
            return self.op_replan_frame()
        if r < 0.54:
            return self.op_replan_frame_raw()
        if r < 0.58:
            return self.op_grid_slots(str(self.rs.choice(["set_grid_slot", "set_grid_slots", "refresh_grid_slots"])))
        if r < 0.60:
            return self.op_clear_slot()
        if r < 0.66:
            return self.op_slot_jobs(str(self.rs.choice(["prepare_slots", "refresh_slots", "prepare_slots_world", "refresh_slots_world"])))
        if r < 0.67:
            return self.op_plan_batch_slots()
        if r < 0.69:
            return self.op_replan_slots()
        if r < 0.82:
            return self.slots_tick()
        if r < 0.85:
            return self.frame_tick()
        if r < 0.87 and self.profile == "tiles":
            return self.emit({"op": "set_slot_reuse", "mode": str(self.rs.choice(["generation", "tiles"]))})
        if r < 0.90:
            return self.op_readback(str(self.rs.choice(["publish_slots", "get_grid_slot"])))
        if r < 0.96:
            return self.op_wp(str(self.rs.choice(["select_st_batch", "select_ccst_batch", "select_slots_batch", "tick_outputs_slots"])))
        if self.profile == "shim":
            return self.op_shim()
        return self.op_replan_slots()

    def op_shim(self):
        if self.rs.random_sample() < 0.5:
            sp = getattr(self, "last_set", None)
            if sp is None or self.rs.random_sample() < 0.4:
                sp = self.changed(self.spec(), 3, (1, 100))
            self.last_set = sp
            occ = (grid_of(sp) == 1).astype(np.uint8)
            s, g = self.queries([occ], 1)
            return self.emit({"op": "jps1_method", "g": sp, "s": s[0], "g2": g[0], "hchoice": 2})
        calls = []
        for v in range(self.ri(1, 4)):
            sp = self.slot_grid(v)
            self.slot_spec[v] = sp
            self.slot_raw.pop(v, None)
            occ = (grid_of(sp) == 1).astype(np.uint8)
            c = np.argwhere(occ == 0)
            s = [int(t) for t in (c[self.ri(0, len(c) - 1)] if len(c) else (0, 0))]  # (a start off its matrix raises before anything is planned)
            calls.append([sp, s, self.cell(occ)])
        return self.emit({"op": "jps1_method_many", "calls": calls, "hchoice": self.ri(1, 2)})


# ------------------------------------------------------------------ the generator of the world profiles
WORLD_KINDS = ("set_prior_map", "set_prior_image", "clear_prior_map", "get_prior_map", "prior_origin", "absorb_prior", "absorb_prior_grow",
               "absorb_prior_slide", "prepare_slots_cropped", "refresh_slots_cropped", "check_paths_slots")
WORLD_OLD_KINDS = ("prepare_slots_world", "refresh_slots_world", "plan_batch_slots", "replan_slots", "set_slot_reuse", "get_grid_slot", "publish_slots",
                   "select_slots_batch", "tick_outputs_slots")
WORLD_REFUSALS = ("prior_not_set", "grow_past_limit", "slide_empty_window", "window_unnamed_prior", "unequal_ori_pre", "world_cleared_prior")
PRIORS = (0, 1, 15)   # the prior maps the world profiles upload
UNSET_PRIOR = 7       # ... and one they never do
MODES = ("overwrite", "occupied", "known")
USES = ("always", "over_limit", "none")


class _WorldGen(_Gen):
    """The sequences of the world profiles: the shared prior maps and every call that reads them.  Everything lies on the
    lattice ORI_PRE + R * integers, so every quotient of the references' arithmetic is exact."""

    def __init__(self, seed, profile):
        _Gen.__init__(self, seed, profile)
        self.cleared = set()  # priors released and not uploaded again
        self.cropped = {}     # slot -> whether its last job was a cropped one

    # -- geometry
    def xy(self, c):
        return [ORI_PRE[0] + c[0] * R, ORI_PRE[1] + c[1] * R]

    def cell_xy(self, o):
        return [int(round((o[0] - ORI_PRE[0]) / R)), int(round((o[1] - ORI_PRE[1]) / R))]

    def raw_spec(self, p=None):
        sp = self.spec(W=self.ri(3, 24), H=self.ri(3, 24), p=float(self.rs.choice([0.0, 0.05, 0.2, 0.5])) if p is None else p)
        return self.changed(sp, self.ri(0, 3), (0, 1, 7, 255))  # (bytes other than 0 / 1: every one an obstacle)

    def place(self, p, w, h, where=None):
        """Where (cells from ORI_PRE) a w x h raw lies relative to prior p, per axis: inside, across the low or the high
        edge, or wholly outside on either side."""
        d = self.m.prior[p]
        c, ext, at = self.cell_xy(d["origin"]), d["bytes"].shape, []
        for k, n in enumerate((w, h)):
            kind = where[k] if where else str(self.rs.choice(["in", "in", "lo", "hi", "out_lo", "out_hi"]))
            if kind == "in":
                at.append(c[k] + self.ri(0, max(ext[k] - n, 0)))
            elif kind == "lo":
                at.append(c[k] - self.ri(1, max(n - 1, 1)))
            elif kind == "hi":
                at.append(c[k] + ext[k] - self.ri(1, max(n - 1, 1)))
            elif kind == "out_lo":
                at.append(c[k] - n - self.ri(0, 4))
            else:
                at.append(c[k] + ext[k] + self.ri(0, 4))
        return at

    # -- priors
    def op_set_prior(self, p=None, image=None, big=False):
        p = PRIORS[self.ri(0, 2)] if p is None else p
        image = bool(self.rs.random_sample() < 0.3) if image is None else image
        origin = self.xy([self.ri(-8, 8), self.ri(-8, 8)])
        lo = 25 if big else 5
        self.cleared.discard(p)
        if image:
            return self.emit({"op": "set_prior_image", "prior": p, "gray": {"rows": self.ri(lo, 40), "cols": self.ri(lo, 40), "seed": self.ri(0, 2 ** 30)},
                              "origin": origin})
        return self.emit({"op": "set_prior_map", "prior": p, "g": self.spec(W=self.ri(lo, 40), H=self.ri(lo, 40), p=float(self.rs.choice([0.05, 0.1, 0.3]))),
                          "origin": origin})

    def a_prior(self):
        """A prior that is set (one is uploaded when none is)."""
        if not self.m.prior:
            self.op_set_prior(image=False)
        live = sorted(self.m.prior)
        return live[self.ri(0, len(live) - 1)]

    def pjob(self, p, where=None, dens=None, crop=0.0):
        """A fold's job on prior p.  crop: the share of jobs absorbed through a crop record (the window of the message's
        occupied cells and a vehicle's cell) where the message has such a window."""
        sp = self.raw_spec(dens)
        j = {"prior": p, "raw": sp, "msg": bool(self.ri(0, 1)), "at": self.place(p, sp["W"], sp["H"], where), "ori": list(self.m.prior[p]["origin"])}
        if self.rs.random_sample() < crop:
            j["crop"] = [self.ri(0, sp["W"] - 1), self.ri(0, sp["H"] - 1)]
            try:
                crops_of([j])
            except ValueError:
                del j["crop"]
        return j

    def fits(self, op):
        try:
            fold_of(self.m.prior_bytes(), op)
        except ValueError:
            return False
        return True

    def around(self, jobs, margin=None, open_side=True):
        """Keep windows around the jobs of each prior they name: [lo_xy, hi_xy] in world metres, None for an infinite bound."""
        keep = {}
        for p in sorted({j["prior"] for j in jobs}):
            mine = [j for j in jobs if j["prior"] == p]
            mg = self.ri(0, 6) if margin is None else margin
            lo = self.xy([min(j["at"][k] for j in mine) - mg for k in range(2)])
            hi = self.xy([max(j["at"][k] + (j["raw"]["W"], j["raw"]["H"])[k] for j in mine) + mg for k in range(2)])
            if open_side and self.rs.random_sample() < 0.4:
                (lo if self.ri(0, 1) else hi)[self.ri(0, 1)] = None
            keep[p] = [lo, hi]
        return keep

    def op_absorb(self, kind, jobs=None, **kw):
        """One absorb / grow / slide call that the library accepts (drawn again until the host reference accepts it)."""
        for _ in range(40):
            js = [self.pjob(self.a_prior(), crop=0.35) for _ in range(self.ri(1, 3))] if jobs is None else jobs
            op = {"op": kind, "jobs": js, "mode": kw.get("mode") or MODES[self.ri(0, 2)]}
            if kind != "absorb_prior":
                op["limit"] = kw.get("limit") or self.ri(48, 96)
            if kind == "absorb_prior_slide":
                op["keep"] = kw["keep"] if "keep" in kw else {p: w for p, w in self.around(js).items() if self.rs.random_sample() < 0.8}
                op["use"] = kw.get("use") or USES[int(self.rs.choice([0, 0, 1, 1, 2]))]
            if self.fits(op):
                return self.emit(op)
            if jobs is not None:
                raise AssertionError("the forced %s is refused: %r" % (kind, op))
            if kind != "absorb_prior" and len(self.m.prior) and self.rs.random_sample() < 0.3:
                self.op_set_prior(self.a_prior(), image=False)  # (a prior that has outgrown every limit is uploaded anew)
        raise AssertionError("no acceptable %s drawn" % kind)

    # -- world-frame and cropped jobs
    def job_ok(self, j, cropped=False, priors=None):
        priors = self.m.prior_bytes() if priors is None else priors
        try:
            wj = world_job(j)
            if cropped:
                grid, out, w, tail = crop_prepared(wj, priors)
                if grid is None:
                    return True
            else:
                grid, out, w = world_prepared(wj, named_prior(priors, wj))
        except (IndexError, ValueError):
            return False
        return all(0 <= out[a][b] < grid.shape[b] for a in (0, 1) for b in (0, 1)) and max(grid.shape) <= 160

    def wjob(self, slot, p="draw", where=None, ori=None, cropped=False, dens=None):
        """A world or cropped job whose preparation succeeds on the priors as they are.  ori: the origin it carries (None:
        the one the model holds now)."""
        for _ in range(80):
            pp = (self.a_prior() if self.rs.random_sample() < 0.8 else None) if p == "draw" else p
            sp = self.raw_spec(float(self.rs.choice([0.0, 0.05, 0.2])) if dens is None else dens)
            W, H = sp["W"], sp["H"]
            j = {"slot": slot, "raw": sp, "msg": bool(self.ri(0, 1)), "start": [self.ri(0, W - 1), self.ri(0, H - 1)],
                 "goal": [self.ri(0, W - 1), self.ri(0, H - 1)], "ifa": self.ri(0, 2), "variant": self.ri(0, 1), "prior": pp,
                 "at": self.place(pp, W, H, where) if pp is not None else [self.ri(-20, 20), self.ri(-20, 20)],
                 "ori": None if pp is None else list(self.m.prior[pp]["origin"]) if ori is None else list(ori)}
            if cropped:
                r = self.rs.random_sample()
                if r < 0.12:
                    j["start"][self.ri(0, 1)] = -2  # (the vehicle left of or below the message: the job is refused on its own)
                elif r < 0.22:
                    j["raw"] = dict(sp, p=0.0, set=[])  # (no occupied cell: not planned)
            if self.job_ok(j, cropped):
                return j
        raise AssertionError("no preparable world job drawn")

    def op_world_jobs(self, kind, slots=None, jobs=None):
        cropped = kind.endswith("_cropped")
        if jobs is None:
            slots = sorted(self.rs.choice(NSLOTS, self.ri(1, 3), replace=False).tolist()) if slots is None else slots
            jobs = []
            for s in slots:
                old, j = self.slot_raw.get(s), None
                r = self.rs.random_sample()
                if kind.startswith("refresh") and old is not None and self.cropped.get(s) == cropped and r < 0.7 and (old["prior"] is None or old["prior"] in self.m.prior):
                    # (the slot's last job again, as it was or with a few cells changed, at the prior's present origin)
                    j = dict(old, ori=None if old["prior"] is None else list(self.m.prior[old["prior"]]["origin"]))
                    if r < 0.25:
                        j["raw"] = self.changed(old["raw"], self.ri(1, 3))
                    j = j if self.job_ok(j, cropped) else None
                jobs.append(j or self.wjob(s, cropped=cropped))
        for j in jobs:
            self.slot_raw[j["slot"]] = j
            self.cropped[j["slot"]] = cropped
        return self.emit({"op": kind, "jobs": jobs})

    def slots_live(self, n=2):
        while len(self.m.slots) < n:
            self.op_world_jobs("prepare_slots_world", slots=[s for s in range(NSLOTS) if s not in self.m.slots][:2])

    def replan_naming(self, slot):
        """A new replan_slots whose first query runs on `slot`."""
        live = sorted(self.m.slots)
        ids = [slot] + [live[self.ri(0, len(live) - 1)] for _ in range(self.ri(1, 5))]
        s, g = self.queries([self.m.slots[i] for i in ids], len(ids))
        self.last_replan = {"ids": ids, "s": s, "g": g, "hchoice": self.ri(1, 2), "mpl": 400}
        return self.emit(dict(self.last_replan, op="replan_slots"))

    def op_check_paths(self, shift="draw"):
        L = self.m.last
        if L is None or L["kind"] != "slots" or L["nq"] < 1:
            self.slots_live()
            self.op_plan_batch_slots()
        if shift == "draw":
            shift = None if self.rs.random_sample() < 0.5 else [self.ri(-2, 2), self.ri(-2, 2)]
        return self.emit({"op": "check_paths_slots", "shift": shift})

    # -- refusals
    def op_refusal(self, which):
        self.count["refused: " + which] = self.count.get("refused: " + which, 0) + 1
        p = self.a_prior()
        kind = str(self.rs.choice(["absorb_prior", "absorb_prior_grow", "absorb_prior_slide"]))
        extra = {"limit": 96, "keep": {}, "use": "none"}
        if which == "prior_not_set":
            unset = [q for q in PRIORS if q not in self.m.prior] + [UNSET_PRIOR]
            jobs = [self.pjob(p), dict(self.pjob(p), prior=unset[0])]
            return self.emit(dict(extra, op=kind, jobs=jobs[self.ri(0, 1):], mode=MODES[self.ri(0, 2)]))
        if which == "grow_past_limit":  # (no window: a side above the limit refuses the call)
            j = self.pjob(p)
            k = self.ri(0, 1)
            j["at"][k] = self.cell_xy(self.m.prior[p]["origin"])[k] + self.m.prior[p]["bytes"].shape[k] + self.ri(60, 90)
            kind = str(self.rs.choice(["absorb_prior_grow", "absorb_prior_slide"]))
            return self.emit(dict(extra, op=kind, jobs=[self.pjob(p, ("in", "in")), j], mode=MODES[self.ri(0, 2)], limit=self.ri(48, 96)))
        if which == "slide_empty_window":
            j = self.pjob(p, ("in", "in"))
            far = self.xy([j["at"][0] - 400, j["at"][1]])
            return self.emit({"op": "absorb_prior_slide", "jobs": [j], "mode": MODES[self.ri(0, 2)], "limit": 96,
                              "keep": {p: [[far[0], None], [far[0] + 2 * R, None]]}, "use": "always"})
        if which == "window_unnamed_prior":
            j = self.pjob(p, ("in", "in"))
            other = [q for q in PRIORS if q != p][self.ri(0, 1)]
            return self.emit({"op": "absorb_prior_slide", "jobs": [j], "mode": MODES[self.ri(0, 2)], "limit": 96,
                              "keep": {**self.around([j], open_side=False), other: [[None, None], [None, None]]}, "use": "always"})
        if which == "unequal_ori_pre":
            a, b = self.pjob(p, ("in", "in")), self.pjob(p, ("in", "in"))
            b["ori"] = [b["ori"][0] + R, b["ori"][1]]
            kind = str(self.rs.choice(["absorb_prior_grow", "absorb_prior_slide"]))
            return self.emit(dict(extra, op=kind, jobs=[a, b], mode=MODES[self.ri(0, 2)]))
        # a world job that names a prior after its clear_prior_map
        if not self.cleared:
            self.emit({"op": "clear_prior_map", "prior": p})
            self.cleared.add(p)
        q = sorted(self.cleared)[0]
        self.slots_live()
        sp = self.raw_spec(0.05)
        j = {"slot": self.ri(0, NSLOTS - 1), "raw": sp, "msg": False, "start": [0, 0], "goal": [sp["W"] - 1, sp["H"] - 1], "ifa": 1, "variant": 0, "prior": q,
             "at": [self.ri(-8, 8), self.ri(-8, 8)], "ori": self.xy([0, 0])}
        return self.emit({"op": str(self.rs.choice(["prepare_slots_world", "refresh_slots_world", "prepare_slots_cropped"])), "jobs": [j]})

    # -- the orders every sequence holds
    def forced(self):
        for p in PRIORS:
            self.op_set_prior(p, image=(p == 15))
        self.op_world_jobs("prepare_slots_world", slots=[0, 1])
        self.op_world_jobs("prepare_slots_world", slots=[2, 3])
        self.op_replan_slots(fresh=True)

    def changing_absorb(self, p, judge):
        """An absorb_prior record on prior p (cells inside it, mostly occupied) for which judge(the priors afterwards) holds."""
        for _ in range(60):
            op = {"op": "absorb_prior", "jobs": [self.pjob(p, ("in", "in"), dens=float(self.rs.choice([0.5, 0.9])))], "mode": MODES[self.ri(0, 1)]}
            after, _, ret = fold_of(self.m.prior_bytes(), op)
            if ret[1][p] > 0 and judge({**self.m.prior_bytes(), **after}):
                return op
        raise AssertionError("no absorb drawn that changes what it has to")

    def seq_prior_changes_under_a_slot(self, tiles=False):
        """A slot prepared from a prior, its queries stored, the prior rewritten under it by an absorb: the replan hands
        every path back (no slot was touched); the refresh with the SAME job is not kept; the replan then searches."""
        if tiles != bool(self.m.mode):
            self.emit({"op": "set_slot_reuse", "mode": "tiles" if tiles else "generation"})
        p = PRIORS[self.ri(0, 2)]
        self.op_set_prior(p, image=False, big=True)  # (larger than every raw: some of its cells lie on the canvas beside the raw)
        slot = self.ri(0, NSLOTS - 1)
        j = self.wjob(slot, p, ("in", "in"))
        self.op_world_jobs("prepare_slots_world", jobs=[j])
        self.replan_naming(slot)

        def differs(priors):
            if not self.job_ok(j, priors=priors):
                return False
            grid = world_prepared(world_job(j), priors[p])[0]
            return grid.shape != self.m.slots[slot].shape or not np.array_equal(grid, self.m.slots[slot])
        self.emit(self.changing_absorb(p, differs))
        self.op_replan_slots(fresh=False, move=0.0)
        self.op_world_jobs("refresh_slots_world", jobs=[dict(j)])
        self.op_replan_slots(fresh=False, move=0.0)

    def seq_absorb_elsewhere(self):
        """An absorb that changes another prior only: the replan hands every path back, the refresh with the same job is kept."""
        p0 = self.a_prior()
        p1 = [q for q in PRIORS if q != p0][self.ri(0, 1)]
        if p1 not in self.m.prior:
            self.op_set_prior(p1, image=False)
        slot = self.ri(0, NSLOTS - 1)
        j = self.wjob(slot, p0)
        self.op_world_jobs(str(self.rs.choice(["prepare_slots_world", "refresh_slots_world"])), jobs=[j])
        self.replan_naming(slot)
        self.emit(self.changing_absorb(p1, lambda priors: True))
        self.op_replan_slots(fresh=False, move=0.0)
        self.op_world_jobs("refresh_slots_world", jobs=[dict(j)])
        self.op_replan_slots(fresh=False, move=0.0)

    def seq_grow_moves_origin(self):
        """A grow that moves a prior's origin between two equal replans; jobs with the new and with the upload's origin;
        then the prior uploaded again: the moved origin is forgotten."""
        p = PRIORS[self.ri(0, 2)]
        self.op_set_prior(p, image=False)
        self.slots_live()
        self.op_replan_slots(fresh=True)
        k = self.ri(0, 1)
        where = [None, None]
        where[k], where[1 - k] = str(self.rs.choice(["lo", "out_lo"])), str(self.rs.choice(["in", "hi", "lo"]))
        self.op_absorb("absorb_prior_grow", [self.pjob(p, where), self.pjob(p)], limit=96)
        self.op_replan_slots(fresh=False, move=0.0)
        self.emit({"op": "prior_origin", "prior": p})
        slot = self.ri(0, NSLOTS - 1)
        try:  # (legal for prepare_slots_world: merge_host's result at that origin, where the two rectangles fit its canvas)
            self.op_world_jobs("prepare_slots_world", jobs=[self.wjob(slot, p, ori=self.m.prior[p]["upload"])])
        except AssertionError:
            pass
        self.op_world_jobs("prepare_slots_world", jobs=[self.wjob((slot + 1) % NSLOTS, p)])
        self.op_set_prior(p, image=bool(self.ri(0, 1)))
        self.emit({"op": "prior_origin", "prior": p})
        self.emit({"op": "get_prior_map", "prior": p})

    def seq_refused_grow_between_two(self):
        p = PRIORS[self.ri(0, 2)]
        self.op_set_prior(p, image=False)
        self.op_absorb("absorb_prior_grow", [self.pjob(p, ("hi", "in"))], limit=96)
        self.op_refusal("grow_past_limit")
        self.op_absorb("absorb_prior_grow", [self.pjob(p, ("in", "lo"))], limit=96)

    def seq_slides(self):
        """A slide that always cuts cells off the low side; an over_limit slide within the limit (not trimmed); one past
        it (trimmed to the window around its job); a slot prepared from the prior that slid."""
        p = PRIORS[self.ri(0, 2)]
        self.op_set_prior(p, image=False, big=True)
        c = self.cell_xy(self.m.prior[p]["origin"])
        k = self.ri(0, 1)
        lo = [None, None]
        lo[k] = self.xy([c[0] + self.ri(1, 4), c[1] + self.ri(1, 4)])[k]
        self.op_absorb("absorb_prior_slide", [self.pjob(p, ("in", "in"))], limit=96, keep={p: [lo, [None, None]]}, use="always")
        js = [self.pjob(p, ("in", "in")), self.pjob(p, ("in", "in"))]
        self.op_absorb("absorb_prior_slide", js, limit=96, keep=self.around(js), use="over_limit")
        far = self.pjob(p)
        c, ext = self.cell_xy(self.m.prior[p]["origin"]), self.m.prior[p]["bytes"].shape
        far["at"] = [c[0] + ext[0] + self.ri(30, 50), c[1] + self.ri(-3, 3)]
        self.op_absorb("absorb_prior_slide", [far], limit=48, keep=self.around([far], margin=self.ri(1, 8), open_side=False), use="over_limit")
        self.emit({"op": "prior_origin", "prior": p})
        self.op_world_jobs("prepare_slots_world", jobs=[self.wjob(self.ri(0, NSLOTS - 1), p)])

    def seq_slide_grow_absorb(self):
        """Slide, then grow, then absorb on ONE prior, each at the origin the call before left, the other priors untouched
        in between; then a slot prepared from it."""
        p = self.a_prior()
        if max(self.m.prior[p]["bytes"].shape) > 40:
            self.op_set_prior(p, image=False)
        js = [self.pjob(p, crop=0.5), self.pjob(p)]
        self.op_absorb("absorb_prior_slide", js, limit=96, keep=self.around(js, open_side=False), use="always")
        self.op_absorb("absorb_prior_grow", [self.pjob(p, (str(self.rs.choice(["lo", "hi"])), "in"))], limit=96)
        self.op_absorb("absorb_prior", [self.pjob(p, crop=0.5), self.pjob(p, ("in", "in"), dens=0.5)])
        kind = str(self.rs.choice(["prepare_slots_world", "prepare_slots_cropped"]))
        self.op_world_jobs(kind, jobs=[self.wjob(self.ri(0, NSLOTS - 1), p, cropped=kind.endswith("_cropped"))])

    def seq_cleared_prior(self):
        p = self.a_prior()
        self.emit({"op": "clear_prior_map", "prior": p})
        self.cleared.add(p)
        self.op_refusal("world_cleared_prior")
        self.emit({"op": "prior_origin", "prior": p})
        self.op_set_prior(p)

    def seq_check_paths(self):
        """The paths of a slots batch judged on the slots as they are now: as the batch left them, with one of them
        rewritten (denser), moved by a small and by a large shift; the resident paths are still the batch's afterwards."""
        self.slots_live(3)
        self.op_plan_batch_slots() if self.ri(0, 1) else self.op_replan_slots(fresh=True)
        self.op_check_paths(None)
        ids = self.m.last["ids"]
        self.op_world_jobs("prepare_slots_world", jobs=[self.wjob(ids[self.ri(0, len(ids) - 1)], dens=float(self.rs.choice([0.35, 0.5])))])
        self.op_check_paths(None)
        self.op_check_paths([self.ri(-1, 1), self.ri(1, 2)])
        self.op_check_paths([self.ri(150, 300), 0])
        self.op_wp("select_slots_batch")

    def step(self):
        r = self.rs.random_sample()
        self.slots_live()
        if r < 0.05:
            return self.op_refusal(WORLD_REFUSALS[self.ri(0, len(WORLD_REFUSALS) - 1)])
        if r < 0.11:
            return self.op_set_prior()
        if r < 0.13:
            if len(self.m.prior) < 2:
                return self.op_set_prior()
            p = self.a_prior()
            self.cleared.add(p)
            return self.emit({"op": "clear_prior_map", "prior": p})
        if r < 0.21:
            return self.op_absorb("absorb_prior")
        if r < 0.28:
            return self.op_absorb("absorb_prior_grow")
        if r < 0.35:
            return self.op_absorb("absorb_prior_slide")
        if r < 0.39:
            return self.emit({"op": str(self.rs.choice(["get_prior_map", "prior_origin"])), "prior": self.a_prior()})
        if r < 0.48:
            return self.op_world_jobs(str(self.rs.choice(["prepare_slots_cropped", "refresh_slots_cropped"])))
        if r < 0.50:
            return self.op_check_paths()
        if r < 0.60:
            return self.op_world_jobs(str(self.rs.choice(["prepare_slots_world", "refresh_slots_world"])))
        if r < 0.64:
            return self.op_plan_batch_slots()
        if r < 0.76:
            return self.op_replan_slots()
        if r < 0.79:
            return self.emit({"op": "set_slot_reuse", "mode": str(self.rs.choice(["generation", "tiles"]))})
        if r < 0.85:
            return self.op_readback(str(self.rs.choice(["publish_slots", "get_grid_slot"])))
        if r < 0.93:
            return self.op_wp(str(self.rs.choice(["select_slots_batch", "tick_outputs_slots"])))
        return self.op_replan_slots(fresh=False if getattr(self, "last_replan", None) is not None else None)


def _generate_world(seed, n_steps, profile):
    g = _WorldGen(seed, profile)
    g.forced()
    seqs = [lambda: g.seq_prior_changes_under_a_slot(False), lambda: g.seq_prior_changes_under_a_slot(True), g.seq_absorb_elsewhere, g.seq_slide_grow_absorb,
            g.seq_grow_moves_origin, g.seq_refused_grow_between_two, g.seq_slides, g.seq_cleared_prior, g.seq_check_paths, g.seq_check_paths]
    order = g.rs.permutation(len(seqs)).tolist()
    marks = sorted(g.rs.choice(np.arange(6, max(n_steps - 10, 20)), len(seqs), replace=False).tolist())
    which = 0
    while len(g.ops) < n_steps or which < len(seqs):
        if which < len(seqs) and (len(g.ops) >= marks[which] or len(g.ops) >= n_steps):
            seqs[order[which]]()
            which += 1
            continue
        g.step()
    # the closing round: every refusal once, every kind three times, whatever was drawn
    closing = {"set_prior_map": lambda: g.op_set_prior(image=False), "set_prior_image": lambda: g.op_set_prior(image=True),
               "clear_prior_map": lambda: (g.cleared.add(g.a_prior()), g.emit({"op": "clear_prior_map", "prior": sorted(g.cleared & set(g.m.prior))[0]})),
               "get_prior_map": lambda: g.emit({"op": "get_prior_map", "prior": g.a_prior()}), "prior_origin": lambda: g.emit({"op": "prior_origin", "prior": g.a_prior()}),
               "absorb_prior": lambda: g.op_absorb("absorb_prior"), "absorb_prior_grow": lambda: g.op_absorb("absorb_prior_grow"),
               "absorb_prior_slide": lambda: g.op_absorb("absorb_prior_slide"), "prepare_slots_cropped": lambda: g.op_world_jobs("prepare_slots_cropped"),
               "refresh_slots_cropped": lambda: g.op_world_jobs("refresh_slots_cropped"), "check_paths_slots": g.op_check_paths,
               "prepare_slots_world": lambda: g.op_world_jobs("prepare_slots_world"), "refresh_slots_world": lambda: g.op_world_jobs("refresh_slots_world"),
               "plan_batch_slots": lambda: (g.slots_live(), g.op_plan_batch_slots()), "replan_slots": lambda: (g.slots_live(), g.op_replan_slots()),
               "set_slot_reuse": lambda: g.emit({"op": "set_slot_reuse", "mode": ["generation", "tiles"][g.ri(0, 1)]}),
               "publish_slots": lambda: (g.slots_live(), g.op_readback("publish_slots")), "get_grid_slot": lambda: (g.slots_live(), g.op_readback("get_grid_slot")),
               "select_slots_batch": lambda: (g.slots_live(), g.op_wp("select_slots_batch")), "tick_outputs_slots": lambda: (g.slots_live(), g.op_wp("tick_outputs_slots"))}
    for which in WORLD_REFUSALS:
        if g.count.get("refused: " + which, 0) < 1:
            g.op_refusal(which)
    for kind in kinds_of(profile):
        for _ in range(50):
            if g.count.get(kind, 0) >= 3:
                break
            closing[kind]()
    return g.ops


def generate(seed, n_steps, profile):
    """-> the op records of sequence `seed` of `profile`: a function of its arguments alone."""
    if profile in WORLD_PROFILES:
        return _generate_world(seed, n_steps, profile)
    g = _Gen(seed, profile)
    g.forced()
    if profile == "tiles":
        g.emit({"op": "set_slot_reuse", "mode": "tiles"})
    order = g.rs.permutation(12).tolist()
    marks = sorted(g.rs.choice(np.arange(6, max(n_steps - 10, 20)), 12, replace=False).tolist())
    which = 0
    while len(g.ops) < n_steps or which < 12:
        if which < 12 and (len(g.ops) >= marks[which] or len(g.ops) >= n_steps):
            g.forced_later(order[which])
            which += 1
            continue
        g.step()
    # the closing round: every kind at least three times, whatever was drawn
    closing = {"set_grid": lambda: g.op_grid("set_grid"), "set_grid_occ": lambda: g.op_grid("set_grid_occ"),
               "set_grid_image": lambda: g.op_grid("set_grid_image"), "prepare_grid": lambda: g.op_grid("prepare_grid"),
               "prepare_occupancy_msg": lambda: g.op_grid("prepare_occupancy_msg"), "refresh_grid": g.op_refresh, "update_cells": g.op_update,
               "get_grid": lambda: g.op_readback("get_grid"), "publish_map": lambda: g.op_readback("publish_map"),
               "snapshot_image": lambda: g.op_readback("snapshot_image"), "plan_batch": g.op_plan_batch, "plan_one": lambda: g.op_plan_one("plan_one"),
               "plan": lambda: g.op_plan_one("plan"), "set_queries": g.op_set_queries, "replan_frame": g.op_replan_frame,
               "replan_frame_raw": g.op_replan_frame_raw, "set_grid_slot": lambda: g.op_grid_slots("set_grid_slot"), "clear_grid_slot": g.op_clear_slot,
               "set_grid_slots": lambda: g.op_grid_slots("set_grid_slots"), "refresh_grid_slots": lambda: g.op_grid_slots("refresh_grid_slots"),
               "prepare_slots": lambda: g.op_slot_jobs("prepare_slots"), "refresh_slots": lambda: g.op_slot_jobs("refresh_slots"),
               "prepare_slots_world": lambda: g.op_slot_jobs("prepare_slots_world"), "refresh_slots_world": lambda: g.op_slot_jobs("refresh_slots_world"),
               "plan_batch_slots": g.op_plan_batch_slots, "replan_slots": g.op_replan_slots,
               "set_slot_reuse": lambda: g.emit({"op": "set_slot_reuse", "mode": ["generation", "tiles"][g.ri(0, 1)]}),
               "publish_slots": lambda: g.op_readback("publish_slots"), "get_grid_slot": lambda: g.op_readback("get_grid_slot"),
               "select_st_batch": lambda: g.op_wp("select_st_batch"), "select_ccst_batch": lambda: g.op_wp("select_ccst_batch"),
               "select_slots_batch": lambda: g.op_wp("select_slots_batch"), "tick_outputs_slots": lambda: g.op_wp("tick_outputs_slots"),
               "fresh_set_queries": lambda: g.emit({"op": "fresh_set_queries", "s": [[0, 0]], "g": [[1, 1]], "hchoice": 2, "mpl": 400})}
    for which in REFUSALS:
        if g.count.get("refused: " + which, 0) < 1:
            g.op_refusal(which)
    for kind in kinds_of(profile):
        for _ in range(50):
            if g.count.get(kind, 0) >= 3:
                break
            (g.op_shim if kind.startswith("jps1") else closing[kind])()
    return g.ops


def kinds_of(profile):
    """The op kinds a sequence of `profile` holds at least three times each."""
    if profile in WORLD_PROFILES:
        return list(WORLD_KINDS + WORLD_OLD_KINDS)
    out = [k for k in KINDS if k != "set_slot_reuse" or profile == "tiles"]
    return out + (["jps1_method", "jps1_method_many"] if profile == "shim" else [])


# ------------------------------------------------------------------ one op on a planner
class _Waypoints(object):
    """The waypoint batch calls of a Planner (module functions that take the planner)."""

    def __init__(self, planner):
        from fuxi_planner_amd import waypoints
        self.p, self.w = planner, waypoints

    def __getattr__(self, name):
        fn = getattr(self.w, name)
        return lambda *a, **kw: fn(self.p, *a, **kw)


def wp_inputs(op, nq):
    """The per-query arguments of a waypoint op, from its seed: positions and goals around the origin, previous waypoints
    for half of the queries, a goal equal to home for one (its z is a NaN or 1)."""
    rs = np.random.RandomState(op["seed"])
    pos = np.round(rs.uniform(-2, 30, (nq, 3)) * 4) / 4
    goal = np.round(rs.uniform(-2, 30, (nq, 3)) * 4) / 4
    home = np.round(rs.uniform(-2, 30, (nq, 2)) * 4) / 4
    if nq:
        home[0] = goal[0, :2]
    eo = (rs.random_sample(nq) < 0.3).astype(np.int32) if op["end_occu"] else None
    pw = pd = None
    if op["prev"]:
        pw, pd = np.round(rs.uniform(-2, 30, (nq, 3)) * 4) / 4, rs.choice([0, 2, 3], nq).astype(np.int32)
    ms = rs.randint(0, 5, (nq, 2)).astype(np.int32)
    return pos, goal, home, eo, pw, pd, ms


def call_wp(wp, op, nq, paths, ids=None):
    """A waypoint op with the resident paths (paths None or (offsets, None)) or with explicit ones."""
    pos, goal, home, eo, pw, pd, ms = wp_inputs(op, nq)
    k = op["op"]
    if k == "select_st_batch":
        return wp.select_st_batch(nq, ms, R, (-2.0, 1.0), pos, goal, eo, pw, pd, paths=paths)
    if k == "select_ccst_batch":
        return wp.select_ccst_batch(nq, R, (-2.0, 1.0), pos, goal, eo, paths=paths)
    rule = (op["rule"] + [0] * nq)[:nq]
    if paths is not None and paths[1] is None and op["form"] == "none":  # (the tick outputs take the offsets on their own then)
        if k == "select_slots_batch":
            return wp.select_slots_batch(rule, ms, R, (-2.0, 1.0), pos, goal, eo, pw, pd, grid_ids=ids, paths=None)
        return wp.tick_outputs_slots(rule, ms, R, (-2.0, 1.0), pos, goal, home, eo, pw, pd, grid_ids=ids, paths=None, offsets=paths[0])
    if k == "select_slots_batch":
        return wp.select_slots_batch(rule, ms, R, (-2.0, 1.0), pos, goal, eo, pw, pd, grid_ids=ids, paths=paths)
    return wp.tick_outputs_slots(rule, ms, R, (-2.0, 1.0), pos, goal, home, eo, pw, pd, grid_ids=ids, paths=paths)


def execute(p, op, wp, fresh):
    """-> what the call returned."""
    k = op["op"]
    if k in ("set_grid", "jps1_method"):
        mat = grid_of(op["g"]).astype(np.float64)
        if k == "set_grid":
            return p.set_grid(mat)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            r = p.jps1_method(mat, tuple(op["s"]), tuple(op["g2"]), op["hchoice"]) if hasattr(p, "jps1_method") else _jps1().method(
                mat, tuple(op["s"]), tuple(op["g2"]), op["hchoice"])
        return r, buf.getvalue()
    if k == "jps1_method_many":
        calls = [(grid_of(c[0]).astype(np.float64), tuple(c[1]), tuple(c[2])) for c in op["calls"]]
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            r = p.jps1_method_many(calls, op["hchoice"]) if hasattr(p, "jps1_method_many") else _jps1().method_many(calls, op["hchoice"])
        return r, buf.getvalue()
    if k == "set_grid_occ":
        return p.set_grid_occ(grid_of(op["g"]))
    if k == "set_grid_image":
        return p.set_grid_image(gray_of(op["gray"]))
    if k in ("prepare_grid", "refresh_grid"):
        out = getattr(p, k)(grid_of(op["raw"]), tuple(op["start"]), tuple(op["goal"]), op["ifa"], op["variant"])
        return (out, p.last_refresh_cells()) if k == "refresh_grid" else out
    if k == "prepare_occupancy_msg":
        return p.prepare_occupancy_msg(msg_of(op["raw"]), op["raw"]["W"], op["raw"]["H"], tuple(op["start"]), tuple(op["goal"]), op["ifa"], op["variant"])
    if k == "update_cells":
        return p.update_cells(np.array(op["xy"], np.int32).reshape(-1, 2), np.array(op["val"], np.uint8), rebuild=op["rebuild"])
    if k == "get_grid":
        return [p.get_grid(c) for c in range(len(p.devices))]
    if k == "publish_map":
        return p.publish_map()
    if k == "snapshot_image":
        return p.snapshot_image(op["channels"])
    if k == "plan_batch":
        return p.plan_batch(np.array(op["s"], np.int32).reshape(-1, 2), np.array(op["g"], np.int32).reshape(-1, 2), op["hchoice"], op["mpl"])
    if k == "plan_one":
        st, cost, cells = p.plan_one(tuple(op["s"]), tuple(op["g"]), op["hchoice"])
        return st, cost, np.array(cells).copy()
    if k == "plan":
        r = p.plan(tuple(op["s"]), tuple(op["g"]), op["hchoice"])
        return r, p.last_cost
    if k in ("set_queries", "fresh_set_queries"):
        if k == "fresh_set_queries":
            q = fresh()
            try:
                return q.set_queries(op["s"], op["g"], op["hchoice"], op["mpl"])
            finally:
                q.close()
        return p.set_queries(op["s"], op["g"], op["hchoice"], op["mpl"])
    if k == "replan_frame":
        out = p.replan_frame(np.array(op["xy"], np.int32).reshape(-1, 2), np.array(op["val"], np.uint8))
        return out, p.timing()["reused"]
    if k == "replan_frame_raw":
        out = p.replan_frame_raw(grid_of(op["raw"]), tuple(op["start"]), tuple(op["goal"]), op["ifa"], op["variant"])
        return out, p.timing()["reused"], p.last_refresh_cells()
    if k == "set_grid_slot":
        return p.set_grid_slot(op["slot"], grid_of(op["g"]).astype(np.float64))
    if k == "clear_grid_slot":
        return p.clear_grid_slot(op["slot"])
    if k in ("set_grid_slots", "refresh_grid_slots"):
        return getattr(p, k)([(s, grid_of(g).astype(np.float64)) for s, g in op["jobs"]])
    if k in ("prepare_slots", "refresh_slots"):
        jobs = [slot_job(j) for j in op["jobs"]]
        jobs = [(j[0], (msg_of(r["raw"]), r["raw"]["W"], r["raw"]["H"])) + j[2:] if r["raw"]["seed"] % 2 else j for j, r in zip(jobs, op["jobs"])]
        return getattr(p, k)(jobs)
    if k in ("prepare_slots_world", "refresh_slots_world", "prepare_slots_cropped", "refresh_slots_cropped"):
        return getattr(p, k)([world_job(j) for j in op["jobs"]])
    if k == "set_prior_map":
        return p.set_prior_map(op["prior"], grid_of(op["g"]))
    if k == "set_prior_image":
        return p.set_prior_image(op["prior"], gray_of(op["gray"]))
    if k in ("clear_prior_map", "get_prior_map", "prior_origin"):
        return getattr(p, k)(op["prior"])
    if k == "absorb_prior":
        return p.absorb_prior([prior_job(j) for j in op["jobs"]], op["mode"], crops_of(op["jobs"]))
    if k == "absorb_prior_grow":
        return p.absorb_prior_grow([prior_job(j) for j in op["jobs"]], op["mode"], crops_of(op["jobs"]), op["limit"])
    if k == "absorb_prior_slide":
        return p.absorb_prior_slide([prior_job(j) for j in op["jobs"]], op["mode"], crops_of(op["jobs"]), op["limit"], keep_of(op), op["use"])
    if k in ("plan_batch_slots", "replan_slots"):
        out = getattr(p, k)(op["ids"], op["s"], op["g"], op["hchoice"], op["mpl"])
        return (out, p.timing()["reused"]) if k == "replan_slots" else out
    if k == "set_slot_reuse":
        return p.set_slot_reuse(op["mode"])
    if k == "publish_slots":
        return p.publish_slots(op["slots"], msg=op["msg"], image_channels=op["channels"])
    if k == "get_grid_slot":
        return p.get_grid_slot(op["slot"])
    raise ValueError("unknown op %r" % (k,))


def _jps1():
    from fuxi_planner_amd import jps1
    return jps1


# ------------------------------------------------------------------ run
class Mismatch(AssertionError):
    """assertion: a compared output or flag differed; False: a call of a check raised something else."""
    assertion = True


def check_maps(dev, occ, what, exact=True, ever_free=None):
    msg = dm.first_difference(dev, dm.reference_maps(truth(occ)))
    assert msg is None, "%s: %s" % (what, msg)
    msg = dm.component_problem(dev["comp"], truth(occ), exact=exact, ever_free=ever_free)
    assert msg is None, "%s: components: %s" % (what, msg)


def run(planner, ops, oracle, fresh=None, contexts=1, seed=None, model=None):
    """Apply every op to `planner` and to a new Model; compare what the host references say.  fresh: () -> another handle
    (for the refusal on a handle without a grid).  contexts: those of the handle.  -> the model."""
    m = Model(contexts) if model is None else model
    wp = planner if hasattr(planner, "select_st_batch") else _Waypoints(planner)
    for i, op in enumerate(ops):
        try:
            _step(planner, wp, m, op, i, oracle, fresh, contexts)
        except Exception as ex:  # noqa: BLE001 (an assertion, or whatever a check's own call raised)
            asserted = isinstance(ex, AssertionError)
            if not asserted:
                ex = "%s: %s" % (type(ex).__name__, ex)
            mm = Mismatch("seed %r, step %d, op %s: %s\n\nreplay: run(planner, ops, oracle) with\nops = %r" % (seed, i, op["op"], ex, ops[:i + 1]))
            mm.assertion = asserted
            raise mm
    return m


def _csr_equal(got, exp, what):
    off, cells, cost, status = got[:4]
    eoff, ecells, ecost, estatus = exp
    assert np.array_equal(np.asarray(status), estatus), "%s: status %r, the oracle's %r" % (what, np.asarray(status).tolist(), estatus.tolist())
    assert np.asarray(cost, np.float64).tobytes() == ecost.tobytes(), "%s: float64 costs differ from the oracle's: %r, %r" % (what, cost, ecost)
    assert np.array_equal(np.asarray(off), eoff), "%s: offsets %r, expected %r" % (what, np.asarray(off).tolist(), eoff.tolist())
    assert np.array_equal(np.asarray(cells).reshape(-1, 2), ecells), "%s: cells differ from the oracle's" % what


def _step(p, wp, m, op, i, oracle, fresh, contexts):
    k = op["op"]
    before_last = m.last
    try:
        e = expect(m, op, oracle)
        refused = None
    except Refused as r:
        e, refused = None, r
    try:
        if k in ("select_st_batch", "select_ccst_batch", "select_slots_batch", "tick_outputs_slots"):
            slots_form = k in ("select_slots_batch", "tick_outputs_slots")
            got = None if refused is None else call_wp(wp, op, op["nq"], (np.zeros(op["nq"] + 1, np.int64), None) if slots_form else None)
        elif k == "check_paths_slots":  # (the explicit paths of the last slots batch: the generator draws the op only after one)
            got = p.check_paths_slots(before_last["ids"], before_last["off"], before_last["cells"], op["shift"])
        else:
            got = execute(p, op, wp, fresh)
        raised = None
    except Exception as ex:  # noqa: BLE001 (whatever the call raises is compared with what it must raise)
        got, raised = None, ex
    if k == "fresh_set_queries":
        assert raised is not None and type(raised).__name__ == "FxjpsError" and raised.code == E_NOGRID, "set_queries on a handle without a grid: %r" % (raised,)
        return
    if refused is not None:
        assert raised is not None, "the call must be refused (%s), it returned" % (refused.kind,)
        assert type(raised).__name__ == refused.kind and (refused.code is None or getattr(raised, "code", None) == refused.code), \
            "refused with %r, expected %s %r" % (raised, refused.kind, refused.code)
        assert m.last is before_last
        _check_priors(p, m, op, i, True)
        return
    if k in ("plan", "jps1_method") and e["csr"][3][0] < 0:
        want = IndexError if e["csr"][3][0] == Q_BAD_START else RuntimeError
        assert isinstance(raised, want), "status %d must raise %s, got %r" % (e["csr"][3][0], want.__name__, raised)
        m.last["off"], m.last["cells"] = e["csr"][0], e["csr"][1]
        return
    if raised is not None:
        raise AssertionError("the call raised %s: %s" % (type(raised).__name__, raised))

    wrote_grid = wrote_slots = ()
    if k in ("set_grid", "set_grid_occ", "set_grid_image") or (k == "update_cells" and op["rebuild"]):
        wrote_grid = (True,)  # (a deferred update is left pending for the next op: reading the maps would rebuild them)
    elif k in ("prepare_grid", "prepare_occupancy_msg"):
        assert same(got, e["out"]), "outputs %r, gridprep's %r" % (got, e["out"])
        wrote_grid = (True,)
    elif k == "refresh_grid":
        out, cells = got
        _refresh_flags(out[:5], out[5], out[6], cells, e)
        wrote_grid = (True,)
    elif k == "get_grid":
        for c, g in enumerate(got):
            assert same(g, m.grid), "context %d: the resident grid's bytes differ from the model's" % c
    elif k == "publish_map":
        assert same(got, adapters.publish_map(truth(m.grid))), "publish_map differs from the adapter's"
    elif k == "snapshot_image":
        assert same(got, adapters.snapshot_image(truth(m.grid), op["channels"])), "snapshot_image differs from the adapter's"
    elif k == "plan_batch":
        _csr_equal(got, e["csr"], k)
    elif k == "plan_one":
        st, cost, cells = got
        _csr_equal((e["csr"][0], cells, [cost], [st]), e["csr"], k)
    elif k in ("plan", "jps1_method"):
        off, cells, cost, status = e["csr"]
        path = [(int(x), int(y)) for x, y in cells]
        if k == "plan":
            assert got[0] == path, "plan: %r, the oracle's %r" % (got[0], path)
            assert np.float64(got[1]).tobytes() == cost[:1].tobytes()
        else:
            (r, secs), printed = got
            if status[0] == 0:
                assert type(r) is int and r == 0 and printed == "", (r, printed)  # (the callers test `path1[0] is 0`)
            else:
                assert r == path, "method: %r, the oracle's %r" % (r, path)
                assert printed.strip() == str(0 if list(op["s"]) == list(op["g2"]) else float(cost[0])), (printed, cost[0])
        wrote_grid = (True,) if k == "jps1_method" else ()
    elif k == "replan_frame":
        out, reused = got
        _csr_equal(out, e["csr"], k)
        assert 0 <= reused <= len(e["csr"][3]), reused
        wrote_grid = (True,)
    elif k == "replan_frame_raw":
        out, reused, cells = got
        _csr_equal(out, e["csr"], k)
        assert 0 <= reused <= len(e["csr"][3]), reused
        _refresh_flags(out[4:9], out[9], out[10], cells, e)
        wrote_grid = (True,)
    elif k in ("set_grid_slot",):
        wrote_slots = (op["slot"],)
    elif k == "set_grid_slots":
        wrote_slots = tuple(s for s, g in op["jobs"])
    elif k == "refresh_grid_slots":
        assert list(got) == e["kept"], "kept %r, expected %r" % (list(got), e["kept"])
        wrote_slots = tuple(s for s, g in op["jobs"])
    elif k in ("prepare_slots", "refresh_slots", "prepare_slots_world", "refresh_slots_world", "prepare_slots_cropped", "refresh_slots_cropped"):
        assert len(got) == len(e["outs"])
        for j, (a, b) in enumerate(zip(got, e["outs"])):
            assert same(tuple(a), tuple(b)), "job %d: outputs %r, the host's %r" % (j, a, b)
        wrote_slots = tuple(j["slot"] for j in op["jobs"])
        for s in wrote_slots:
            if s not in m.slots:  # (a cropped job that was not planned or refused on its own leaves its slot empty)
                try:
                    p.get_grid_slot(s)
                except Exception as ex:  # noqa: BLE001
                    assert type(ex).__name__ == "FxjpsError" and ex.code == E_ARG, "slot %d must be empty: get_grid_slot raised %r" % (s, ex)
                else:
                    raise AssertionError("slot %d must be empty after a job that took no part in the call" % s)
    elif k == "prior_origin":
        want = m.prior[op["prior"]]["origin"] if op["prior"] in m.prior and m.prior[op["prior"]]["moved"] else None
        assert same(got, want), "prior_origin(%d) is %r, expected %r" % (op["prior"], got, want)
    elif k == "get_prior_map":
        want = m.prior[op["prior"]]["bytes"]
        assert got.shape == want.shape and same(got, want), "prior %d: %r bytes differ from the model's %r" % (op["prior"], got.shape, want.shape)
    elif k in ("absorb_prior", "absorb_prior_grow", "absorb_prior_slide"):
        assert len(got) == 2 and same(list(got[0]), list(e["ret"][0])), "per job %r, the host's %r" % (got[0], e["ret"][0])
        assert sorted(got[1]) == sorted(e["ret"][1]), "priors named %r, expected %r" % (sorted(got[1]), sorted(e["ret"][1]))
        for q in sorted(got[1]):
            if isinstance(got[1][q], dict):
                for f in sorted(e["ret"][1][q]):
                    assert same(got[1][q][f], e["ret"][1][q][f]), "prior %d: %s %r, the host's %r" % (q, f, got[1][q][f], e["ret"][1][q][f])
            else:
                assert got[1][q] == e["ret"][1][q], "prior %d: changed %r, the host's %r" % (q, got[1][q], e["ret"][1][q])
    elif k == "check_paths_slots":
        verdict, seg, cell = got
        for q, (v, sg, c) in enumerate(e["checks"]):
            assert (int(verdict[q]), int(seg[q]), (int(cell[q][0]), int(cell[q][1]))) == (v, sg, c), \
                "path %d on slot %d: %r, check_path on the slot's bytes %r" % (q, m.last["ids"][q], (int(verdict[q]), int(seg[q]), cell[q].tolist()), (v, sg, c))
        assert m.last is before_last
    elif k == "plan_batch_slots":
        _csr_equal(got, e["csr"], k)
    elif k in ("replan_slots", "jps1_method_many"):
        if k == "replan_slots":
            out, treused = got
            _csr_equal(out, e["csr"], k)
            flags = [int(v) for v in out[4]]
            stored = e["stored"]
            if contexts > 1 or m.mode == 0:
                assert flags == e["reused"], "out_reused %r, by the header's rule %r" % (flags, e["reused"])
            else:
                for q, f in enumerate(flags):
                    assert f == 1 if e["reused"][q] else f in (0, 2), "query %d: out_reused %d, the generation rule says %d" % (q, f, e["reused"][q])
                    assert f != 2 or (e["same"][q] and stored is not None and stored[q] > 0), "query %d: handed back by the tile rule without a stored path" % q
            assert treused == sum(1 for f in flags if f), "timing reused %d, flags %r" % (treused, flags)
        else:
            rets, printed = got
            off, cells, cost, status = e["csr"]
            want = []
            for v, (r, secs) in enumerate(rets):
                if status[v] == 0:
                    assert type(r) is int and r == 0, (v, r)
                else:
                    assert r == [(int(x), int(y)) for x, y in cells[off[v]:off[v + 1]]], "vehicle %d: path differs from the oracle's" % v
                    want.append(str(0 if list(op["calls"][v][1]) == list(op["calls"][v][2]) else float(cost[v])))
            assert printed.split() == want, "printed %r, expected %r" % (printed, want)
            wrote_slots = tuple(range(len(op["calls"])))
        if m.prev is not None:
            m.prev["status"] = [int(v) for v in e["csr"][3]]
    elif k == "publish_slots":
        for (data, wh, img), s in zip(got, op["slots"]):
            g = m.slots[s]
            ed, ew, eh = adapters.publish_map(g)
            assert tuple(wh) == (ew, eh) and same(data, ed if op["msg"] else None), "slot %d: the message differs from the adapter's" % s
            assert same(img, adapters.snapshot_image(g, op["channels"]) if op["channels"] else None), "slot %d: the image differs from the adapter's" % s
    elif k == "get_grid_slot":
        assert same(got, m.slots[op["slot"]]), "slot %d: bytes differ from the model's" % op["slot"]
    elif k in ("select_st_batch", "select_ccst_batch", "select_slots_batch", "tick_outputs_slots"):
        L = m.last
        nq = L["nq"]
        # (the resident form first: what the explicit form leaves behind -- a table of angles sized for its paths -- must
        # not be what makes the resident form right)
        try:
            res = call_wp(wp, op, nq, (L["off"], None) if k in ("select_slots_batch", "tick_outputs_slots") else None)
        except Exception as ex:  # noqa: BLE001
            raise AssertionError("the call on the resident paths raised %s: %s" % (type(ex).__name__, ex))
        explicit = call_wp(wp, op, nq, (L["off"], L["cells"]), L["ids"])
        assert same(res, explicit), "the resident paths give %r, the model's paths %r" % (res, explicit)
    if "csr" in e:
        m.last["off"], m.last["cells"] = e["csr"][0], e["csr"][1]

    _check_priors(p, m, op, i, False)

    # the derived maps: after every write, and every 8th step whatever the op was
    if wrote_grid or (i % 8 == 7 and m.grid is not None):
        check_maps(p.debug_maps(), m.grid, "resident maps", exact=m.whole, ever_free=m.ever_free)
    check = set(wrote_slots) | (set(m.slots) if i % 8 == 7 else set())
    for s in sorted(check):
        if s in m.slots:
            check_maps(p.debug_slot_maps(s), m.slots[s], "maps of slot %d" % s)
            for c in range(1, contexts):
                occ, maps = p.debug_slot_context(c, s)
                assert same(occ, m.slots[s]), "slot %d on context %d: bytes differ" % (s, c)
                check_maps(maps, m.slots[s], "maps of slot %d on context %d" % (s, c))


PRIOR_WRITERS = ("set_prior_map", "set_prior_image", "clear_prior_map", "absorb_prior", "absorb_prior_grow", "absorb_prior_slide")


def _check_priors(p, m, op, i, refused):
    """prior_origin of every prior the op names; get_prior_map of EVERY set prior (the unnamed ones too) after an op that
    writes a prior or is refused on one, and on every 8th step; a named prior that is not set must be refused."""
    k = op["op"]
    named = {op["prior"]} if "prior" in op else set()
    named |= {j["prior"] for j in op.get("jobs", ()) if isinstance(j, dict) and "ori" in j and j["prior"] is not None}
    for q in sorted(named):
        want = m.prior[q]["origin"] if q in m.prior and m.prior[q]["moved"] else None
        got = p.prior_origin(q)
        assert same(got, want), "prior_origin(%d) is %r, expected %r" % (q, got, want)
    if not (k in PRIOR_WRITERS or (refused and named) or (i % 8 == 7 and m.prior)):
        return
    for q, d in sorted(m.prior.items()):
        got = p.get_prior_map(q)
        assert got.shape == d["bytes"].shape, "prior %d has %r cells, the model's %r" % (q, got.shape, d["bytes"].shape)
        assert same(got, d["bytes"]), "prior %d: bytes differ from the model's at %r" % (q, np.argwhere(got != d["bytes"])[:5].tolist())
    for q in sorted(named - set(m.prior)):
        try:
            p.get_prior_map(q)
        except Exception as ex:  # noqa: BLE001
            assert type(ex).__name__ == "FxjpsError" and ex.code == E_ARG, "get_prior_map(%d) raised %r" % (q, ex)
        else:
            raise AssertionError("prior %d must not be set" % q)


def _refresh_flags(out5, changed, mode, cells, e):
    assert same(tuple(out5), e["out"]), "outputs %r, gridprep's %r" % (out5, e["out"])
    assert (mode == 0) == e["mode0"], "mode %d, but the prepared bytes %s the resident ones" % (mode, "equal" if e["mode0"] else "differ from")
    if mode == 0:
        assert changed == 0 and len(cells[1]) == 0
    elif mode == 1:
        xy, val = e["diff"]
        assert changed == len(xy), "changed %d, %d bytes differ" % (changed, len(xy))
        assert same(cells[0], xy) and same(cells[1], val), "last_refresh_cells %r, the differing cells %r" % (cells, (xy, val))
    else:
        assert mode == 2 and len(cells[1]) == 0 and (changed == -1 if e["diff"] is None else changed == len(e["diff"][0])), (mode, changed)
