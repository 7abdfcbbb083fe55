"""CPU suite: the random call sequences of tests/call_sequences.py, without a GPU.

HostTwin has Planner's method names and answers every op from the host references (the C oracle, oracle/gridprep.py,
oracle/adapters.py, oracle/derived_maps.py, worldprep.merge_host, the host waypoint rules).  Unlike the model it KEEPS
results: the stored results of replan_frame and replan_slots are real caches, dropped by the header's rules, and the
resident paths are whatever the last batch left.  `run` must pass on it for every seed and profile the GPU file runs.

The op lists are a function of (seed, steps, profile) alone, so what is asserted about them here -- every op kind at least
three times, every invalidating kind between a stored result and its replan, the shares of reused and searched-again
queries -- holds on the GPU too.

Teeth: a twin with ONE invalidation rule taken out must fail within the same seeds.  A twin that survives would mean the
generator never builds the order that rule exists for."""
import numpy as np
import pytest

import call_sequences as cs
from call_sequences import E_ARG, E_NOGRID, PROFILES, SEEDS, STEPS
from oracle import adapters
from oracle import derived_maps as dm

BROKEN = ("update_cells_keeps_frame_results", "set_grid_image_keeps_frame_results", "plan_batch_keeps_slot_results", "set_grid_slot_does_not_bump",
          "mode_change_keeps_slot_results", "equal_set_grid_skipped_after_update_cells", "refresh_grid_keeps_slot_results",
          "refused_batch_drops_resident_paths", "equal_set_grid_uploaded_again")


def _err(code, msg):
    from fuxi_planner_amd._lib import FxjpsError
    return FxjpsError(code, msg)


class HostTwin(object):
    def __init__(self, oracle, devices=(0,), broken=()):
        self.o = oracle
        self.devices = list(devices)
        self.broken = set(broken)
        self.grid = None
        self.memo = None       # the matrix set_grid uploaded, while nothing else wrote the grid
        self.queries = None
        self.frame = None      # stored results of replan_frame: (off, cells, cost, status)
        self.slots = {}
        self.gen = {}
        self.prior = None
        self.mode = 0
        self.rs = None         # stored results of replan_slots
        self.last = None
        self.refresh_cells = (np.zeros((0, 2), np.int32), np.zeros(0, np.uint8))
        self.reused = 0
        self.last_cost = 0.0

    def close(self):
        pass

    # -- state
    @property
    def shape(self):
        return None if self.grid is None else self.grid.shape

    def _write(self, grid, keep_frame=False, keep_rs=False):
        self.grid = np.ascontiguousarray(grid, dtype=np.uint8)
        self.memo = None
        if not keep_frame:
            self.frame = None
        if not keep_rs:
            self.rs = None

    def _batch(self, kind, res, ids=None):
        self.last = {"kind": kind, "nq": len(res[3]), "ids": ids, "off": res[0], "cells": res[1]}
        return res

    def _need(self):
        if self.grid is None:
            raise _err(E_NOGRID, "no grid")

    # -- resident grid
    def set_grid(self, matrix):
        occ = (np.asarray(matrix) == 1).astype(np.uint8)
        if self.memo is not None and self.memo.shape == occ.shape and np.array_equal(self.memo, occ) and "equal_set_grid_uploaded_again" not in self.broken:
            return
        self._write(occ)
        self.memo = occ

    def set_grid_occ(self, occ):
        self._write(occ)

    def set_grid_image(self, gray):
        keep = "set_grid_image_keeps_frame_results" in self.broken
        self._write(adapters.load_image(gray), keep_frame=keep and self.grid is not None and self.grid.shape == (gray.shape[1], gray.shape[0]))

    def prepare_grid(self, raw, start, goal, ifa, variant="st"):
        grid, out = cs.prepared(raw, start, goal, ifa, variant)
        self._write(grid)
        return out

    def prepare_occupancy_msg(self, data, width, height, start, goal, ifa, variant="st"):
        return self.prepare_grid(np.asarray(data).reshape(height, width).T, start, goal, ifa, variant)

    def _diff(self, grid):
        if self.grid is None or self.grid.shape != grid.shape:
            return None
        d = np.argwhere(self.grid != grid)
        return d.astype(np.int32), grid[d[:, 0], d[:, 1]]

    def refresh_grid(self, raw, start, goal, ifa, variant="st"):
        grid, out = cs.prepared(raw, start, goal, ifa, variant)
        d = self._diff(grid)
        self._write(grid, keep_rs="refresh_grid_keeps_slot_results" in self.broken)
        self.refresh_cells = d if d is not None and len(d[0]) else (np.zeros((0, 2), np.int32), np.zeros(0, np.uint8))
        return out + ((-1, 2) if d is None else (len(d[0]), 1 if len(d[0]) else 0))

    def last_refresh_cells(self):
        return self.refresh_cells

    def get_grid(self, context=0):
        self._need()
        return self.grid.copy()

    def publish_map(self):
        self._need()
        return adapters.publish_map(cs.truth(self.grid))

    def snapshot_image(self, channels=1):
        self._need()
        return adapters.snapshot_image(cs.truth(self.grid), channels)

    def _apply(self, xy, val):
        g = self.grid.copy()
        for (x, y), v in zip(np.asarray(xy).reshape(-1, 2), val):
            if 0 <= x < g.shape[0] and 0 <= y < g.shape[1]:
                g[x, y] = 1 if v else 0
        return g

    def update_cells(self, xy, val, rebuild=True):
        self._need()
        g = self._apply(xy, val)
        memo = self.memo if "equal_set_grid_skipped_after_update_cells" in self.broken else None
        self._write(g, keep_frame="update_cells_keeps_frame_results" in self.broken)
        self.memo = memo

    # -- planning
    def _hchoice(self, h):
        if h not in (1, 2):
            raise TypeError("hchoice must be 1 or 2")

    def plan_batch(self, starts, goals, hchoice=2, max_path_len=None):
        self._need()
        self._hchoice(hchoice)
        W, H = self.grid.shape
        res = cs.csr(self.o, self.grid, starts, goals, hchoice, W * H + 1 if max_path_len is None else max_path_len)
        self.frame, self.reused = None, 0
        if "plan_batch_keeps_slot_results" not in self.broken:
            self.rs = None
        return self._batch("resident", res)

    def plan_one(self, start, goal, hchoice=2):
        off, cells, cost, status = self.plan_batch([start], [goal], hchoice)
        return int(status[0]), float(cost[0]), cells

    def plan(self, start, goal, hchoice=2):
        st, cost, cells = self.plan_one(start, goal, hchoice)
        self.last_cost = cost
        if st == cs.Q_BAD_START:
            raise IndexError("start outside the grid")
        if st < 0:
            raise _err(st, "query failed")
        return [(int(x), int(y)) for x, y in cells]

    def set_queries(self, starts, goals, hchoice=2, max_path_len=None):
        self._need()
        self._hchoice(hchoice)
        self.queries = (np.array(starts, np.int32).reshape(-1, 2), np.array(goals, np.int32).reshape(-1, 2), hchoice, max_path_len)
        self.frame = self.rs = None

    def _frame(self, grid):
        """Plan the stored queries on `grid`, which replaces the resident one: the stored results when they stand and no
        cell's truth changes."""
        if self.frame is not None and self.grid.shape == grid.shape and np.array_equal(self.grid != 0, grid != 0):
            res, self.reused = self.frame, len(self.frame[3])
        else:
            s, g, h, mpl = self.queries
            res, self.reused = cs.csr(self.o, grid, s, g, h, mpl), 0
        self._write(grid)
        self.frame = res
        return self._batch("resident", res)

    def replan_frame(self, xy=None, val=None):
        if self.queries is None:
            raise _err(E_ARG, "replan_frame before set_queries")
        self._need()
        return self._frame(self._apply(xy, val))

    def replan_frame_raw(self, raw, start, goal, ifa, variant="st"):
        self.memo = None  # (as Planner: forgotten before the call, whatever becomes of it)
        grid, out = cs.prepared(raw, start, goal, ifa, variant)
        if self.queries is None or self.grid is None or self.grid.shape != grid.shape:
            raise _err(E_ARG, "replan_frame_raw needs set_queries and a grid of the prepared extents")
        d = self._diff(grid)
        self.refresh_cells = d
        return tuple(self._frame(grid)) + out + (len(d[0]), 1 if len(d[0]) else 0)

    def timing(self):
        return {"reused": self.reused}

    # -- slots
    def _bump(self, slot):
        self.gen[slot] = self.gen.get(slot, 0) + 1

    def _slot_set(self, slot, grid, bump=True):
        self.slots[slot] = np.ascontiguousarray(grid, dtype=np.uint8)
        if bump:
            self._bump(slot)

    def _slot_refresh(self, slot, grid):
        old = self.slots.get(slot)
        kept = old is not None and old.shape == grid.shape and np.array_equal(old, grid)
        if not kept:
            self._slot_set(slot, grid)
        return kept

    def set_grid_slot(self, slot, matrix):
        self._slot_set(slot, (np.asarray(matrix) == 1).astype(np.uint8), bump="set_grid_slot_does_not_bump" not in self.broken)

    def clear_grid_slot(self, slot):
        self.slots.pop(slot, None)
        self._bump(slot)

    def get_grid_slot(self, slot):
        if slot not in self.slots:
            raise _err(E_ARG, "empty slot")
        return self.slots[slot].copy()

    def set_grid_slots(self, jobs):
        for slot, m in jobs:
            self._slot_set(slot, (np.asarray(m) == 1).astype(np.uint8))

    def refresh_grid_slots(self, jobs):
        return [self._slot_refresh(slot, (np.asarray(m) == 1).astype(np.uint8)) for slot, m in jobs]

    def _jobs(self, jobs, refresh, world):
        outs = []
        for j in jobs:
            if world:
                grid, out, w = cs.world_prepared(j, self.prior)
            else:
                raw = j[1]
                raw = np.asarray(raw[0]).reshape(raw[2], raw[1]).T if isinstance(raw, tuple) else raw
                grid, out = cs.prepared(raw, j[2], j[3], j[4], j[5])
                w = ()
            if refresh:
                outs.append(out + (True, self._slot_refresh(j[0], grid)) + w)
            else:
                self._slot_set(j[0], grid)
                outs.append(out + (True,) + w)
        return outs

    def prepare_slots(self, jobs):
        return self._jobs(jobs, False, False)

    def refresh_slots(self, jobs):
        return self._jobs(jobs, True, False)

    def prepare_slots_world(self, jobs):
        return self._jobs(jobs, False, True)

    def refresh_slots_world(self, jobs):
        return self._jobs(jobs, True, True)

    def set_prior_map(self, prior, matrix):
        self.prior = (np.asarray(matrix) > 0).astype(np.uint8)

    def _slots_args(self, ids, hchoice):
        self._hchoice(hchoice)
        if any(i not in self.slots for i in ids):
            if "refused_batch_drops_resident_paths" in self.broken:
                self.last = None
            raise _err(E_ARG, "an empty slot is named")

    def plan_batch_slots(self, ids, starts, goals, hchoice=2, max_path_len=None):
        ids = [int(i) for i in ids]
        self._slots_args(ids, hchoice)
        res = cs.csr(self.o, [self.slots[i] for i in ids], starts, goals, hchoice, max_path_len)
        self.frame = self.rs = None
        self.reused = 0
        return self._batch("slots", res, ids)

    def replan_slots(self, ids, starts, goals, hchoice=2, max_path_len=None):
        ids = [int(i) for i in ids]
        self._slots_args(ids, hchoice)
        if len(self.devices) > 1:
            return self.plan_batch_slots(ids, starts, goals, hchoice, max_path_len) + (np.zeros(len(ids), np.int32),)
        s, g = np.array(starts, np.int32).reshape(-1, 2), np.array(goals, np.int32).reshape(-1, 2)
        n = len(ids)
        r = self.rs
        ok = r is not None and len(r["ids"]) == n and r["h"] == hchoice and r["mpl"] == max_path_len
        flags = np.zeros(n, np.int32)
        per = []
        for q in range(n):
            if ok and r["ids"][q] == ids[q] and np.array_equal(r["s"][q], s[q]) and np.array_equal(r["g"][q], g[q]) and r["gen"][q] == self.gen.get(ids[q], 0):
                flags[q] = 1
                per.append(r["per"][q])
            else:
                off, cells, cost, status = cs.csr(self.o, [self.slots[ids[q]]], s[q:q + 1], g[q:q + 1], hchoice, max_path_len)
                per.append((cells, cost[0], status[0]))
        status = np.array([p[2] for p in per], np.int32)
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum(np.maximum(status, 0))
        cells = np.concatenate([p[0] for p in per]).reshape(-1, 2).astype(np.int32) if n else np.zeros((0, 2), np.int32)
        res = (off, cells, np.array([p[1] for p in per], np.float64), status)
        self.frame = None
        self.rs = {"ids": ids, "s": s, "g": g, "h": hchoice, "mpl": max_path_len, "gen": [self.gen.get(i, 0) for i in ids], "per": per}
        self.reused = int(flags.sum())
        return self._batch("slots", res, ids) + (flags,)

    def set_slot_reuse(self, mode):
        new = {"generation": 0, "tiles": 1}[mode]
        if new != self.mode:
            self.mode = new
            if "mode_change_keeps_slot_results" not in self.broken:
                self.rs = None

    def publish_slots(self, slots, msg=True, image_channels=None):
        out = []
        for s in slots:
            if s not in self.slots:
                raise _err(E_ARG, "empty slot")
            g = self.slots[s]
            d, w, h = adapters.publish_map(g)
            out.append((d if msg else None, (w, h), adapters.snapshot_image(g, image_channels) if image_channels else None))
        return out

    # -- the derived maps
    def debug_maps(self):
        return dm.reference_maps(cs.truth(self.grid))

    def debug_slot_maps(self, slot):
        return dm.reference_maps(cs.truth(self.slots[slot]))

    def debug_slot_context(self, context, slot):
        return self.slots[slot].copy(), self.debug_slot_maps(slot)

    # -- the waypoint calls: the host rules path by path, on explicit paths or on those the last batch left
    def _paths(self, nq, paths, want):
        if paths is not None and paths[1] is not None:
            return np.asarray(paths[0]), np.asarray(paths[1]).reshape(-1, 2), None
        L = self.last
        if L is None or L["nq"] != nq or (want is not None and L["kind"] != want):
            raise _err(E_ARG, "not the last batch's")
        return L["off"], L["cells"], L["ids"]

    def _rows(self, nq, paths, want, rule, ms, pos, goal, eo, pw, pd, ids):
        from fuxi_planner_amd import waypoints
        off, cells, lids = self._paths(nq, paths, want)
        ids = lids if ids is None else ids
        rows = []
        for q in range(nq):
            path = cells[off[q]:off[q + 1]]
            e = 0 if eo is None else int(eo[q])
            if len(path) == 0:
                rows.append((np.array(goal[q]), 3, np.array(goal[q]), 0.0, 0))
            elif rule[q] == 0:
                prev = None if pw is None or pd[q] == 0 else pw[q][:pd[q]]
                wp, gout, ang = waypoints.select_st(path, ms[q], cs.R, (-2.0, 1.0), pos[q], goal[q], e, prev_wp=prev)
                rows.append((np.r_[wp, np.zeros(3 - len(wp))], len(wp), gout, ang, 0))
            else:
                grid = self.grid if ids is None else self.slots[ids[q]]
                wp, kept, gout = waypoints.select_ccst(path, cs.truth(grid), cs.R, (-2.0, 1.0), pos[q], goal[q], e, return_goal=True)
                rows.append((wp, 3, gout, 0.0, len(kept)))
        return tuple(np.array([r[c] for r in rows]) for c in range(5))

    def select_st_batch(self, nq, map_start, map_reso, map_o, pos, global_goal, end_occu=None, prev_wp=None, prev_dim=None, paths=None):
        return self._rows(nq, paths, None, [0] * nq, map_start, pos, global_goal, end_occu, prev_wp, prev_dim, None)[:4]

    def select_ccst_batch(self, nq, map_reso, map_o, pos, global_goal, end_occu=None, paths=None):
        self._need()
        return self._rows(nq, paths, "resident", [1] * nq, None, pos, global_goal, end_occu, None, None, None)

    def select_slots_batch(self, rule, map_start, map_reso, map_o, pos, global_goal, end_occu=None, prev_wp=None, prev_dim=None, grid_ids=None,
                           paths=None):
        return self._rows(len(rule), paths, "slots", rule, map_start, pos, global_goal, end_occu, prev_wp, prev_dim, grid_ids)

    def tick_outputs_slots(self, rule, map_start, map_reso, map_o, pos, global_goal, home, end_occu=None, prev_wp=None, prev_dim=None, grid_ids=None,
                           paths=None, offsets=None):
        return self._rows(len(rule), paths, "slots", rule, map_start, pos, global_goal, end_occu, prev_wp, prev_dim, grid_ids) + (np.asarray(home),)

    # -- the jps1 shim's two entry points, composed as fuxi_planner_amd/jps1.py composes them
    def jps1_method(self, matrix, start, goal, hchoice):
        self.set_grid(matrix)
        st, cost, cells = self.plan_one(start, goal, hchoice)
        if st == cs.Q_BAD_START:
            raise IndexError("start outside the grid")
        if st == 0:
            return (0, 0.0)
        print(0 if tuple(start) == tuple(goal) else cost)
        return ([(int(x), int(y)) for x, y in cells], 0.0)

    def jps1_method_many(self, calls, hchoice):
        self._hchoice(hchoice)
        self.refresh_grid_slots([(v, c[0]) for v, c in enumerate(calls)])
        ids = list(range(len(calls)))
        mpl = max(cs.default_mpl(*self.slots[i].shape) for i in ids)
        off, cells, cost, status, _ = self.replan_slots(ids, [c[1] for c in calls], [c[2] for c in calls], hchoice, mpl)
        out = []
        for v, st in enumerate(status):
            if st == 0:
                out.append((0, 0.0))
                continue
            out.append(([(int(x), int(y)) for x, y in cells[off[v]:off[v + 1]]], 0.0))
            print(0 if tuple(calls[v][1]) == tuple(calls[v][2]) else float(cost[v]))
        return out


def contexts_of(profile):
    return 2 if profile == "two_contexts" else 1


def run_twin(oracle, profile, seed, broken=()):
    dev = [0] * contexts_of(profile)
    return cs.run(HostTwin(oracle, dev, broken), cs.generate(seed, STEPS, profile), oracle, fresh=lambda: HostTwin(oracle, dev), contexts=len(dev),
                  seed=(profile, seed))


# ------------------------------------------------------------------ the twin passes
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("profile", PROFILES)
def test_twin_passes_every_sequence(oracle, profile, seed):
    run_twin(oracle, profile, seed)


def test_op_lists_are_a_function_of_their_arguments():
    assert cs.generate(1, 60, "tiles") == cs.generate(1, 60, "tiles")
    assert cs.generate(1, 60, "tiles") != cs.generate(2, 60, "tiles")


# ------------------------------------------------------------------ coverage conditions on the op lists
def walk(profile, seed):
    """-> (ops, per op: what the model expected or the Refused it raised, and the model's stored-results state before it)."""
    ops = cs.generate(seed, STEPS, profile)
    m = cs.Model(contexts_of(profile))
    out = []
    for op in ops:
        had = {"slots": m.prev is not None, "frame_queries": m.queries is not None}
        try:
            e = cs.expect(m, op)
        except cs.Refused as r:
            e = r
        had["slots_after"] = m.prev is not None
        out.append((op, e, had))
    return out


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("profile", PROFILES)
def test_every_op_kind_at_least_three_times_and_the_forced_shapes(profile, seed):
    w = walk(profile, seed)
    count = {}
    for op, e, had in w:
        count[op["op"]] = count.get(op["op"], 0) + 1
    few = {k: count.get(k, 0) for k in cs.kinds_of(profile) if count.get(k, 0) < 3}
    assert not few, few
    refused = [op for op, e, had in w if isinstance(e, cs.Refused)]
    assert any(op.get("hchoice") == 3 for op in refused), "no hchoice 3"
    assert any(set(op.get("ids", ())) & set(cs.EMPTY_SLOTS) for op in refused), "no batch that names an empty slot"
    assert any(op["op"] == "replan_frame_raw" for op in refused), "no replan_frame_raw of other extents"
    assert any(op["op"] in ("select_st_batch", "select_ccst_batch", "select_slots_batch", "tick_outputs_slots") for op in refused), "no wrong nq"
    # the forced shapes, read off the model as the ops go by
    m = cs.Model(contexts_of(profile))
    shapes, slot_shapes, kept = [], set(), set()
    for op, e, had in w:
        before = m.grid
        try:
            ex = cs.expect(m, op)
        except cs.Refused:
            continue
        if m.grid is not before:
            shapes.append(m.grid.shape)
        slot_shapes |= {g.shape for g in m.slots.values()}
        kept |= set(ex.get("kept", [])) | {o[6] for o in ex.get("outs", []) if op["op"].startswith("refresh")}
    assert any(min(s) == 1 for s in shapes), "no 1-wide resident grid"
    assert any(65 <= s[0] <= 140 and s[1] % 64 for s in shapes), "no resident grid whose lines cross a 64-bit word"
    assert any(a == b for a, b in zip(shapes, shapes[1:])) and any(a != b for a, b in zip(shapes, shapes[1:]))
    assert len(slot_shapes) >= 3 and any(min(s) == 1 for s in slot_shapes) and any(max(s) >= 65 for s in slot_shapes)
    assert kept == {True, False}, kept
    assert {0, 1} <= {len(op["s"]) for op, e, had in w if op["op"] == "plan_batch" and not isinstance(e, cs.Refused)}, "no plan_batch of 0 and of 1 queries"
    for kind in ("select_slots_batch", "tick_outputs_slots"):
        assert {"none", "offsets"} <= {op["form"] for op, e, had in w if op["op"] == kind and not isinstance(e, cs.Refused)}, kind
    assert max(max(s) for s in shapes) <= 1024


BATCH_CALLS = ("plan_batch", "plan_one", "plan", "plan_batch_slots", "replan_slots", "replan_frame", "replan_frame_raw", "jps1_method",
               "jps1_method_many")


def same_batch(a, b):
    return all(a[k] == b[k] for k in ("ids", "s", "g", "hchoice", "mpl"))


@pytest.mark.parametrize("profile", PROFILES)
def test_every_invalidating_kind_lies_between_stored_results_and_their_replan(profile):
    """Over the seeds of a profile, for every kind K that drops stored results: a replan call has stored its results; K is
    the FIRST call after it that drops them (they were still there when it ran); and the next batch call -- K itself apart
    -- is the matching replan, for replan_slots with the arguments of the stored one.  And the shares of replan_slots
    queries the header's rule hands back, and of those searched although the previous call stored a result for them."""
    seen_slots, seen_frame = set(), set()
    reused = searched_again = total = 0
    for seed in SEEDS:
        # stored: the replan op whose results stand; K: the one dropper seen since (None: none yet)
        stored_s = k_s = stored_f = k_f = None
        for op, e, had in walk(profile, seed):
            k = op["op"]
            if isinstance(e, cs.Refused):
                continue  # (a refused call touches nothing)
            if k == "replan_slots":
                total += len(e["reused"])
                reused += sum(e["reused"])
                searched_again += sum(1 for q, f in enumerate(e["reused"]) if not f and e["same"][q])
            # -- the slot results: the model says whether they stood before and after the op
            if stored_s is not None and k_s is not None and k in BATCH_CALLS:
                if k == "replan_slots" and same_batch(op, stored_s):
                    seen_slots.add(k_s)
                stored_s = k_s = None
            if stored_s is not None and k_s is None and had["slots"] and not had["slots_after"]:
                k_s = k  # the first dropper, on results that were there
            if k == "replan_slots" and had["slots_after"]:
                stored_s, k_s = op, None
            elif stored_s is not None and k_s is None and not had["slots_after"]:
                stored_s = None
            # -- the frame results: dropped by kind (a set_grid that was skipped drops nothing)
            dropper = k in cs.FRAME_DROPPERS and not (k == "set_grid" and e.get("skipped"))
            if stored_f is not None and k_f is not None and k in BATCH_CALLS:
                if k in ("replan_frame", "replan_frame_raw"):
                    seen_frame.add(k_f)
                stored_f = k_f = None
            if stored_f is not None and k_f is None and dropper:
                k_f = k
            if k in ("replan_frame", "replan_frame_raw"):
                stored_f, k_f = op, None
    want_s = set(cs.SLOT_DROPPERS) | ({"set_slot_reuse"} if profile == "tiles" else set())
    want_f = set(cs.FRAME_DROPPERS)
    if profile != "two_contexts":  # (several contexts: replan_slots is a plain batch and stores nothing)
        assert not want_s - seen_slots, "never the first dropper between a replan_slots and its repeat: %r" % sorted(want_s - seen_slots)
        assert 10 * reused >= total, (reused, total)
        assert 10 * searched_again >= total, (searched_again, total)
    assert not want_f - seen_frame, "never the first dropper between two replan_frame calls: %r" % sorted(want_f - seen_frame)


# ------------------------------------------------------------------ teeth
@pytest.mark.parametrize("broken", BROKEN)
def test_a_twin_without_one_invalidation_rule_fails(oracle, broken):
    profiles = ("tiles",) if broken == "mode_change_keeps_slot_results" else ("single", "tiles")
    for profile in profiles:
        for seed in SEEDS:
            try:
                run_twin(oracle, profile, seed, broken=(broken,))
            except cs.Mismatch as mm:
                assert mm.assertion, "the twin crashed instead of answering wrongly: %s" % str(mm)[:400]
                return
    raise AssertionError("a twin with %r passes every sequence: the generator never builds the order this rule is for" % broken)
