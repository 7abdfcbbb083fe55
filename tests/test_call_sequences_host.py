"""CPU suite: the random call sequences of tests/call_sequences.py, without a GPU.

HostTwin has Planner's method names and answers every op from the host references (the C oracle, oracle/gridprep.py,
oracle/adapters.py, oracle/derived_maps.py, worldprep.merge_host, the host waypoint rules).  Unlike the model it KEEPS
results: the stored results of replan_frame and replan_slots are real caches, dropped by the header's rules, and the
resident paths are whatever the last batch left.  `run` must pass on it for every seed and profile the GPU file runs.

The op lists are a function of (seed, steps, profile) alone, so what is asserted about them here -- every op kind at least
three times, every invalidating kind between a stored result and its replan, the shares of reused and searched-again
queries -- holds on the GPU too.

Teeth: a twin with ONE invalidation rule taken out must fail within the same seeds.  A twin that survives would mean the
generator never builds the order that rule exists for.

The world profiles (`world`, `world_two_contexts`): the twin holds the prior maps and the origins Planner remembers, and
answers absorb / grow / slide, the cropped prepares and check_paths_slots from worldprep's and waypoints' host references.
test_world_sequences_hold_the_orders_in_which_a_prior_goes_stale asserts, for every seed, what the op lists alone show:
every new kind three times, every new refusal, grows and slides that change extents and move an origin, a trimmed slide
with a non-zero cut_lo and an over_limit slide left untrimmed, a refresh with the slot's last job that is NOT kept because
only the prior changed and one that IS kept after an absorb elsewhere, equal replans straight after a prior-writing op, a
world job naming a released prior, a job carrying the upload's origin after a grow, a world refresh under the tile rule.
WORLD_BROKEN are the twins with one prior rule taken out.  DIGESTS pins the op lists of the four earlier profiles to what
the generator drew before the world profiles were added."""
import numpy as np
import pytest

import call_sequences as cs
import hashlib

from call_sequences import ALL_PROFILES, E_ARG, E_NOGRID, PROFILES, SEEDS, STEPS, WORLD_PROFILES
from oracle import adapters
from oracle import derived_maps as dm

BROKEN = ("update_cells_keeps_frame_results", "set_grid_image_keeps_frame_results", "plan_batch_keeps_slot_results", "set_grid_slot_does_not_bump",
          "mode_change_keeps_slot_results", "equal_set_grid_skipped_after_update_cells", "refresh_grid_keeps_slot_results",
          "refused_batch_drops_resident_paths", "equal_set_grid_uploaded_again")
WORLD_BROKEN = ("absorb_drops_slot_results", "absorb_bumps_generation", "grow_keeps_old_origin", "refused_grow_swaps_prior", "set_prior_keeps_moved_origin",
                "clear_prior_keeps_bytes", "slide_over_limit_never_trims", "absorb_writes_unnamed_prior", "refresh_world_keeps_by_job",
                "check_paths_reads_batch_time_slots")

# sha256 of repr(generate(seed, STEPS, profile)) as the generator stood before the world profiles were added (commit 73e1e4d)
DIGESTS = {
    ('single', 0): "867cb5a6cde02a9bc552f7556371a4de1f1f8018278e73a31823aa11b7d54426",
    ('single', 1): "66e698a06a9dac7d6c9b608acd2ef81791935b754052c52f06dd59b6a5ec0379",
    ('single', 2): "24d1b7cc750ba06d7d74763c715d6d6d9b730f508547e1b6b24d2d8c095135ce",
    ('single', 3): "167a0d2e77c0ae8871e5f69cfc876aaa31c7929eb16edd5903c94c64b8bc8e9c",
    ('tiles', 0): "cb20562cdd54f5853a171f31295160928c655fc5da2a920b93d7289401c1bcfe",
    ('tiles', 1): "8d09f5de9a053f9aec3c337c7563ef8ae276dd8b46d6b4ffb30cf0c2c4a05baf",
    ('tiles', 2): "dc3b0054c182f4ca8e02c769dd6bcdd03b68b299e56a0ac0a0fee93d0b246ba5",
    ('tiles', 3): "22073a64b7b0364ba8d67acf2907abf7b9210978df54b478c87c7c32241dda13",
    ('two_contexts', 0): "7eadf425e589a8177b435134d8369938549aaf69bd252188f595cc7be57e340b",
    ('two_contexts', 1): "06698bcd7840aa4395307aceca3a1657711aba5ca1fccde6e3b5034c69ddcc3f",
    ('two_contexts', 2): "75eed9292adf263482aa0477807004d2289f55a5b0c9a99dc5c38bd1d3df3f3b",
    ('two_contexts', 3): "63e923b9f91057040cede5104ab4747a22aa83ee4471e5a52b05b90792f2217f",
    ('shim', 0): "5ff821f30849f9935778ca676521102df2998481effca275d0d0b54b73bbdd85",
    ('shim', 1): "071f07ee8658991b58a5a12e0d355a2a641246c17517e13371350c2daf3cf935",
    ('shim', 2): "4e477cdf8f483498be3da9e0f4e9e169c54dc1527dd95f6a29ea698b1f59ec25",
    ('shim', 3): "bc24dd40ffe5963add017a77e8904c60652ec1cd68cb965409bbdd1b039fb727",
}


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
        self.prior = {}        # index -> bytes
        self.origins = {}      # index -> the origin a grow or slide left (Planner's memory: the library stores none)
        self.last_job = {}     # slot -> the world job that wrote it last (read by a broken twin only)
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
        self.batch_slots = dict(self.slots)  # (read by a broken twin only)
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
        self._was = old
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

    def _jobs(self, jobs, refresh, world, cropped=False):
        done = []
        for j in jobs:
            tail = ()
            try:
                if cropped:
                    grid, out, w, tail = cs.crop_prepared(j, self.prior)
                elif world:
                    grid, out, w = cs.world_prepared(j, cs.named_prior(self.prior, j))
                else:
                    raw = j[1]
                    raw = np.asarray(raw[0]).reshape(raw[2], raw[1]).T if isinstance(raw, tuple) else raw
                    grid, out = cs.prepared(raw, j[2], j[3], j[4], j[5])
                    w = ()
            except ValueError as ex:
                if not world:
                    raise
                raise _err(E_ARG, str(ex))  # (the whole call, before a slot is written)
            done.append((grid, out, w, tail))
        outs = []
        for j, (grid, out, w, tail) in zip(jobs, done):
            if grid is None:
                self.clear_grid_slot(j[0])
                outs.append(out + ((False,) if refresh else ()) + w + tail)
            elif refresh:
                kept = self._slot_refresh(j[0], grid)
                if "refresh_world_keeps_by_job" in self.broken and world and not cropped and cs.same(self.last_job.get(j[0]), j[1:]) and not kept:
                    self.slots[j[0]], kept = self._was, True  # (judged from the job alone: the slot stays as it was)
                    self.gen[j[0]] -= 1
                outs.append(out + (True, kept) + w + tail)
            else:
                self._slot_set(j[0], grid)
                outs.append(out + (True,) + w + tail)
            self.last_job[j[0]] = j[1:] if world and not cropped else None
        return outs

    def prepare_slots(self, jobs):
        return self._jobs(jobs, False, False)

    def refresh_slots(self, jobs):
        return self._jobs(jobs, True, False)

    def prepare_slots_world(self, jobs):
        return self._jobs(jobs, False, True)

    def refresh_slots_world(self, jobs):
        return self._jobs(jobs, True, True)

    def prepare_slots_cropped(self, jobs):
        return self._jobs(jobs, False, True, cropped=True)

    def refresh_slots_cropped(self, jobs):
        return self._jobs(jobs, True, True, cropped=True)

    # -- the shared prior maps
    def set_prior_map(self, prior, matrix):
        self.prior[prior] = (np.asarray(matrix) > 0).astype(np.uint8)
        if "set_prior_keeps_moved_origin" not in self.broken:
            self.origins.pop(prior, None)

    def set_prior_image(self, prior, gray):
        from fuxi_planner_amd import worldprep
        self.set_prior_map(prior, worldprep.prior_from_image(gray))

    def clear_prior_map(self, prior):
        self.origins.pop(prior, None)
        if "clear_prior_keeps_bytes" not in self.broken:
            self.prior.pop(prior, None)

    def get_prior_map(self, prior):
        if prior not in self.prior:
            raise _err(E_ARG, "the prior is not set")
        return self.prior[prior].copy()

    def prior_origin(self, prior):
        return self.origins.get(prior)

    def _fold(self, op, jobs, crops):
        """One absorb / grow / slide call by cs.prior_fold (worldprep's host references) on the twin's own priors."""
        b = self.broken
        try:
            if "slide_over_limit_never_trims" in b and op.get("use") == "over_limit":
                op = dict(op, use="none", keep={}, limit=8190)
            after, origin, ret = cs.prior_fold(self.prior, jobs, op, crops)
        except ValueError as ex:
            if "refused_grow_swaps_prior" in b and op["op"] != "absorb_prior" and "above" in str(ex):
                try:  # (the limit is found too late: the grown priors are already in place)
                    self.prior.update(cs.prior_fold(self.prior, jobs, dict(op, limit=8190), crops)[0])
                except ValueError:
                    pass
            raise _err(E_ARG, str(ex))
        self.prior.update(after)
        if "grow_keeps_old_origin" in b:
            ret = (ret[0], {p: dict(r, origin=list(self.origins.get(p, jobs[[j[8] for j in jobs].index(p)][9]))) for p, r in ret[1].items()})
        else:
            self.origins.update({p: (float(o[0]), float(o[1])) for p, o in origin.items()})
        if "absorb_drops_slot_results" in b:
            self.rs = None
        if "absorb_bumps_generation" in b:
            for s in self.slots:
                self._bump(s)
        if "absorb_writes_unnamed_prior" in b:
            for p in self.prior:
                if p not in after:
                    self.prior[p] = self.prior[p].copy()
                    self.prior[p][0, 0] ^= 1
        return ret

    def absorb_prior(self, jobs, mode="overwrite", crops=None):
        return self._fold({"op": "absorb_prior", "mode": mode}, list(jobs), crops)

    def absorb_prior_grow(self, jobs, mode="overwrite", crops=None, limit=None):
        return self._fold({"op": "absorb_prior_grow", "mode": mode, "limit": limit}, list(jobs), crops)

    def absorb_prior_slide(self, jobs, mode="overwrite", crops=None, limit=None, keep=None, use="over_limit"):
        inf = float("inf")
        keep = {p: [[None if v == -inf else v for v in lo], [None if v == inf else v for v in hi]] for p, (lo, hi) in (keep or {}).items()}
        return self._fold({"op": "absorb_prior_slide", "mode": mode, "limit": limit, "keep": keep, "use": use}, list(jobs), crops)

    def check_paths_slots(self, grid_ids, offsets, cells, shift=None):
        from fuxi_planner_amd import waypoints
        ids = [int(i) for i in grid_ids]
        if any(i not in self.slots for i in ids):
            raise _err(E_ARG, "an empty slot is named")
        slots = self.batch_slots if "check_paths_reads_batch_time_slots" in self.broken else self.slots
        off, cells = np.asarray(offsets), np.asarray(cells).reshape(-1, 2)
        res = [waypoints.check_path(cells[off[q]:off[q + 1]], slots[i], shift) for q, i in enumerate(ids)]
        return (np.array([r[0] for r in res], np.int32), np.array([r[1] for r in res], np.int32), np.array([r[2] for r in res], np.int32).reshape(-1, 2))

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
    return 2 if profile in ("two_contexts", "world_two_contexts") else 1


def run_twin(oracle, profile, seed, broken=()):
    dev = [0] * contexts_of(profile)
    return cs.run(HostTwin(oracle, dev, broken), cs.generate(seed, STEPS, profile), oracle, fresh=lambda: HostTwin(oracle, dev), contexts=len(dev),
                  seed=(profile, seed))


# ------------------------------------------------------------------ the twin passes
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("profile", ALL_PROFILES)
def test_twin_passes_every_sequence(oracle, profile, seed):
    run_twin(oracle, profile, seed)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("profile", PROFILES)
def test_the_earlier_profiles_draw_the_op_lists_they_drew(profile, seed):
    """The world profiles have their own generator and their own draws: the sequences of the four earlier profiles are,
    op for op, those the suite ran before."""
    assert hashlib.sha256(repr(cs.generate(seed, STEPS, profile)).encode()).hexdigest() == DIGESTS[(profile, seed)]


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


SLOT_JOB_KINDS = ("prepare_slots_world", "refresh_slots_world", "prepare_slots_cropped", "refresh_slots_cropped")
FOLDS = ("absorb_prior", "absorb_prior_grow", "absorb_prior_slide")
VERDICTS = {"VALID": 1, "EMPTY": 0, "BLOCKED": 2, "OUTSIDE": 3}  # FXJPS_PATH_*


def world_facts(profile, seed, oracle):
    """What the op list of a world sequence holds, read off the model as the ops go by (the oracle gives the paths that
    check_paths_slots is expected to judge)."""
    m = cs.Model(contexts_of(profile))
    f = {"count": {}, "refusals": set(), "refused": 0, "extents": 0, "origin": 0, "cut_lo": 0, "untrimmed": 0, "not_kept": 0, "kept": 0, "reused": 0,
         "replans_after_a_fold": 0, "verdicts": set(), "statuses": set(), "stale_origin": 0, "tiles_refresh": 0}
    last_job, absorbed, cleared, prior_written, previous = {}, {}, set(), False, None
    ops = cs.generate(seed, STEPS, profile)
    f["steps"] = len(ops)
    for op in ops:
        k = op["op"]
        f["count"][k] = f["count"].get(k, 0) + 1
        before = {p: (d["bytes"].shape, d["origin"]) for p, d in m.prior.items()}
        set_before = set(m.prior)
        try:
            e = cs.expect(m, op, oracle)
        except cs.Refused:
            f["refused"] += 1
            if k in FOLDS:
                try:
                    cs.fold_of(m.prior_bytes(), op)
                except ValueError as ex:
                    for word, name in (("is not set", "prior_not_set"), ("above", "grow_past_limit"), ("holds no cell", "slide_empty_window"),
                                       ("no job names", "window_unnamed_prior"), ("differ from those", "unequal_ori_pre")):
                        if word in str(ex):
                            assert name != "grow_past_limit" or not any(u != "none" for u in [op.get("use", "none")] if op.get("keep")), op
                            f["refusals"].add(name)
            elif k in SLOT_JOB_KINDS and any(j["prior"] in cleared and j["prior"] not in set_before for j in op["jobs"]):
                f["refusals"].add("world_cleared_prior")
            continue
        if k == "clear_prior_map":
            cleared.add(op["prior"])
        if k in FOLDS + ("set_prior_map", "set_prior_image", "clear_prior_map"):
            prior_written = True
        if k in FOLDS:
            changed = {p: (r["changed"] if isinstance(r, dict) else r) for p, r in e["ret"][1].items()}
            if k == "absorb_prior" and sum(changed.values()) > 0:
                absorbed = {s: True for s in m.slots}
            for p, r in e["ret"][1].items():
                if k != "absorb_prior":
                    f["extents"] += (r["W"], r["H"]) != before[p][0]
                    f["origin"] += tuple(r["origin"]) != tuple(before[p][1])
                if k == "absorb_prior_slide":
                    f["cut_lo"] += r["trimmed"] and any(r["cut_lo"])
                    f["untrimmed"] += op["use"] == "over_limit" and p in op["keep"] and not r["trimmed"]
        if k in SLOT_JOB_KINDS:
            prior_written = False
            for j, out in zip(op["jobs"], e["outs"]):
                if k.endswith("_cropped"):
                    f["statuses"].add(out[-2])
                if j["prior"] is not None and m.prior[j["prior"]]["moved"] and tuple(j["ori"]) != m.prior[j["prior"]]["origin"]:
                    f["stale_origin"] += 1
                if k.startswith("refresh") and out[5] and j == last_job.get(j["slot"]):  # (raw, position, goal, prior and origin repeated)
                    f["not_kept"] += not out[6]
                    f["kept"] += bool(out[6]) and absorbed.get(j["slot"], False)
                    f["tiles_refresh"] += not out[6] and m.mode == 1
                last_job[j["slot"]] = j
                absorbed[j["slot"]] = False
        if k == "replan_slots":
            if prior_written and e["reused"] and all(e["reused"]):
                f["reused"] += 1
            f["replans_after_a_fold"] += prior_written and previous is not None and same_batch(op, previous)
            prior_written, previous = False, op
        elif k in BATCH_CALLS:
            previous = None
        if k == "check_paths_slots":
            f["verdicts"] |= {c[0] for c in e["checks"]}
    return f


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("profile", WORLD_PROFILES)
def test_world_sequences_hold_the_orders_in_which_a_prior_goes_stale(oracle, profile, seed):
    f = world_facts(profile, seed, oracle)
    few = {k: f["count"].get(k, 0) for k in cs.kinds_of(profile) if f["count"].get(k, 0) < 3}
    assert not few, few
    assert f["refusals"] == set(cs.WORLD_REFUSALS), sorted(set(cs.WORLD_REFUSALS) - f["refusals"])
    assert f["extents"] >= 2, "fewer than two grow or slide calls change a prior's extents"
    assert f["origin"] >= 1, "no grow or slide call moves a prior's origin"
    assert f["cut_lo"] >= 1, "no slide is trimmed with a non-zero cut_lo"
    assert f["untrimmed"] >= 1, "no over_limit slide is left untrimmed"
    assert f["not_kept"] >= 1, "no refresh with the slot's last job is expected kept == False (only the prior changed)"
    assert f["kept"] >= 1, "no refresh with the slot's last job is expected kept == True after an absorb that changed cells elsewhere"
    # (replan_slots on a handle with several contexts is a plain batch, every flag 0 -- fxjps.h -- so there the order is
    # asserted -- an equal replan straight after a prior-writing op -- and the flags only on one context)
    assert f["replans_after_a_fold"] >= 2, "fewer than two equal replan_slots follow a prior-writing op with no slot write in between"
    assert contexts_of(profile) > 1 or f["reused"] >= 2, "fewer than two such replans are expected all-reused"
    assert "world_cleared_prior" in f["refusals"], "no world job names a prior after its clear_prior_map"
    assert f["stale_origin"] >= 1, "no world job carries the upload's origin after a grow moved it"
    assert f["tiles_refresh"] >= 1, "no world refresh under the tile rule whose changed cells come from the prior"
    assert 5 * f["refused"] <= f["steps"], (f["refused"], f["steps"])


@pytest.mark.parametrize("profile", WORLD_PROFILES)
def test_check_paths_slots_meets_every_verdict(oracle, profile):
    seen, statuses = set(), set()
    for seed in SEEDS:
        f = world_facts(profile, seed, oracle)
        seen |= f["verdicts"]
        statuses |= f["statuses"]
    assert set(VERDICTS.values()) <= seen, "verdicts never expected: %r" % sorted(k for k, v in VERDICTS.items() if v not in seen)
    assert {0, 1, E_ARG} <= statuses, "cropped job outcomes never expected: %r" % sorted({0, 1, E_ARG} - statuses)


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
@pytest.mark.parametrize("broken", BROKEN + WORLD_BROKEN)
def test_a_twin_without_one_invalidation_rule_fails(oracle, broken):
    profiles = ("tiles",) if broken == "mode_change_keeps_slot_results" else WORLD_PROFILES if broken in WORLD_BROKEN else ("single", "tiles")
    for profile in profiles:
        for seed in SEEDS:
            try:
                run_twin(oracle, profile, seed, broken=(broken,))
            except cs.Mismatch as mm:
                assert mm.assertion, "the twin crashed instead of answering wrongly: %s" % str(mm)[:400]
                return
    raise AssertionError("a twin with %r passes every sequence: the generator never builds the order this rule is for" % broken)
