"""GPU suite (-m gpu): the search at 13-bit coordinates and on both sides of the table choice.

The kernel packs a cell into fixed bit fields (x << 17 | y << 4 | dir, cell = x << 13 | y, a path cell x << 16 | y), and on
cell-indexed ("direct") visited tables a node's slot is (cell >> 13) << direct_ly | (cell & 0x1FFF), derived again at every
tier of the open list.  The library takes grids of 1..8190 cells a side and the direct layout whenever
ceil_log2(W) + ceil_log2(H) <= 20 (ensure_pool), so 8190 x 128 and 128 x 8190 are direct grids with a
13-bit coordinate.  What is planned here, against the oracle (offsets, cells, float64 cost bytes, status; per-query pops; the
batch's pops and pushes by pops_gpu == pops_ref, pushes_gpu == pushes_ref - 1 with retried == 0; timing()["table_direct"]
against the host formula restated in fits()):

  long x / long y           8190 x 16 and 16 x 8190 at 5 %: a 13-bit x with direct_ly 4, a 13-bit y with direct_ly 13
  table edge x / y          8190 x 128 and 128 x 8190 at 10 %: 20 bits, the largest direct table, the far tier in use
  one wide                  8190 x 1 and 1 x 8190, empty and at 0.1 %: a single line, occupied starts, goals cut off
  choice                    2048 x 512 (20 bits, direct), 2049 x 512 and 1024 x 1025 (21 bits: hashed by x, by y) at 20 %
  limits                    on long x / long y: starts and goals at W, H and W - 1, H - 1
  hashed twin               long x, long y, one wide under FXJPS_DIRECT=0 in a child of its own
  slots, direct by union    2048 x 8, 8 x 512, 64 x 64: 11 bits from one slot, direct_ly 9 from another
  slots, hashed by union    long x and long y in one batch (26 bits), then long x alone on the same handle (direct again)
  tracked                   set_queries + replan_frame on long x / long y, read sets against the cells the reference reads;
                            replan_slots under the tile rule, twice (searched, then handed back)
  one query                 (0, 0) -> (W - 1, H - 1) through Planner.plan_one and jps1.method (no FXJPS_QSTAT: in-process)

Queries per grid: half from free cells within W/16 x H/16 of one corner to free cells within that of the opposite corner,
every second one reversed, half from synth.synth_queries.  The conditions the shapes were chosen by (check_conditions) are
asserted from the reference alone before the GPU is asked, and on the CPU by test_search_extents_host.py.

The helpers are those of test_search_work_gpu.py; FXJPS_QSTAT=1 switches the single-call path off for a whole process,
hence the children: one per table mode, and the five grids at the table choice in a third, because their references take
as long as everything else here together.  Table edge runs 16 queries a grid and choice 24 (32 and 48 made the direct
child an 8.4 s test); no shape was cut.

Measured on an MI355X (wall time of each pytest call, the oracle's references and the child's start included):
  test_both_sides_of_the_table_choice                 4.3 s  (the reference alone 1.0 s; 0.1 - 0.5 s per scenario and heuristic)
  test_cell_indexed_tables_up_to_13_bit_coordinates   3.6 s  (the reference alone 0.7 s; the read-set check 0.3 s a grid)
  test_hashed_twin                                    1.2 s
  test_one_query_path_at_the_far_corner               0.6 s
  the file                                           10.0 s
Nothing differed: every scenario met the identity with retried == 0 and the table kind the formula names.
"""
import contextlib
import io
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import test_search_work_gpu as work
from test_search_work_gpu import TIERS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPL = 4096          # the longest reference path here (8190 x 128) has 2138 jump points
GRID_SEED, QSEED = 31, 7
NTHREADS = 16
HALF = 4096         # a coordinate from here on needs the 13th bit

# name -> (W, H, p, queries)
GRIDS = {
    "long x": (8190, 16, 0.05, 96),
    "long y": (16, 8190, 0.05, 96),
    "table edge x": (8190, 128, 0.10, 16),
    "table edge y": (128, 8190, 0.10, 16),
    "one wide x, empty": (8190, 1, 0.0, 96),
    "one wide y, empty": (1, 8190, 0.0, 96),
    "one wide x": (8190, 1, 0.001, 96),
    "one wide y": (1, 8190, 0.001, 96),
    "choice 2048x512": (2048, 512, 0.20, 24),
    "choice 2049x512": (2049, 512, 0.20, 24),
    "choice 1024x1025": (1024, 1025, 0.20, 24),
}
LONG = ("long x", "long y")
EDGE = ("table edge x", "table edge y")
WIDE = ("one wide x, empty", "one wide y, empty", "one wide x", "one wide y")
CHOICE = ("choice 2048x512", "choice 2049x512", "choice 1024x1025")
UNION_SLOTS = {0: (2048, 8), 1: (8, 512), 2: (64, 64)}  # at 5 %, 64 queries each
N_OCCUPIED_STARTS = 12
MIN_FAR, MIN_CLASS = 8, 10


def fits(W, H):
    """The host's table choice (ensure_pool), restated: cell-indexed tables iff the rounded-up extents take 20 bits or fewer."""
    return (W - 1).bit_length() + (H - 1).bit_length() <= 20


def slots_fit(shapes):
    """A slots batch is configured for the largest W and the largest H of the slots it names."""
    return fits(max(w for w, _ in shapes), max(h for _, h in shapes))


# ------------------------------------------------------------------ inputs
def grid(name):
    from fuxi_planner_amd import synth
    W, H, p, _ = GRIDS[name]
    return synth.synth_grid(W, H, GRID_SEED, p)


def queries(occ, n, qseed=QSEED):
    """n queries: the first half between opposite corner boxes of W/16 x H/16 cells (every second one reversed), the rest
    from synth.synth_queries."""
    from fuxi_planner_amd import synth
    W, H = occ.shape
    s, g = synth.synth_queries(occ, qseed, n)
    bw, bh = max(W // 16, 1), max(H // 16, 1)
    rng = np.random.default_rng(5)
    lo = np.argwhere(occ[:bw, :bh] == 0)
    hi = np.argwhere(occ[W - bw:, H - bh:] == 0) + [W - bw, H - bh]
    k = n // 2
    a = lo[rng.integers(0, len(lo), k)].astype(np.int32)
    b = hi[rng.integers(0, len(hi), k)].astype(np.int32)
    a[1::2], b[1::2] = b[1::2].copy(), a[1::2].copy()
    s[:k], g[:k] = a, b
    return s, g


def limit_queries(W, H):
    """Starts and goals at the limits of a W x H grid: two starts off the grid, three goals off it, start == goal in the
    last cell, and the first cell to the last."""
    s = np.array([[W, 0], [0, H], [0, 0], [0, 0], [0, 0], [W - 1, H - 1], [0, 0]], dtype=np.int32)
    g = np.array([[W - 1, H - 1], [W - 1, H - 1], [W, 0], [0, H], [W - 1, H], [W - 1, H - 1], [W - 1, H - 1]], dtype=np.int32)
    return s, g


def limit_status(ref_len):
    """What the seven limit queries must report, whatever the grid: -> None, or what is wrong."""
    from fuxi_planner_amd import _lib
    st = [int(v) for v in ref_len]
    if st[:2] != [_lib.Q_BAD_START] * 2 or st[2:5] != [0, 0, 0] or st[5] != 1:
        return "limit queries report %s" % st
    return None


def register_inputs():
    """Every batch of this file under a name of its own in test_search_work_gpu's table of inputs."""
    if "extents long x" in work._inputs:
        return
    for name, (W, H, p, n) in GRIDS.items():
        occ = grid(name)
        s, g = queries(occ, n)
        if name in WIDE and p > 0:  # (occupied starts: searched like any other)
            full = np.argwhere(occ != 0)
            s[n - N_OCCUPIED_STARTS:] = full[np.arange(N_OCCUPIED_STARTS) % len(full)]
        work._inputs["extents " + name] = (occ, s, g)
    for name in LONG:
        occ = work._inputs["extents " + name][0]
        work._inputs["extents %s limits" % name] = (occ,) + limit_queries(*occ.shape)
    from fuxi_planner_amd import synth
    union = {k: synth.synth_grid(W, H, GRID_SEED + 1 + k, 0.05) for k, (W, H) in UNION_SLOTS.items()}
    work._inputs["extents union slots"] = slots_batch({k: (occ,) + queries(occ, 64, QSEED + 1 + k) for k, occ in union.items()}, 11)
    work._inputs["extents long slots"] = slots_batch({k: work._inputs["extents " + name] for k, name in enumerate(LONG)}, 12)
    tracked = {k: (occ,) + queries(occ, 64, QSEED + 1 + k) for k, occ in union.items()}
    tracked[3] = work._inputs["extents long x"]
    work._inputs["extents tracked slots"] = slots_batch(tracked, 13)
    # (beside the batch above, which the union of 8190 and 512 makes a hashed one: two that record read sets on cell-indexed
    # tables, one with the union slots alone, one with the 13-bit x in -- 8190 x 16, 2048 x 8 and 64 x 64 take 13 + 6 bits)
    work._inputs["extents tracked union slots"] = slots_batch({k: tracked[k] for k in (0, 1, 2)}, 14)
    work._inputs["extents tracked long-x slots"] = slots_batch({0: tracked[0], 2: tracked[2], 3: tracked[3]}, 15)


def slots_batch(per_slot, seed):
    """{slot: (occ, starts, goals)} -> ({slot: occ}, ids, starts, goals), shuffled."""
    ids = np.concatenate([np.full(len(v[1]), k, np.int32) for k, v in per_slot.items()])
    s = np.concatenate([v[1] for v in per_slot.values()]).astype(np.int32)
    g = np.concatenate([v[2] for v in per_slot.values()]).astype(np.int32)
    perm = np.random.default_rng(seed).permutation(len(ids))
    return {k: v[0] for k, v in per_slot.items()}, ids[perm], s[perm], g[perm]


SLOT_INPUTS = ("extents union slots", "extents long slots", "extents tracked slots", "extents tracked union slots", "extents tracked long-x slots")


def slot_shapes(inp):
    return [occ.shape for occ in work.inputs(inp)[0].values()]


# ------------------------------------------------------------------ the reference
_labels = {}


def reference(oracle, occ, s, g, h):
    """test_search_work_gpu.reference with the oracle's own flood fill (a million cells) and 16 threads."""
    key = (occ.shape, occ.tobytes())
    if key not in _labels:
        _labels[key] = oracle.components(occ)
    oc, ol, ocost, st = oracle.plan_batch(occ, s, g, h, literal=False, max_len=MPL, nthreads=NTHREADS, want_stats=True)
    keep = np.arange(MPL)[None, :] < np.maximum(ol, 0)[:, None]
    off = np.zeros(len(ol) + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.maximum(ol, 0))
    m = work.searched(occ, s, g, _labels[key])
    return {"csr": (off, oc[keep].reshape(-1, 2), ocost, ol), "searched": m, "ref_pops": st["pops"].copy(), "ref_pushes": st["pushes"].copy(),
            "peak": st["open_peak"].copy(), "pops": np.where(m, st["pops"], 0), "pushes": np.where(m, st["pushes"] - 1, 0)}


FIELDS = ("searched", "ref_pops", "ref_pushes", "peak", "pops", "pushes")


def expected(oracle, inp, h):
    """The reference of the inputs `inp` under heuristic `h`, once per process, where test_search_work_gpu keeps its own."""
    register_inputs()
    key = (inp, h, MPL)
    if key not in work._refs:
        v = work.inputs(inp)
        if len(v) == 4:  # a slots batch: every slot's part on that slot's grid
            grids, ids, s, g = v
            parts = {int(k): (np.flatnonzero(ids == k), reference(oracle, grids[int(k)], s[ids == k], g[ids == k], h)) for k in np.unique(ids)}
            r = {f: np.zeros(len(ids), dtype=bool if f == "searched" else np.int64) for f in FIELDS}
            for idx, p in parts.values():
                for f in FIELDS:
                    r[f][idx] = p[f]
            r["parts"] = parts
            work._refs[key] = r
        else:
            work._refs[key] = reference(oracle, *v, h)
    return work._refs[key]


def through_half(ref, axis):
    """Per query: does the reference's path hold a jump point whose coordinate `axis` is 4096 or more?"""
    off, cells = ref["csr"][0], ref["csr"][1]
    return np.array([bool((cells[off[q]:off[q + 1], axis] >= HALF).any()) for q in range(len(off) - 1)])


def check_conditions(oracle, names=None):
    """What the shapes and queries were chosen by, from the reference alone, for both heuristics.  -> the figures."""
    register_inputs()
    fig = {}
    plain = [n for n in LONG + EDGE + CHOICE if names is None or n in names]
    for name in plain + [n for n in SLOT_INPUTS if names is None or n in names]:
        inp = name if name in SLOT_INPUTS else "extents " + name
        for h in (2, 1):
            ref = expected(oracle, inp, h)
            m, ln = ref["searched"], (np.concatenate([p["csr"][3] for _, p in ref["parts"].values()]) if "parts" in ref else ref["csr"][3])
            fig[name, h] = {"queries": len(m), "searched": int(m.sum()), "longest": int(ln.max()), "peak": int(ref["peak"].max()),
                            "far": int((ref["peak"][m] > TIERS).sum())}
            assert m.sum() >= 0.95 * len(m), (name, h, int(m.sum()), len(m))
            assert (ln >= 0).all() and ln.max() < MPL, (name, h, int(ln.min()), int(ln.max()))
            if name in LONG + EDGE:
                n_half = int(through_half(ref, 0 if name.endswith("x") else 1).sum())
                fig[name, h]["through 4096"] = n_half
                assert n_half >= 0.40 * len(m), (name, h, n_half, len(m))
            if name in EDGE and h == 1:
                assert fig[name, h]["far"] >= MIN_FAR, (name, fig[name, h])
    for name in WIDE:
        if names is not None and name not in names:
            continue
        occ, s, g = work.inputs("extents " + name)
        cls = work.edge_classes(occ, s, g, _labels.get((occ.shape, occ.tobytes())))
        for h in (2, 1):
            m = expected(oracle, "extents " + name, h)["searched"]
            fig[name, h] = {"queries": len(m), "searched": int(m.sum()), "occupied start": int(cls["occupied start"].sum()),
                            "goal in another component": int(cls["goal in another component"].sum())}
            if GRIDS[name][2] == 0:
                assert m.all(), name
            else:
                assert cls["occupied start"].sum() >= MIN_CLASS and cls["goal in another component"].sum() >= MIN_CLASS, (name, fig[name, h])
                assert (m & cls["occupied start"]).sum() >= MIN_CLASS, name
    for name in LONG:
        if names is None or name in names:
            for h in (2, 1):
                ref = expected(oracle, "extents %s limits" % name, h)
                assert limit_status(ref["csr"][3]) is None and not ref["searched"][:6].any(), (name, ref["csr"][3])
    return fig


# ------------------------------------------------------------------ the child processes (FXJPS_QSTAT=1)
def work_line(p, name, h, res, ref, n, want_direct, parts=None, qstat=True):
    """The checks of test_search_work_gpu.run_scenario on a call already made: -> (line, what is wrong)."""
    from test_grid_slots_gpu import subset
    bad = []
    if parts is None:
        d = work.same_bytes(res[:4], ref["csr"])
        if d:
            bad.append("%s differ from the oracle's" % d)
    else:
        for k, (idx, part) in parts.items():
            d = work.same_bytes(subset(res[:4], idx), part["csr"])
            if d:
                bad.append("slot %d: %s differ from the oracle's" % (k, d))
    t = p.timing()
    m = ref["searched"]
    want_pops, want_pushes = int(ref["pops"].sum()), int(ref["pushes"].sum())
    ndiff = -1
    if qstat:
        q = p.debug_qstat(n)[:, 2].astype(np.int64)
        diff = np.flatnonzero(q != ref["pops"])
        ndiff = len(diff)
        if ndiff:
            bad.append("per-query pops: %d of %d differ, first: %s" % (ndiff, n, [(int(i), "gpu %d" % q[i], "reference %d" % ref["pops"][i]) for i in diff[:6]]))
    line = ("%s h=%d: %d queries, %d searched, far tier %d | pops %d (reference %d), pushes %d (reference %d - %d), per-query pops differ on %d, "
            "retried %d, launches %d, table_direct %d" % (name, h, n, int(m.sum()), int((ref["peak"][m] > TIERS).sum()), t["pops"], want_pops, t["pushes"],
                                                         int(ref["ref_pushes"][m].sum()), int(m.sum()), ndiff, t["retried"], t["search_launches"],
                                                         t["table_direct"]))
    if t["retried"] != 0:
        bad.append("%d queries were retried: the batch's sums are not exact" % t["retried"])
    if (t["pops"], t["pushes"]) != (want_pops, want_pushes):
        bad.append("batch sums: pops %d pushes %d, expected %d and %d" % (t["pops"], t["pushes"], want_pops, want_pushes))
    if t["table_direct"] != int(want_direct):
        bad.append("table_direct %d, the host formula says %d" % (t["table_direct"], int(want_direct)))
    return line, bad


class Report(object):
    def __init__(self):
        self.failed = 0

    def __call__(self, line, bad, t0):
        print(("work ok  " if not bad else "work BAD ") + line + " [%.2f s]" % (time.time() - t0), flush=True)
        for b in bad:
            print("    " + b, flush=True)
        self.failed += bool(bad)


# (test_search_work_gpu's scenario records: name, inputs, kind, environment, heuristics, far tier, retries, path slot)
MODES = ("direct", "edge", "hashed")  # the children: "edge" is the direct child's table edge and choice grids, in a process of their own


def scenarios(mode):
    hashed = mode == "hashed"
    env = {"FXJPS_DIRECT": "0"} if hashed else {}
    if mode == "edge":
        return [(name, "extents " + name, "batch", env, (2, 1), False, False, MPL) for name in EDGE + CHOICE]
    sc = [(("hashed " if hashed else "") + name, "extents " + name, "batch", env, (2, 1), False, False, MPL) for name in LONG]
    if not hashed:
        sc.append(("union slots", "extents union slots", "slots", env, (2, 1), False, False, MPL))
    return sc


def custom_names(mode):
    """The lines the child prints beside those of scenarios()."""
    if mode == "edge":
        return []
    names = [("hashed " if mode == "hashed" else "") + n for n in WIDE]
    if mode == "direct":
        names += ["%s limits" % n for n in LONG] + ["tracked %s" % n for n in LONG]
        names += ["long slots", "long slots, then long x alone"]
        names += [n[len("extents "):] for n in SLOT_INPUTS[2:]] + [n[len("extents "):] + ", again" for n in SLOT_INPUTS[2:]]
    return names


def want_direct(inp, hashed):
    if hashed:
        return False
    v = work.inputs(inp)
    return slots_fit(slot_shapes(inp)) if len(v) == 4 else fits(*v[0].shape)


def child_main(mode):
    """One process under FXJPS_QSTAT=1 (and FXJPS_DIRECT=0 for the hashed twin).  One line per scenario and heuristic."""
    hashed = mode == "hashed"
    assert mode in MODES and os.environ.get("FXJPS_QSTAT") == "1" and (os.environ.get("FXJPS_DIRECT") == "0") == hashed
    import fuxi_planner_amd as fx
    from oracle import oracle
    oracle.build()
    t0 = time.time()
    check_conditions(oracle, {"direct": LONG + WIDE + SLOT_INPUTS, "edge": EDGE + CHOICE, "hashed": LONG + WIDE}[mode])
    print("conditions: the reference alone, %.2f s" % (time.time() - t0), flush=True)
    report = Report()
    for sc in scenarios(mode):
        for h in sc[4]:
            t0 = time.time()
            expected(oracle, sc[1], h)
            line, bad = work.run_scenario(fx, oracle, sc, h)
            if "table_direct %d" % int(want_direct(sc[1], hashed)) not in line:
                bad.append("the host formula says table_direct %d" % int(want_direct(sc[1], hashed)))
            report(line, bad, t0)
    tag = "hashed " if hashed else ""
    for h in (2, 1) if mode != "edge" else ():
        # ---- single lines, and the queries at the limits: most of them are answered without a search
        for name in WIDE + (() if hashed else tuple("%s limits" % n for n in LONG)):
            t0 = time.time()
            inp = "extents " + name
            occ, s, g = work.inputs(inp)
            ref = expected(oracle, inp, h)
            with fx.Planner([0]) as p:
                p.set_grid_occ(occ)
                res = p.plan_batch(s, g, h, MPL)
                line, bad = work_line(p, tag + name, h, res, ref, len(s), want_direct(inp, hashed))
            if name.endswith("limits") and limit_status(res[3]):
                bad.append(limit_status(res[3]))
            report(line, bad, t0)
        if hashed:
            continue
        # ---- the read sets of the tracking searches at tile shift 7
        from oracle import read_sets as rs
        from test_read_sets_gpu import check_cover
        for name in LONG:
            t0 = time.time()
            inp = "extents " + name
            occ, s, g = work.inputs(inp)
            ref = expected(oracle, inp, h)
            bad = []
            with fx.Planner([0]) as p:
                p.set_grid_occ(occ)
                p.set_queries(s, g, h, MPL)
                res = p.replan_frame()
                line, bad = work_line(p, "tracked " + name, h, res, ref, len(s), True)
                if p.timing()["reused"] != 0 or rs.tile_shift(*occ.shape) != 7:
                    bad.append("reused %d, tile shift %d" % (p.timing()["reused"], rs.tile_shift(*occ.shape)))
                try:
                    check_cover(p, oracle, occ, s, g, h, res, name)
                except AssertionError as e:
                    bad.append("read sets do not cover the reference's reads: %s" % str(e)[:1500])
            report(line, bad, t0)
        # ---- slots, hashed by union: long x and long y in one batch, then long x alone on the same handle
        t0 = time.time()
        inp = "extents long slots"
        grids, ids, s, g = work.inputs(inp)
        ref = expected(oracle, inp, h)
        with fx.Planner([0]) as p:
            for k, occ in grids.items():
                p.set_grid_slot(k, occ)
            res = p.plan_batch_slots(ids, s, g, h, MPL)
            line, bad = work_line(p, "long slots", h, res, ref, len(s), False, ref["parts"])
            report(line, bad, t0)
            t0 = time.time()
            idx, part = ref["parts"][0]
            res = p.plan_batch_slots(ids[idx], s[idx], g[idx], h, MPL)
            line, bad = work_line(p, "long slots, then long x alone", h, res, part, len(idx), True)
            report(line, bad, t0)
        # ---- slots that record read sets (the tile rule): searched, then handed back
        for inp in SLOT_INPUTS[2:]:
            t0 = time.time()
            grids, ids, s, g = work.inputs(inp)
            ref = expected(oracle, inp, h)
            with fx.Planner([0]) as p:
                p.set_slot_reuse("tiles")
                for k, occ in grids.items():
                    p.set_grid_slot(k, occ)
                first = p.replan_slots(ids, s, g, h, MPL)
                line, bad = work_line(p, inp[len("extents "):], h, first, ref, len(s), want_direct(inp, False), ref["parts"])
                if first[4].any() or p.timing()["reused"] != 0:
                    bad.append("the first call hands back %d stored results" % int((first[4] != 0).sum()))
                report(line, bad, t0)
                t0 = time.time()
                again = p.replan_slots(ids, s, g, h, MPL)
                t = p.timing()
                bad = []
                if not (again[4] == 1).all() or t["reused"] != len(s):
                    bad.append("the second call reports reused %s, timing %d" % (np.bincount(again[4].astype(np.int64), minlength=3).tolist(), t["reused"]))
                d = work.same_bytes(again[:4], first[:4])
                if d:
                    bad.append("%s differ from the first call's" % d)
                if (t["pops"], t["pushes"]) != (0, 0):
                    bad.append("pops %d, pushes %d in a call that searched nothing" % (t["pops"], t["pushes"]))
                report("%s, again h=%d: %d queries, %d handed back" % (inp[len("extents "):], h, len(s), int((again[4] == 1).sum())), bad, t0)
    if report.failed:
        sys.exit("%d checks failed" % report.failed)


def run_child(mode):
    env = dict(os.environ, FXJPS_QSTAT="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    env.pop("FXJPS_DIRECT", None)
    if mode == "hashed":
        env["FXJPS_DIRECT"] = "0"
    r = subprocess.run([sys.executable, "-c", "import test_search_extents_gpu as t; t.child_main(%r)" % mode], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout[-8000:], r.stderr[-4000:])
    for sc in scenarios(mode):
        for h in sc[4]:
            assert "work ok  %s h=%d:" % (sc[0], h) in r.stdout, (sc[0], h, r.stdout[-8000:])
    for name in custom_names(mode):
        for h in (2, 1):
            assert "work ok  %s h=%d:" % (name, h) in r.stdout, (name, h, r.stdout[-8000:])


def test_cell_indexed_tables_up_to_13_bit_coordinates():
    """Long x, long y, the single lines, the limits, the slots batches and the tracking kernels, in one child process."""
    run_child("direct")


def test_both_sides_of_the_table_choice():
    """8190 x 128 and 128 x 8190 (the largest direct tables), 2048 x 512 beside 2049 x 512 and 1024 x 1025, in a child of
    their own: the reference of these five grids takes as long as everything else in this file together."""
    run_child("edge")


def test_hashed_twin():
    """FXJPS_DIRECT=0 in a child process: long x, long y and the four single lines on hashed tables, the same reference."""
    run_child("hashed")


def test_one_query_path_at_the_far_corner(oracle):
    """(0, 0) -> (W - 1, H - 1) on long x and long y through Planner.plan_one -- the single-call path, where start and goal
    travel as kernel arguments -- and once through jps1.method on the float64 matrix: the printed cost is the oracle's."""
    assert "FXJPS_QSTAT" not in os.environ and os.environ.get("FXJPS_SINGLE", "1") != "0"
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import jps1
    register_inputs()
    with fx.Planner([0]) as p:
        for name in LONG:
            occ = work.inputs("extents " + name)[0]
            W, H = occ.shape
            s, g = (0, 0), (W - 1, H - 1)
            p.set_grid_occ(occ)
            for h in (2, 1):
                want, cost, stats = oracle.plan(occ, s, g, h, literal=False)
                st, c, cells = p.plan_one(s, g, h)
                t = p.timing()
                assert t["waves"] == 1 and t["search_launches"] == 1 and t["table_direct"] == 1, (name, h, t)
                assert st == (len(want) if want else 0) and [tuple(v) for v in np.asarray(cells).tolist()] == (want or []), (name, h, st)
                assert np.float64(c).tobytes() == np.float64(cost).tobytes(), (name, h, c, cost)
                if work.searched(occ, [s], [g], oracle.components(occ))[0]:
                    assert (t["pops"], t["pushes"]) == (stats["pops"], stats["pushes"] - 1), (name, h, t["pops"], t["pushes"], stats)
                with contextlib.redirect_stdout(io.StringIO()) as buf:
                    r = jps1.method(occ.astype(np.float64), s, g, h)
                if want:
                    assert r[0] == want and buf.getvalue().strip() == repr(cost), (name, h, buf.getvalue(), cost)
                else:
                    assert r[0] is 0 and buf.getvalue() == ""  # noqa: F632
