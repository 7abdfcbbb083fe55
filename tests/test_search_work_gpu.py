"""GPU suite (-m gpu): how much WORK the search kernel does -- its open-list pops and pushes -- against the reference's.

Every other GPU test of the search compares what comes out (cells, lengths, float64 cost).  An open-list entry lost in a
refill, handed out twice, or a relaxation committed in the wrong order among equal keys seldom changes a path, but always
changes the number of pops or pushes.  The kernel counts both per query (`search_one`), the oracle counts the reference's
(oracle/jps_oracle.c, pinned to the counts of the real jps1.py by test_oracle_golden.py).

The identity.  On a grid freshly uploaded (component labels flat) a query is SEARCHED iff
  * its start is inside the grid,
  * start != goal,
  * its goal is inside the grid and free,
  * its start is occupied, or start and goal lie in the same 4-connected component of free cells
(`run_query` answers every other query without a search).  `searched()` below computes this from the grid alone, with a
flood fill of its own.  Then, exactly:
  * a searched query:    pops_gpu == pops_ref   and   pushes_gpu == pushes_ref - 1
    (the start goes straight into the register tier and is not counted; the reference's push of jps1.py:192 is),
  * every other query:   pops_gpu == 0, and it adds nothing to the batch's pushes.
A result of -1 (a path longer than its slot) and an occupied start are searched queries like any other.  pops_gpu of
query q is qstat[q, 2] (FXJPS_QSTAT=1), the batch's sums are fxjps_timing_t::pops / ::pushes.  A query that is run
again on the large pool starts over: its qstat row is the final attempt's, the batch's sums hold the abandoned attempts
as well (>= there, == wherever nothing was retried).

Confirmed on an MI355X for every scenario below, the `- 1` on pushes included: see `test_counts_per_query` (one child
process, because FXJPS_QSTAT switches the single-call path off for the whole process) and the in-process tests behind it.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import grid_from_bits, load_golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPL = 1024
NTHREADS = 8
TIERS = 320  # the 64 register entries plus the 256 LDS entries of the open list: a larger open list is in the far tier


# ------------------------------------------------------------------ the host side: predicate, reference counts, inputs
def components(occ):
    """4-connected components of the free cells by a flood fill: int32[W, H], a label per component, -1 on occupied cells."""
    W, H = occ.shape
    PH = H + 2
    pad = np.ones((W + 2, PH), dtype=np.uint8)  # (a border of occupied cells: no bounds tests in the loop)
    pad[1:-1, 1:-1] = occ != 0
    flat = pad.reshape(-1)
    done = bytearray(flat.tobytes())  # occupied, border or labelled
    lab = np.full(len(done), -1, dtype=np.int32)
    for i0 in np.flatnonzero(flat == 0).tolist():
        if done[i0]:
            continue
        done[i0] = 1
        stack, members = [i0], []
        while stack:
            i = stack.pop()
            members.append(i)
            for j in (i - 1, i + 1, i - PH, i + PH):
                if not done[j]:
                    done[j] = 1
                    stack.append(j)
        lab[members] = i0
    return lab.reshape(W + 2, PH)[1:-1, 1:-1]


def searched(occ, s, g, lab=None):
    """The predicate of the module docstring, from the grid alone: bool[nq]."""
    W, H = occ.shape
    s, g = np.asarray(s, dtype=np.int64).reshape(-1, 2), np.asarray(g, dtype=np.int64).reshape(-1, 2)
    if lab is None:
        lab = components(occ)
    s_in = (s[:, 0] >= 0) & (s[:, 0] < W) & (s[:, 1] >= 0) & (s[:, 1] < H)
    g_in = (g[:, 0] >= 0) & (g[:, 0] < W) & (g[:, 1] >= 0) & (g[:, 1] < H)
    sx, sy = np.clip(s[:, 0], 0, W - 1), np.clip(s[:, 1], 0, H - 1)
    gx, gy = np.clip(g[:, 0], 0, W - 1), np.clip(g[:, 1], 0, H - 1)
    s_occ = occ[sx, sy] != 0
    g_free = g_in & (occ[gx, gy] == 0)
    return s_in & (s != g).any(axis=1) & g_free & (s_occ | (lab[sx, sy] == lab[gx, gy]))


def reference(oracle, occ, s, g, h, mpl=MPL):
    """The oracle's answer in the planner's CSR layout, its counts, and the counts the identity expects of the kernel."""
    oc, ol, ocost, st = oracle.plan_batch(occ, s, g, h, literal=False, max_len=mpl, nthreads=NTHREADS, want_stats=True)
    keep = np.arange(mpl)[None, :] < np.maximum(ol, 0)[:, None]
    off = np.zeros(len(ol) + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.maximum(ol, 0))
    m = searched(occ, s, g)
    return {"csr": (off, oc[keep].reshape(-1, 2), ocost, ol), "searched": m, "ref_pops": st["pops"].copy(), "ref_pushes": st["pushes"].copy(),
            "peak": st["open_peak"].copy(), "pops": np.where(m, st["pops"], 0), "pushes": np.where(m, st["pushes"] - 1, 0)}


def rooms_map():
    """The 193 x 193 rooms-and-doors map of test_gpu_parity.test_structured_maps_vs_oracle, its sealed pocket included."""
    W = H = 193
    occ = np.zeros((W, H), dtype=np.uint8)
    occ[::16, :] = 1
    occ[:, ::16] = 1
    rng = np.random.default_rng(3)
    for k in range(1, 12):  # doors
        for j in range(12):
            occ[16 * k, 16 * j + int(rng.integers(1, 16))] = 0
            occ[16 * j + int(rng.integers(1, 16)), 16 * k] = 0
    occ[100:110, 100:110] = 1
    occ[103:106, 103:106] = 0  # sealed pocket
    return occ


EDGE_CLASSES = ("occupied start", "start == goal", "goal occupied", "goal off the grid", "start off the grid", "goal in another component")


def edge_classes(occ, s, g, lab=None):
    """Which class of the edge batch a query belongs to, from the grid alone: {class name: bool[nq]}."""
    W, H = occ.shape
    s, g = np.asarray(s, dtype=np.int64), np.asarray(g, dtype=np.int64)
    if lab is None:
        lab = components(occ)
    s_in = (s[:, 0] >= 0) & (s[:, 0] < W) & (s[:, 1] >= 0) & (s[:, 1] < H)
    g_in = (g[:, 0] >= 0) & (g[:, 0] < W) & (g[:, 1] >= 0) & (g[:, 1] < H)
    sx, sy = np.clip(s[:, 0], 0, W - 1), np.clip(s[:, 1], 0, H - 1)
    gx, gy = np.clip(g[:, 0], 0, W - 1), np.clip(g[:, 1], 0, H - 1)
    s_free, g_free = s_in & (occ[sx, sy] == 0), g_in & (occ[gx, gy] == 0)
    same = (s == g).all(axis=1)
    return {"occupied start": s_in & ~s_free & g_free,
            "start == goal": s_in & same,
            "goal occupied": s_free & g_in & ~g_free,
            "goal off the grid": s_free & ~g_in,
            "start off the grid": ~s_in,
            "goal in another component": s_free & g_free & (lab[sx, sy] != lab[gx, gy])}


def edge_batch(occ, per_class=40):
    """`per_class` queries of each of EDGE_CLASSES on `occ`, shuffled."""
    W, H = occ.shape
    rng = np.random.default_rng(17)
    lab = components(occ)
    free, full = np.argwhere(occ == 0), np.argwhere(occ != 0)
    ids, counts = np.unique(lab[lab >= 0], return_counts=True)
    main = ids[np.argmax(counts)]
    inside = np.argwhere(lab == main)
    outside = np.argwhere((lab >= 0) & (lab != main))
    assert len(outside) >= 10 and len(full) >= per_class

    def pick(a, n=per_class):
        return a[rng.integers(0, len(a), n)]

    off = np.stack([rng.choice([-1, -7, W, W + 5], per_class), rng.integers(-2, H + 2, per_class)], 1)
    off[::2] = np.stack([rng.integers(-2, W + 2, per_class), rng.choice([-1, -3, H, H + 9], per_class)], 1)[::2]
    S, G = [], []
    S.append(pick(full)), G.append(pick(free))            # occupied start, free goal
    same = np.concatenate([pick(free, per_class - 4), pick(full, 4)])
    S.append(same), G.append(same.copy())                 # start == goal (four of them on an obstacle)
    S.append(pick(free)), G.append(pick(full))            # goal occupied
    S.append(pick(free)), G.append(off)                   # goal off the grid
    S.append(off[::-1].copy()), G.append(pick(free))      # start off the grid
    a, b = pick(inside), pick(outside)                    # goal in another component: into the small ones, and out of them
    a[::2], b[::2] = b[::2].copy(), a[::2].copy()
    S.append(a), G.append(b)
    s, g = np.concatenate(S).astype(np.int32), np.concatenate(G).astype(np.int32)
    perm = rng.permutation(len(s))
    return s[perm], g[perm]


_inputs = {}


def inputs(name):
    """The seeded inputs of the scenarios: name -> (occ, starts, goals), or for "slots" ({slot: occ}, ids, starts, goals)."""
    if name in _inputs:
        return _inputs[name]
    from fuxi_planner_amd import synth
    if name == "small":
        occ = synth.synth_grid(96, 80, 7, 0.25)
        v = (occ,) + synth.synth_queries(occ, 3, 600)
    elif name == "sparse":
        occ = synth.synth_grid(300, 200, 11, 0.02)
        v = (occ,) + synth.synth_queries(occ, 11, 400)
    elif name == "rooms":
        occ = rooms_map()
        rng = np.random.default_rng(4)
        free = np.argwhere(occ == 0)
        s = free[rng.integers(0, len(free), 800)].astype(np.int32)
        g = free[rng.integers(0, len(free), 800)].astype(np.int32)
        g[:20] = [104, 104]   # into the sealed pocket
        s[20:30] = [104, 105]  # out of it
        v = (occ, s, g)
    elif name == "square512":
        occ = synth.synth_grid(512, 512, 5, 0.20)
        v = (occ,) + synth.synth_queries(occ, 5, 600)
    elif name == "tall":
        occ = synth.synth_grid(130, 2100, 3, 0.20)
        v = (occ,) + synth.synth_queries(occ, 12, 300)
    elif name == "head":
        occ = synth.synth_grid(256, 256, 3, 0.20)
        v = (occ,) + synth.synth_queries(occ, 3, 4608)
    elif name == "edge":
        occ = inputs("small")[0]
        v = (occ,) + edge_batch(occ)
    elif name == "slots":
        grids = {0: inputs("small")[0], 1: inputs("sparse")[0], 2: synth.synth_grid(3, 40, 4, 0.10), 3: synth.synth_grid(130, 600, 6, 0.20)}
        nper = {0: 260, 1: 260, 2: 20, 3: 260}
        ids, S, G = [], [], []
        for k, occ in grids.items():
            s, g = synth.synth_queries(occ, 20 + k, nper[k])
            ids.append(np.full(nper[k], k, np.int32))
            S.append(s)
            G.append(g)
        perm = np.random.default_rng(9).permutation(800)
        v = (grids, np.concatenate(ids)[perm], np.concatenate(S)[perm].astype(np.int32), np.concatenate(G)[perm].astype(np.int32))
    else:
        raise KeyError(name)
    _inputs[name] = v
    return v


_refs = {}


def expected(oracle, name, h, mpl=MPL):
    """reference() of the scenario inputs `name` under heuristic `h`, computed once per process."""
    key = (name, h, mpl)
    if key not in _refs:
        if name == "slots":
            grids, ids, s, g = inputs(name)
            parts = {int(k): (np.flatnonzero(ids == k), reference(oracle, grids[int(k)], s[ids == k], g[ids == k], h, mpl)) for k in np.unique(ids)}
            r = {f: np.zeros(len(ids), dtype=bool if f == "searched" else np.int64) for f in ("searched", "ref_pops", "ref_pushes", "peak", "pops", "pushes")}
            for idx, p in parts.values():
                for f in r:
                    r[f][idx] = p[f]
            r["parts"] = parts
            _refs[key] = r
        else:
            occ, s, g = inputs(name)
            _refs[key] = reference(oracle, occ, s, g, h, mpl)
    return _refs[key]


def check_oracle_side(name, ref, edge=False, far=False):
    """What a scenario must be before the GPU is asked: mostly searched queries, open lists that outgrow the two fast
    tiers where the far tier is the point, and more pushes than pops (a wide-open map pops three nodes per query)."""
    m = ref["searched"]
    if edge:
        occ, s, g = inputs(name)
        for c, members in edge_classes(occ, s, g).items():
            assert members.sum() >= 30, (name, c, int(members.sum()))
    else:
        assert m.sum() >= 0.95 * len(m), (name, int(m.sum()), len(m))
    if far:
        assert (ref["peak"][m] > TIERS).sum() >= 50, (name, int((ref["peak"][m] > TIERS).sum()))
    assert (ref["ref_pushes"][m] - ref["ref_pops"][m]).sum() > 0, name
    assert (ref["ref_pops"][m] >= 1).all(), name


# (name, inputs, kind, environment, heuristics, far tier must be used, retries: True there must be some / False there must be
# none, so that the batch's sums are exact / None as it comes, path slot)
SCENARIOS = (
    ("small 96x80", "small", "batch", {}, (2, 1), False, False, MPL),
    ("small 96x80, slot of 3 cells", "small", "batch", {}, (2,), False, False, 3),
    ("sparse 300x200", "sparse", "batch", {}, (2, 1), True, False, MPL),
    ("rooms 193x193", "rooms", "batch", {}, (2, 1), False, False, MPL),
    ("square 512x512", "square512", "batch", {}, (2, 1), True, False, MPL),
    ("tall 130x2100", "tall", "batch", {}, (2,), True, False, MPL),
    ("edge batch 96x80", "edge", "batch", {}, (2, 1), False, False, MPL),
    ("head launch 256x256", "head", "head", {}, (2, 1), True, False, MPL),
    ("slots", "slots", "slots", {}, (2, 1), False, False, MPL),
    ("tracked small 96x80", "small", "replan", {}, (2, 1), False, False, MPL),
    ("tracked sparse 300x200", "sparse", "replan", {}, (2, 1), True, False, MPL),
    ("hashed small 96x80", "small", "batch", {"FXJPS_DIRECT": "0"}, (2, 1), False, False, MPL),
    ("hashed sparse 300x200", "sparse", "batch", {"FXJPS_DIRECT": "0"}, (2, 1), True, False, MPL),
    ("hashed tall 130x2100", "tall", "batch", {"FXJPS_DIRECT": "0"}, (2,), True, False, MPL),
    ("hashed slots", "slots", "slots", {"FXJPS_DIRECT": "0"}, (2, 1), False, False, MPL),
    ("hashed tracked small 96x80", "small", "replan", {"FXJPS_DIRECT": "0"}, (2,), False, False, MPL),
    ("banded 512x512", "square512", "batch", {"FXJPS_DIRECT": "0", "FXJPS_BANDED": "1"}, (2,), True, None, MPL),
    ("banded 512x512, near band of 32", "square512", "batch", {"FXJPS_DIRECT": "0", "FXJPS_BANDED": "1", "FXJPS_NEAR_MAX": "32"}, (2,), True, None, MPL),
    ("banded 512x512, far tier of 131072", "square512", "batch", {"FXJPS_DIRECT": "0", "FXJPS_BANDED": "1", "FXJPS_FAR_CAP": "131072"}, (2,), True, False, MPL),
    ("retry sparse 300x200, far tier of 64", "sparse", "batch", {"FXJPS_FAR_CAP": "64"}, (2, 1), True, True, MPL),
    ("retry sparse 300x200, table of 256", "sparse", "batch", {"FXJPS_TABLE_LOG2": "8"}, (2, 1), True, True, MPL),
)


def scenario_names():
    return ["%s h=%d" % (sc[0], h) for sc in SCENARIOS for h in sc[4]]


# ------------------------------------------------------------------ the child process (FXJPS_QSTAT=1)
def same_bytes(a, b):
    """Cells, lengths and float64 cost bit for bit: -> None, or what differs."""
    for what, x, y in zip(("offsets", "cells", "cost", "status"), a, b):
        if np.asarray(x).tobytes() != np.asarray(y).tobytes():
            return what
    return None


def run_scenario(fx, oracle, sc, h):
    """-> (the line to print, the list of what is wrong)."""
    name, inp, kind, env, _, far, retry, mpl = sc
    ref = expected(oracle, inp, h, mpl)
    check_oracle_side(inp, ref, edge=inp == "edge", far=far)  # before the GPU is asked
    bad = []
    with fx.Planner([0]) as p:
        t0 = p.timing()["solo_timeouts"]
        if kind == "slots":
            grids, ids, s, g = inputs(inp)
            for k, occ in grids.items():
                p.set_grid_slot(k, occ)
            res = p.plan_batch_slots(ids, s, g, h, mpl)
            for k, (idx, part) in ref["parts"].items():
                from test_grid_slots_gpu import subset
                d = same_bytes(subset(res, idx), part["csr"])
                if d:
                    bad.append("slot %d: %s differ from the oracle's" % (k, d))
        else:
            occ, s, g = inputs(inp)
            p.set_grid_occ(occ)
            if kind == "replan":
                p.set_queries(s, g, h, mpl)
                res = p.replan_frame()
            else:
                res = p.plan_batch(s, g, h, mpl)
            d = same_bytes(res, ref["csr"])
            if d:
                bad.append("%s differ from the oracle's" % d)
        t = p.timing()
        q = p.debug_qstat(len(s))[:, 2].astype(np.int64)
    want_pops, want_pushes = int(ref["pops"].sum()), int(ref["pushes"].sum())
    line = ("%s h=%d: %d queries, %d searched, far tier %d | pops %d (reference %d), pushes %d (reference %d - %d), per-query pops differ on %d, "
            "retried %d, launches %d, table_direct %d" % (name, h, len(s), int(ref["searched"].sum()), int((ref["peak"][ref["searched"]] > TIERS).sum()),
                                                         t["pops"], want_pops, t["pushes"], int(ref["ref_pushes"][ref["searched"]].sum()),
                                                         int(ref["searched"].sum()), int((q != ref["pops"]).sum()), t["retried"],
                                                         t["search_launches"], t["table_direct"]))
    diff = np.flatnonzero(q != ref["pops"])
    if len(diff):
        bad.append("per-query pops: %d of %d differ, first: %s" % (len(diff), len(q), [
            (int(i), s[i].tolist(), g[i].tolist(), "gpu %d" % q[i], "reference %d" % ref["pops"][i], "searched %d" % ref["searched"][i]) for i in diff[:6]]))
    if t["retried"] == 0:
        if (t["pops"], t["pushes"]) != (want_pops, want_pushes):
            bad.append("batch sums: pops %d pushes %d, expected %d and %d" % (t["pops"], t["pushes"], want_pops, want_pushes))
    elif t["pops"] < want_pops or t["pushes"] < want_pushes:  # (the abandoned attempts are in the sums)
        bad.append("batch sums with retries: pops %d pushes %d, expected at least %d and %d" % (t["pops"], t["pushes"], want_pops, want_pushes))
    if retry is True and t["retried"] <= 0:
        bad.append("nothing was retried")
    if retry is False and t["retried"] != 0:
        bad.append("%d queries were retried: the batch's sums are not exact" % t["retried"])
    if env.get("FXJPS_DIRECT") == "0" and t["table_direct"] != 0:
        bad.append("the tables are not hashed")
    if kind == "replan" and t["reused"] != 0:
        bad.append("%d results reused" % t["reused"])
    if kind == "head" and not (t["search_launches"] == 2 or t["solo_timeouts"] > t0):
        bad.append("no head launch: %r" % (t,))
    return line, bad


def child_main(select=None):
    """Every scenario, one after the other, in THIS process (FXJPS_QSTAT=1 is in its environment from the start); one line
    per scenario.  A scenario whose counts differ is reported and the next one runs; an error of the library ends the run.
    `select`: the names (SCENARIOS[i][0]) of the scenarios to run, in the table's order; all of them without it."""
    assert os.environ.get("FXJPS_QSTAT") == "1"
    import fuxi_planner_amd as fx
    from oracle import oracle
    oracle.build()
    knobs = sorted({k for sc in SCENARIOS for k in sc[3]})
    failed = 0
    if select is not None:
        unknown = set(select) - {sc[0] for sc in SCENARIOS}
        assert not unknown, unknown
    for sc in SCENARIOS:
        if select is not None and sc[0] not in select:
            continue
        for k in knobs:
            os.environ.pop(k, None)
        os.environ.update(sc[3])
        for h in sc[4]:
            line, bad = run_scenario(fx, oracle, sc, h)
            print(("work ok  " if not bad else "work BAD ") + line, flush=True)
            for b in bad:
                print("    " + b, flush=True)
            failed += bool(bad)
    if failed:
        sys.exit("%d scenarios failed" % failed)


def test_counts_per_query():
    """Per query and per batch, over every instantiation of k_search, both table kinds, the three tiers, the large-pool
    retry, the head launch, grid slots and the tracking form: the identity of the module docstring, and the usual
    bit-exact comparison of cells and cost beside it."""
    env = dict(os.environ, FXJPS_QSTAT="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-c", "import test_search_work_gpu as t; t.child_main()"], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout[-6000:], r.stderr[-4000:])
    for name in scenario_names():
        assert "work ok  " + name + ":" in r.stdout, (name, r.stdout[-6000:])


# ------------------------------------------------------------------ in this process (no FXJPS_QSTAT)
@pytest.fixture(scope="module")
def planner():
    import fuxi_planner_amd as fx
    p = fx.Planner([0])
    yield p
    p.close()


def golden_records(map_grids):
    """Every record of the three golden files that carry the counts of the real jps1.py, with its grid: (file, grid, rec)."""
    for rec in load_golden("random_small.json"):
        yield "random_small", grid_from_bits(rec["grid_bits"], rec["shape"]), rec
    for rec in load_golden("known_answers.json"):
        yield "known_answers", (np.array(rec["grid"], dtype=np.float64).reshape(rec["shape"]) == 1).astype(np.uint8), rec
    for rec in load_golden("maps_png.json"):
        bits = np.unpackbits(map_grids[rec["map"]])
        if "canvas" in rec:
            occ = np.zeros((256, 256), dtype=np.uint8)
            occ[:147, :112] = bits[:147 * 112].reshape(147, 112)
        else:
            W, H = rec["shape"]
            occ = bits[:W * H].reshape(W, H).astype(np.uint8)
        yield "maps_png", occ, rec


def test_single_call_counts_equal_the_real_jps1(planner, map_grids):
    """The one-query call (plan_single: one wavefront, counters in pinned host memory) against the counts captured from
    the reference itself: pops == rec["pops"] and pushes == rec["pushes"] - 1 when the record is searched, 0 and 0 otherwise."""
    assert "FXJPS_QSTAT" not in os.environ and os.environ.get("FXJPS_SINGLE", "1") != "0"
    n = {"random_small": 0, "known_answers": 0, "maps_png": 0}
    n_searched = 0
    labs = {}
    for name, occ, rec in golden_records(map_grids):
        key = occ.tobytes()
        if key not in labs:
            labs[key] = components(occ)
        planner.set_grid_occ(occ)
        off, cells, cost, st = planner.plan_batch([rec["start"]], [rec["goal"]], rec["hchoice"])
        t = planner.timing()
        assert t["waves"] == 1 and t["search_launches"] == 1, (name, rec["start"], rec["goal"], t)  # (the single-call path)
        if searched(occ, [rec["start"]], [rec["goal"]], labs[key])[0]:
            want = (rec["pops"], rec["pushes"] - 1)
            n_searched += 1
        else:
            want = (0, 0)
        assert (t["pops"], t["pushes"]) == want, (name, rec["shape"] if "shape" in rec else None, rec["start"], rec["goal"], rec["hchoice"],
                                                  (t["pops"], t["pushes"]), want)
        n[name] += 1
    assert n == {"random_small": 400, "known_answers": 16, "maps_png": 180} and n_searched >= 300, (n, n_searched)


def test_two_contexts_sum_to_the_reference(oracle):
    """Two contexts on device 0, a shard each: the timing record sums both contexts' counters."""
    import fuxi_planner_amd as fx
    occ, s, g = inputs("sparse")
    with fx.Planner([0, 0]) as p2:
        p2.set_grid_occ(occ)
        for h in (2, 1):
            ref = expected(oracle, "sparse", h)
            check_oracle_side("sparse", ref, far=True)
            res = p2.plan_batch(s, g, h, MPL)
            t = p2.timing()
            assert same_bytes(res, ref["csr"]) is None
            assert [c["queries"] for c in p2.timing_per_context()] == [200, 200]
            print("two contexts h=%d: pops %d (reference %d), pushes %d (reference %d)" % (h, t["pops"], ref["pops"].sum(), t["pushes"], ref["pushes"].sum()))
            assert t["retried"] == 0 and (t["pops"], t["pushes"]) == (int(ref["pops"].sum()), int(ref["pushes"].sum())), t
