"""GPU suite (-m gpu): fxjps_waypoint_slots_batch -- both waypoint rules over a grid-slots batch in ONE call, every query
with its own rule, slot, resolution and origin.  Everything is compared for equality of bytes: with the vectors captured
from the reference's own lines (waypoints.json, tick.json), with the one-path host functions those vectors pin
(fxjps_waypoint_st / fxjps_waypoint_ccst on get_grid_slot), and with the numpy restatement oracle/waypoints.py."""
import numpy as np
import pytest

from conftest import load_golden
from test_waypoints import cases, grid_of

pytestmark = pytest.mark.gpu
RESOS = (0.2, 0.5, 1.0)


@pytest.fixture(scope="module")
def planner():
    import fuxi_planner_amd as fx
    p = fx.Planner([0])
    yield p
    p.close()


def csr(paths):
    off = np.zeros(len(paths) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(p) for p in paths])
    cells = np.array([c for p in paths for c in p], dtype=np.int32).reshape(-1, 2)
    return off, cells


def same(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_reference_vectors_in_one_call(planner):
    from fuxi_planner_amd import waypoints
    recs = cases()
    assert len(recs) == 300
    rules = np.array([r["variant"] for r in recs], np.int32)
    assert (rules == 1).sum() == 150 and (rules == 0).sum() == 150
    assert (rules[:-1] != rules[1:]).sum() > 100, "the rules are to be interleaved"
    ids = np.zeros(300, np.int32)
    slot = 0
    for q, r in enumerate(recs):
        if r["variant"] == 1:
            planner.set_grid_slot(slot, grid_of(r))
            ids[q] = slot
            slot += 1
    assert slot == 150
    planner.set_grid_occ(np.zeros((8, 8), np.uint8))  # (no rule may read it)
    off, cells = csr([r["path"] for r in recs])
    ms = np.array([r.get("map_start", (0, 0)) for r in recs], np.int32)
    prev = np.array([(r.get("prev_wp") or []) + [0.0] * (3 - len(r.get("prev_wp") or [])) for r in recs])
    pdim = np.array([len(r.get("prev_wp") or []) for r in recs], np.int32)
    assert set(pdim[rules == 0].tolist()) == {0, 2, 3}
    assert len({tuple(r["origin"]) for r in recs}) == 300 and len({r["reso"] for r in recs}) == 4
    wp, dim, gout, ang, nk, kept = waypoints.select_slots_batch(
        planner, rules, ms, [r["reso"] for r in recs], [r["origin"] for r in recs], [r["pos"] for r in recs], [r["goal"] for r in recs],
        [r["end_occu"] for r in recs], prev, pdim, grid_ids=ids, paths=(off, cells), return_kept=True)
    pruned = moved = two = held = 0
    for q, r in enumerate(recs):
        exp = r["out"]
        assert wp[q, :dim[q]].tolist() == exp["wp"] and gout[q].tolist() == exp["goal_out"], (q, r["variant"], wp[q], exp)
        if r["variant"] == 1:
            assert dim[q] == 3 and ang[q] == 0.0
            assert kept[off[q]:off[q] + nk[q]].tolist() == exp["kept"], q
            pruned += len(exp["kept"]) < len(r["path"])
            moved += exp["wp"] != r["goal"]
        else:
            assert ang[q] == exp["ang_wp"] and nk[q] == 0, q
            two += len(exp["wp"]) == 2
        held += r["end_occu"] == 1
    # what the fixture exercises (144 / 84 / 66 / 45 as it stands), so that a thinner one cannot pass silently
    assert pruned >= 140 and moved >= 80 and two >= 60 and held >= 40, (pruned, moved, two, held)
    for s in range(150):
        planner.clear_grid_slot(s)


def fleet_tick(p):
    """The 120 ticks of tick.json as one fleet tick of three calls.  -> everything the waypoint call needs and returned"""
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import waypoints
    from test_prepare_slots_gpu import golden_job
    recs = load_golden("tick.json")
    assert len(recs) == 120 and {r["variant"] for r in recs} == {0, 1}
    outs = p.prepare_slots([golden_job(i, r) for i, r in enumerate(recs)])
    assert all(o[5] for o in outs)
    off, cells, cost, st = p.plan_batch_slots(np.arange(120), [o[0] for o in outs], [o[1] for o in outs], 2)
    args = dict(rule=[r["variant"] for r in recs], map_start=[o[0] for o in outs], map_reso=[r["reso"] for r in recs],
                map_o=[fx.Planner.shifted_origin(r["origin"], o[2], r["reso"]) for r, o in zip(recs, outs)], pos=[r["pos"] for r in recs],
                global_goal=[r["goal3"] for r in recs], end_occu=[o[4] for o in outs],
                prev_wp=[(r["prev_wp"] or []) + [0.0] * (3 - len(r["prev_wp"] or [])) for r in recs],
                prev_dim=[len(r["prev_wp"] or []) for r in recs])
    res = waypoints.select_slots_batch(p, **args)                              # the resident paths, the ids of the batch
    wp, dim, gout, ang, nk = res
    planned = inter = held = 0
    for i, (o, r) in enumerate(zip(outs, recs)):
        if r["path"] is None:
            assert st[i] == 0 and wp[i].tolist() == r["goal3"] and dim[i] == 3 and nk[i] == 0, i
            continue
        assert st[i] > 0 and cells[off[i]:off[i + 1]].tolist() == r["path"], i
        planned += 1
        assert gout[i].tolist() == r["goal_out"], i
        assert wp[i, :dim[i]].tolist() == r["wp"], (i, r["variant"], wp[i], r["wp"])
        inter += r["wp"][:2] != r["goal3"][:2]
        held += o[4]
    assert planned > 50 and inter > 20 and held > 15
    return args, (off, cells), res


def test_golden_fleet_tick_in_one_call(planner):
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import waypoints
    args, paths, res = fleet_tick(planner)
    again = waypoints.select_slots_batch(planner, paths=paths, grid_ids=np.arange(120), **args)
    assert same(again, res)
    with fx.Planner([0, 0]) as p2:
        _, _, res2 = fleet_tick(p2)
        per = [t["queries"] for t in p2.timing_per_context()]
        assert sum(per) == 120 and min(per) > 0, per  # (both contexts served a shard)
        assert same(res2, res)


def serpentine(W, H, step=3):
    """Walls every `step` columns, open at alternating ends: a path across turns twice per wall."""
    occ = np.zeros((W, H), np.uint8)
    for k, x in enumerate(range(step - 1, W - 1, step)):
        occ[x, :] = 1
        occ[x, 0 if k & 1 else H - 1] = 0
    return occ


def sizes_case():
    """Host only: 26 grids of clearly different extents, their queries and the per-query inputs of test 3.
    -> (grids, ids, starts, goals, inputs)"""
    from fuxi_planner_amd import synth
    rng = np.random.default_rng(730)
    shapes = [(31, 47), (64, 64), (90, 33), (120, 200), (257, 129), (300, 300), (720, 700), (500, 61), (45, 410), (160, 160), (200, 96), (77, 77),
              (350, 220), (128, 512), (610, 140), (33, 33), (240, 180), (99, 301), (420, 400), (150, 55), (70, 260), (280, 75), (512, 512), (111, 222)]
    grids = [synth.synth_grid(W, H, 900 + k, 0.15 + 0.10 * (k % 5) / 4) for k, (W, H) in enumerate(shapes)]
    grids.append(np.zeros((140, 90), np.uint8))  # open
    grids.append(serpentine(420, 24))
    ids, starts, goals = [], [], []
    for k, occ in enumerate(grids):
        n = int(rng.integers(20, 61))
        if k == len(grids) - 1:  # the serpentine: across the whole of it and across half of it, four times each (both rules)
            s = np.array([(0, 1)] * 4 + [(0, 2)] * 4 + [(1, 5)] * (n - 8), np.int32)
            g = np.array([(419, 3)] * 4 + [(150, 3)] * 4 + [(40, 7)] * (n - 8), np.int32)
        else:
            s, g = synth.synth_queries(occ, 40 + k, n)
        ids += [k] * n
        starts.append(s)
        goals.append(g)
    ids = np.array(ids, np.int32)
    s, g = np.concatenate(starts).astype(np.int32), np.concatenate(goals).astype(np.int32)
    nq = len(ids)
    rule = (np.arange(nq) & 1).astype(np.int32)
    reso = np.array([RESOS[k % 3] for k in ids])
    slot_o = rng.uniform(-50, 50, (len(grids), 2))
    origin = slot_o[ids]
    # the vehicle near its start cell in the frame of its rule: st path2 = path + (1, 1), ccst path2 = path + (1, 0)
    pos = np.c_[(s[:, 0] + 1) * reso + origin[:, 0] + rng.normal(0, 0.4, nq), (s[:, 1] + 1 - rule) * reso + origin[:, 1] + rng.normal(0, 0.4, nq),
                rng.choice([0.0, 0.5, 1.2], nq)]
    goal = np.c_[(g[:, 0] + 1) * reso + origin[:, 0], (g[:, 1] + 1 - rule) * reso + origin[:, 1], np.full(nq, 1.5)]
    inputs = dict(rule=rule, map_start=s + 1 + rng.integers(-1, 2, (nq, 2)), map_reso=reso, map_o=origin, pos=pos, global_goal=goal,
                  end_occu=(rng.random(nq) < 0.1).astype(np.int32), prev_wp=rng.uniform(-60, 200, (nq, 3)),
                  prev_dim=rng.choice([0, 0, 2, 3], nq).astype(np.int32))
    return grids, ids, s, g, inputs


def sizes_expect(grids, ids, off, cells, st, inp, check=None):
    """The one-path host functions on every query (and the numpy restatement on the first 320 ccst queries with a path);
    check(q, wp, dim, goal, ang, kept) compares.  -> the coverage figures"""
    from fuxi_planner_amd import waypoints
    from oracle import waypoints as ow
    long_ = {0: 0, 1: 0}
    n_ccst = pruned = n_st = inter = restated = 0
    for q in range(len(ids)):
        path = cells[off[q]:off[q + 1]]
        o, ps, gl, eo, rs = inp["map_o"][q], inp["pos"][q], inp["global_goal"][q], int(inp["end_occu"][q]), inp["map_reso"][q]
        if st[q] <= 0:
            exp = (gl, 3, gl, 0.0, path[:0])
        elif inp["rule"][q] == 1:
            w, k, g1 = waypoints.select_ccst(path, grids[ids[q]], rs, o, ps, gl, eo, return_goal=True)
            exp = (w, 3, g1, 0.0, k)
            n_ccst += 1
            pruned += len(k) < len(path)
            if restated < 320:
                w2, k2, g2 = ow.select_ccst(path, grids[ids[q]].astype(np.float64), rs, o, ps, gl, eo)
                assert np.array_equal(k, k2) and w.tobytes() == np.asarray(w2, np.float64).tobytes() and g1.tobytes() == np.asarray(g2, np.float64).tobytes(), q
                restated += 1
        else:
            pd = int(inp["prev_dim"][q])
            w, g1, a = waypoints.select_st(path, inp["map_start"][q], rs, o, ps, gl, eo, inp["prev_wp"][q][:pd] if pd else None)
            exp = (w, len(w), g1, a, path[:0])
            n_st += 1
            inter += len(w) == 2
        if st[q] > 128:
            long_[int(inp["rule"][q])] += 1
        if check:
            check(q, *exp)
    return dict(n_ccst=n_ccst, pruned=pruned, n_st=n_st, inter=inter, long_st=long_[0], long_ccst=long_[1], restated=restated,
                mid=int(((st > 64) & (st <= 128)).sum()))


def assert_sizes_coverage(c, grids):
    assert len(grids) >= 24 and max(min(g.shape) for g in grids) >= 700
    assert c["long_st"] >= 1 and c["long_ccst"] >= 1 and c["mid"] >= 1, c
    assert 2 * c["pruned"] >= c["n_ccst"] and 5 * c["inter"] >= c["n_st"] and c["restated"] >= 300, c


def test_different_sizes_and_long_paths(planner):
    from fuxi_planner_amd import waypoints
    grids, ids, s, g, inp = sizes_case()
    for k, occ in enumerate(grids):
        planner.set_grid_slot(k, occ)
    off, cells, cost, st = planner.plan_batch_slots(ids, s, g, 2, 2048)
    wp, dim, gout, ang, nk, kept = waypoints.select_slots_batch(planner, grid_ids=ids, paths=(off, cells), return_kept=True, **inp)
    res = waypoints.select_slots_batch(planner, **inp)  # ... and the resident paths
    assert same(res, (wp, dim, gout, ang, nk))

    def check(q, w, d, g1, a, k):
        assert dim[q] == d and wp[q, :d].tobytes() == np.asarray(w, np.float64).tobytes() and not wp[q, d:].any(), (q, wp[q], w)
        assert gout[q].tobytes() == np.asarray(g1, np.float64).tobytes() and ang[q] == a, (q, ang[q], a)
        assert nk[q] == len(k) and np.array_equal(kept[off[q]:off[q] + nk[q]], k), q
    assert_sizes_coverage(sizes_expect([planner.get_grid_slot(k) for k in range(len(grids))], ids, off, cells, st, inp, check), grids)
    for k in range(len(grids)):
        planner.clear_grid_slot(k)


def two_slot_case():
    """Two grids of the same extents whose obstacles make the ccst pruning of one path differ; the resident grid is free."""
    a = np.zeros((40, 40), np.uint8)
    b = a.copy()
    b[10:20, 10:20] = 1  # on the straight lines between the points of the path
    path = [(2, 2), (8, 14), (15, 15), (22, 16), (30, 30), (36, 31)]
    return a, b, path


def test_the_named_slot_is_read(planner):
    from fuxi_planner_amd import waypoints
    a, b, path = two_slot_case()
    planner.set_grid_slot(7, a)
    planner.set_grid_slot(9, b)
    planner.set_grid_occ(np.zeros((40, 40), np.uint8))
    off, cells = csr([path, path])
    pos, goal = (100.0, 100.0, 0.0), (36.0, 31.0, 1.0)
    one = {k: waypoints.select_ccst(path, m, 1.0, (0.0, 0.0), pos, goal, 0, return_goal=True) for k, m in ((7, a), (9, b))}
    assert len(one[7][1]) != len(one[9][1]) and one[7][0].tobytes() != one[9][0].tobytes()
    for ids in ((7, 9), (9, 7)):
        wp, dim, gout, ang, nk, kept = waypoints.select_slots_batch(planner, [1, 1], None, 1.0, (0.0, 0.0), pos, goal, grid_ids=ids,
                                                                    paths=(off, cells), return_kept=True)
        for q, k in enumerate(ids):
            assert wp[q].tobytes() == one[k][0].tobytes() and np.array_equal(kept[off[q]:off[q] + nk[q]], one[k][1]), (ids, q)
    planner.clear_grid_slot(7)
    planner.clear_grid_slot(9)


def small_fleet(p, first_slot=20, n=6, seed=5):
    from fuxi_planner_amd import synth
    rng = np.random.default_rng(seed)
    grids = [synth.synth_grid(50 + 9 * k, 70 - 5 * k, 60 + k, 0.2) for k in range(n)]
    for k, occ in enumerate(grids):
        p.set_grid_slot(first_slot + k, occ)
    ids = np.repeat(np.arange(first_slot, first_slot + n), 5).astype(np.int32)
    q = [synth.synth_queries(occ, 70 + k, 5) for k, occ in enumerate(grids)]
    s, g = np.concatenate([x[0] for x in q]).astype(np.int32), np.concatenate([x[1] for x in q]).astype(np.int32)
    nq = len(ids)
    inp = dict(rule=(np.arange(nq) & 1).astype(np.int32), map_start=s + 1, map_reso=np.array(RESOS)[ids % 3], map_o=rng.uniform(-5, 5, (nq, 2)),
               pos=np.c_[s + rng.normal(0, 0.5, (nq, 2)), np.zeros(nq)], global_goal=np.c_[g + 1.0, np.ones(nq)],
               end_occu=(rng.random(nq) < 0.2).astype(np.int32), prev_wp=rng.uniform(0, 50, (nq, 3)), prev_dim=rng.choice([0, 2, 3], nq).astype(np.int32))
    return grids, ids, s, g, inp


def raw_call(p, nq, off, cells, ids, inp, rule=None):
    """The C call itself (the refusals need what the wrapper cannot express).  -> (rc, error text)"""
    import ctypes as C
    from fuxi_planner_amd import _lib
    f64 = lambda a, shape: np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float64), shape))  # noqa: E731
    i32 = lambda a, shape: np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.int32), shape))    # noqa: E731
    n = max(nq, 1)
    a = dict(rule=i32(inp["rule"] if rule is None else rule, (len(inp["rule"]),)), ms=i32(inp["map_start"], (len(inp["rule"]), 2)),
             reso=f64(inp["map_reso"], (len(inp["rule"]),)), o=f64(inp["map_o"], (len(inp["rule"]), 2)), pos=f64(inp["pos"], (len(inp["rule"]), 3)),
             goal=f64(inp["global_goal"], (len(inp["rule"]), 3)), wp=np.zeros((n, 3)))
    opt = lambda x, t: None if x is None else _lib.ptr(x, t)  # noqa: E731
    rc = p._L.fxjps_waypoint_slots_batch(p._h, nq, opt(off, C.c_int64), opt(cells, C.c_int32), opt(ids, C.c_int32), _lib.ptr(a["rule"], C.c_int32),
                                         _lib.ptr(a["ms"], C.c_int32), _lib.ptr(a["reso"], C.c_double), _lib.ptr(a["o"], C.c_double),
                                         _lib.ptr(a["pos"], C.c_double), _lib.ptr(a["goal"], C.c_double), None, 2.0, 0.7, None, None,
                                         _lib.ptr(a["wp"], C.c_double), None, None, None, None, None, 0, 0)
    return rc, p._L.fxjps_last_error(p._h).decode()


def test_refusals_change_nothing(planner):
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import _lib, waypoints
    grids, ids, s, g, inp = small_fleet(planner)
    nq = len(ids)
    planner.set_grid_occ(grids[0])
    off, cells, cost, st = planner.plan_batch_slots(ids, s, g, 2)
    good = waypoints.select_slots_batch(planner, **inp)
    k = 7  # (a ccst query: rule = q & 1)
    assert inp["rule"][k] == 1 and st[k] > 1

    def edit(a, v):
        a = np.array(a)
        a[k] = v
        return a
    neg = cells.copy()
    neg[off[k] + 1, 1] = -1
    down = off.copy()
    down[k + 1] = down[k] - 1
    planner.clear_grid_slot(31)
    refused = [(nq, off, cells, edit(ids, _lib.MAX_GRID_SLOTS), None), (nq, off, cells, edit(ids, -1), None), (nq, off, cells, edit(ids, 31), None),
               (nq, None, None, edit(ids, 31), None), (nq, off, cells, ids, edit(inp["rule"], 2)), (nq, None, None, None, edit(inp["rule"], -1)),
               (nq, down, cells, ids, None), (nq, off, neg, ids, None)]
    for args in refused:
        rc, text = raw_call(planner, *args[:4], inp, rule=args[4])
        assert rc == _lib.E_ARG and "query %d" % k in text, (args[3:], rc, text)
    rc, text = raw_call(planner, nq, off, cells, None, inp)  # explicit paths, a ccst query (the first is query 1) and no ids
    assert rc == _lib.E_ARG and "query 1:" in text, text
    # (an st query ignores its slot and may have negative cells: the same edits at an st query are no refusals)
    st_q = 6
    ids_st = np.array(ids)
    ids_st[st_q] = -1
    assert raw_call(planner, nq, off, cells, ids_st, inp)[0] == 0
    rc, text = raw_call(planner, nq - 1, None, None, None, inp)  # not the last batch's nq
    assert rc == _lib.E_ARG and str(nq) in text
    assert raw_call(planner, 0, np.zeros(1, np.int64), np.zeros((1, 2), np.int32), None, inp)[0] == 0  # an empty call does nothing
    assert same(waypoints.select_slots_batch(planner, **inp), good)
    # after the call the ccst batch call still refuses resident paths of a slots batch
    with pytest.raises(fx.FxjpsError) as e:
        waypoints.select_ccst_batch(planner, nq, 1.0, (0.0, 0.0), inp["pos"], inp["global_goal"])
    assert e.value.code == _lib.E_ARG
    assert same(waypoints.select_slots_batch(planner, **inp), good)
    # resident paths of a batch that was not a slots batch
    planner.plan_batch(s[:5], g[:5], 2)
    sub = {key: (v[:5] if isinstance(v, np.ndarray) else v) for key, v in inp.items()}
    rc, text = raw_call(planner, 5, None, None, ids[:5], sub)
    assert rc == _lib.E_ARG and "slots" in text
    planner.plan_batch_slots(ids, s, g, 2)
    assert same(waypoints.select_slots_batch(planner, **inp), good)
    for k in range(len(grids)):
        planner.clear_grid_slot(20 + k)


def test_nothing_else_moved(planner):
    from fuxi_planner_amd import synth, waypoints
    grids, ids, s, g, inp = small_fleet(planner, first_slot=40, seed=6)
    keep = {60: synth.synth_grid(90, 70, 21, 0.2), 61: synth.synth_grid(40, 130, 22, 0.25)}
    for k, occ in keep.items():
        planner.set_grid_slot(k, occ)
    resident = synth.synth_grid(150, 110, 23, 0.2)
    rs, rg = synth.synth_queries(resident, 23, 100)
    planner.set_grid_occ(resident)
    planner.set_queries(rs, rg, 2)
    first = planner.replan_frame()
    planner.replan_frame()
    reused = planner.timing()["reused"]
    assert reused > 0
    plan = planner.plan_batch_slots(ids, s, g, 2)
    a = waypoints.select_slots_batch(planner, **inp)
    b = waypoints.select_slots_batch(planner, **inp)  # the resident paths are what they were
    c = waypoints.select_slots_batch(planner, grid_ids=ids, paths=plan[:2], **inp)
    assert same(a, b) and same(a, c)
    for k, occ in enumerate(grids):
        assert np.array_equal(planner.get_grid_slot(40 + k), occ), k
    for k, occ in keep.items():
        assert np.array_equal(planner.get_grid_slot(k), occ), k
    assert np.array_equal(planner.get_grid(), resident)
    assert same(planner.plan_batch_slots(ids, s, g, 2), plan)
    planner.set_queries(rs, rg, 2)  # (a batch in between drops the stored results, as ever: store them again)
    planner.replan_frame()
    waypoints.select_slots_batch(planner, grid_ids=ids, paths=plan[:2], **inp)
    assert same(planner.replan_frame(), first) and planner.timing()["reused"] == reused
    for k in list(keep) + [40 + k for k in range(len(grids))]:
        planner.clear_grid_slot(k)


def test_host_form_of_the_st_rule(planner, monkeypatch):
    from fuxi_planner_amd import waypoints
    grids, ids, s, g, inp = small_fleet(planner, first_slot=80, seed=7)
    plan = planner.plan_batch_slots(ids, s, g, 2)
    dev = waypoints.select_slots_batch(planner, **inp)
    dev2 = waypoints.select_slots_batch(planner, grid_ids=ids, paths=plan[:2], return_kept=True, **inp)
    monkeypatch.setenv("FXJPS_WAYPOINT_ST_HOST", "1")
    host = waypoints.select_slots_batch(planner, **inp)
    host2 = waypoints.select_slots_batch(planner, grid_ids=ids, paths=plan[:2], return_kept=True, **inp)
    monkeypatch.delenv("FXJPS_WAYPOINT_ST_HOST")
    assert same(dev, host) and same(dev2, host2) and same(dev, dev2[:5])
    assert set(dev[1].tolist()) == {2, 3} and (dev[4] > 0).any()
    # a map_start so far off the grid that the table of angles would not fit: the call takes the host form by itself
    far = dict(inp, map_start=np.tile(np.array([[3000000, -2000000]], np.int32), (len(ids), 1)))
    got = waypoints.select_slots_batch(planner, **far)
    for q in range(len(ids)):
        if inp["rule"][q] == 0 and plan[3][q] > 0:
            pd = int(inp["prev_dim"][q])
            w, g1, a = waypoints.select_st(plan[1][plan[0][q]:plan[0][q + 1]], far["map_start"][q], inp["map_reso"][q], inp["map_o"][q], inp["pos"][q],
                                           inp["global_goal"][q], int(inp["end_occu"][q]), inp["prev_wp"][q][:pd] if pd else None)
            assert got[0][q, :got[1][q]].tobytes() == w.tobytes() and got[3][q] == a, q
        elif inp["rule"][q] == 1:
            assert all(x[q].tobytes() == y[q].tobytes() for x, y in zip(got, dev)), q
    for k in range(len(grids)):
        planner.clear_grid_slot(80 + k)
