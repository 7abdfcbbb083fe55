"""GPU suite (-m gpu): fxjps_tick_outputs_slots -- the waypoint, the Point of /goal_global, /jps_path and the ccst node's
/direct_jps_path of every query of a grid-slots batch in ONE call.  Everything is compared as bit patterns (view(np.uint64),
so a NaN z has to be the reference's NaN): with tests/golden/tick_outputs.json, produced by executing the nodes' own lines,
and, on crafted and planned paths, with the one-path host functions (fxjps_waypoint_st / fxjps_waypoint_ccst, which that
file and waypoints.json pin) followed by the numpy restatement of tests/test_tick_outputs_host.py.  Every reference value is
computed on the host before the device is asked."""
import ctypes as C

import numpy as np
import pytest

from test_tick_outputs_host import f64, load_golden, restate, u64

pytestmark = pytest.mark.gpu
EMPTY, SERP = 6, 7  # slots behind the golden maps: an open 48 x 48 grid and a serpentine one


def serpentine(W, H, step=3):
    occ = np.zeros((W, H), np.uint8)
    for k, x in enumerate(range(step - 1, W - 1, step)):
        occ[x, :] = 1
        occ[x, 0 if k & 1 else H - 1] = 0
    return occ


GRIDS = {EMPTY: np.zeros((48, 48), np.uint8), SERP: serpentine(48, 48)}


@pytest.fixture(scope="module")
def golden():
    return load_golden()


@pytest.fixture(scope="module")
def planner(golden):
    import fuxi_planner_amd as fx
    p = fx.Planner([0])
    for s, m in enumerate(golden[0]):
        p.set_grid_slot(s, m)
        GRIDS[s] = m
    p.set_grid_slot(EMPTY, GRIDS[EMPTY])
    p.set_grid_slot(SERP, GRIDS[SERP])
    yield p
    p.close()


def csr(paths):
    off = np.zeros(len(paths) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(p) for p in paths])
    cells = np.array([c for p in paths for c in p], dtype=np.int32).reshape(-1, 2)
    return off, cells


def query(variant, slot, path, reso=0.25, origin=(-1.5, 2.25), pos=(-40.0, -35.5, 1.0), goal=(9.0, 7.5, 2.0), home=(-3.0, 4.0), end_occu=0,
          map_start=(1, 1), prev_wp=None):
    return dict(variant=variant, map=slot, path=[list(map(int, c)) for c in path], reso=reso, origin=list(origin), pos=list(pos), goal=list(goal),
                home=list(home), end_occu=end_occu, map_start=list(map_start), prev_wp=prev_wp)


def expect(c):
    """One query on the host: the one-path rule, then the restatement.  -> dict of what the call returns for it"""
    from fuxi_planner_amd import waypoints
    kept, ang = [], 0.0
    if not c["path"]:
        wp, gout = np.array(c["goal"], dtype=np.float64), np.array(c["goal"], dtype=np.float64)
    elif c["variant"] == 0:
        wp, gout, ang = waypoints.select_st(c["path"], c["map_start"], c["reso"], c["origin"], c["pos"], c["goal"], c["end_occu"], c.get("prev_wp"))
    else:
        wp, kept, gout = waypoints.select_ccst(c["path"], GRIDS[c["map"]], c["reso"], c["origin"], c["pos"], c["goal"], c["end_occu"], return_goal=True)
    point, path3, dirp, back = restate(c["variant"], c["path"], c["reso"], c["origin"], c["pos"], c["home"], c["end_occu"], wp, gout, kept)
    return dict(wp=wp, goal_out=gout, ang=ang, n_kept=len(kept), kept=np.asarray(kept, np.int32).reshape(-1, 2), point=point, path3=path3, dir=dirp,
                back=back)


def call(p, cs, paths="explicit", offsets=None):
    from fuxi_planner_amd import waypoints
    prev = np.array([(c.get("prev_wp") or []) + [0.0] * (3 - len(c.get("prev_wp") or [])) for c in cs])
    pdim = np.array([len(c.get("prev_wp") or []) for c in cs], np.int32)
    kw = dict(paths=csr([c["path"] for c in cs]), grid_ids=[c["map"] for c in cs]) if paths == "explicit" else dict(offsets=offsets)
    return waypoints.tick_outputs_slots(p, [c["variant"] for c in cs], [c.get("map_start", (0, 0)) for c in cs], [c["reso"] for c in cs],
                                        [c["origin"] for c in cs], [c["pos"] for c in cs], [c["goal"] for c in cs], [c["home"] for c in cs],
                                        [c["end_occu"] for c in cs], prev, pdim, return_kept=True, **kw)


def flat(res):
    """every byte a call returned, in one tuple of arrays"""
    wp, dim, gout, ang, nk, point, paths, dirs, back, kept = res
    return [wp, dim, gout, ang, nk, point, back, kept] + list(paths) + list(dirs)


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def check(res, q, e, tag):
    wp, dim, gout, ang, nk, point, paths, dirs, back, kept = res
    at = sum(len(p) for p in paths[:q])  # (offsets[q]: where path q's cells, and so its kept cells, begin)
    assert nk[q] == len(e["kept"]) and kept[at:at + nk[q]].tolist() == e["kept"].tolist(), (tag, q, kept[at:at + nk[q]], e["kept"])
    assert u64(wp[q, :dim[q]]).tolist() == u64(e["wp"]).tolist(), (tag, q, wp[q], e["wp"])
    assert u64(gout[q]).tolist() == u64(e["goal_out"]).tolist(), (tag, q)
    assert u64(ang[q:q + 1]).tolist() == u64([e["ang"]]).tolist() and nk[q] == e["n_kept"], (tag, q)
    assert u64(point[q]).tolist() == u64(e["point"]).tolist(), (tag, q, point[q], e["point"])
    assert paths[q].shape == e["path3"].shape and u64(paths[q]).tolist() == u64(e["path3"]).tolist(), (tag, q)
    assert dirs[q].shape == e["dir"].shape and u64(dirs[q]).tolist() == u64(e["dir"]).tolist(), (tag, q, dirs[q], e["dir"])
    assert back[q] == e["back"], (tag, q)


def test_golden_vectors_in_one_call(planner, golden):
    from fuxi_planner_amd import waypoints
    maps, cases = golden
    rules = np.array([c["variant"] for c in cases])
    assert (rules[:-1] != rules[1:]).all(), "st and ccst alternate inside every block of four wavefronts"
    for c in cases:
        c.setdefault("map_start", [0, 0])
    exp = [expect(c) for c in cases]
    res = call(planner, cases)
    wp, dim, gout, ang, nk, point, paths, dirs, back, kept = res
    nan = 0
    for q, c in enumerate(cases):
        o = c["out"]
        assert ["%016x" % v for v in u64(wp[q, :dim[q]])] == o["wp"] and ["%016x" % v for v in u64(gout[q])] == o["goal_out"], q
        assert ["%016x" % v for v in u64(point[q])] == o["point"], (q, point[q], f64(o["point"]))
        assert ["%016x" % v for v in u64(paths[q])] == o["path3"] and len(paths[q]) == len(c["path"]), q
        assert ["%016x" % v for v in u64(dirs[q])] == o["dir"] and back[q] == o["dir_back"], q
        if c["variant"] == 0:
            assert "%016x" % u64(ang[q:q + 1])[0] == o["ang_wp"] and nk[q] == 0 and len(dirs[q]) == 0, q
        else:
            assert nk[q] == len(o["kept"]) and len(dirs[q]) == (nk[q] if c["path"] else 2), q
        check(res, q, exp[q], "golden")
        nan += bool(np.isnan(point[q, 2]))
    assert nan >= 4
    # the six shared outputs are fxjps_waypoint_slots_batch's on the same batch; a second call returns the same bytes
    prev = np.array([(c.get("prev_wp") or []) + [0.0] * (3 - len(c.get("prev_wp") or [])) for c in cases])
    pdim = np.array([len(c.get("prev_wp") or []) for c in cases], np.int32)
    old = waypoints.select_slots_batch(planner, rules, [c["map_start"] for c in cases], [c["reso"] for c in cases], [c["origin"] for c in cases],
                                       [c["pos"] for c in cases], [c["goal"] for c in cases], [c["end_occu"] for c in cases], prev, pdim,
                                       grid_ids=[c["map"] for c in cases], paths=csr([c["path"] for c in cases]), return_kept=True)
    assert same(list(old), [wp, dim, gout, ang, nk, kept])
    off = csr([c["path"] for c in cases])[0]
    pruned = 0
    for q, c in enumerate(cases):  # (the sixth against the file too, and as the direct path it becomes)
        if c["variant"] == 1 and c["path"]:
            k = kept[off[q]:off[q] + nk[q]]
            assert k.tolist() == c["out"]["kept"], q
            assert u64(dirs[q][:, 0]).tolist() == u64((k[:, 0] + 1) * c["reso"] + c["origin"][0]).tolist(), q
            pruned += len(k) < len(c["path"])
    assert pruned >= 8
    assert same(flat(call(planner, cases)), flat(res))


def shapes_case(planner):
    """Crafted paths of 0, 1, 2, 3, 64 and 65 points under both rules (on the open grid the pruning keeps two), a planned one
    and one the pruning keeps whole."""
    zig = [(i % 47, (7 * i) % 45 + (i & 1)) for i in range(65)]
    off, cells, _, st = planner.plan_batch_slots([SERP], [(0, 0)], [(47, 47)], 2)
    assert st[0] > 8
    serp = cells[off[0]:off[1]].tolist()
    cs = []
    for n in (0, 1, 2, 3, 64, 65):
        cs.append(query(0, EMPTY, zig[:n], map_start=(2, 3), home=(-3.0 + n, 4.0)))
        cs.append(query(1, EMPTY, zig[:n], reso=0.5, origin=(0.125, -7.0)))
    cs.append(query(1, SERP, serp, reso=0.2, pos=(-30.0, 1.0, 0.5)))                               # every point blocks a line
    cs.append(query(1, SERP, serp, reso=0.2, origin=(0.0, 0.0), pos=(0.3, 0.1, 0.5), end_occu=1))  # the near points go, the position is held
    cs.append(query(0, SERP, serp, map_start=(1, 1), pos=(0.0, 0.0, 1.0), prev_wp=[1.0, 2.0]))
    cs.append(query(1, SERP, [[1, 41], [6, 20], [22, 13], [33, 39], [43, 12]]))                     # every line is blocked: all five stay
    cs.append(query(0, EMPTY, zig[:3], goal=(-3.0, 4.0, 1.5)))                                     # goal == home: x / 0
    cs.append(query(1, EMPTY, [], goal=(-3.0, 4.0, 1.5)))                                          # ... and 0 / 0
    return cs


def test_smallest_shapes_that_can_go_wrong(planner):
    cs = shapes_case(planner)
    exp = [expect(c) for c in cs]
    kept = {(len(c["path"]), e["n_kept"]) for c, e in zip(cs, exp) if c["variant"] == 1}
    assert (65, 2) in kept and (64, 2) in kept and any(n > 3 and k == n for n, k in kept), kept  # the pruning keeps 2, and keeps all
    assert np.isnan(exp[-1]["point"][2]) and not np.isnan(exp[-2]["point"][2])
    for q, c in enumerate(cs):  # nq = 1: a block with one wavefront at work
        check(call(planner, [c]), 0, exp[q], "alone")
    for q0 in range(0, len(cs) - 4, 3):  # nq = 5: a partial last block, the rules alternating in the first
        res = call(planner, cs[q0:q0 + 5])
        for i in range(5):
            check(res, i, exp[q0 + i], "five")
    res = call(planner, cs)
    for q in range(len(cs)):
        check(res, q, exp[q], "all")


def fleet(golden):
    """Eight vehicles on the golden maps (one whose preparation fails), as Planner.fleet_tick takes them."""
    maps, _ = golden
    rng = np.random.default_rng(750)
    cross = np.zeros((5, 4), np.uint8)
    cross[2, :] = 1
    cross[:, 1] = 1
    jobs, pos, goals, home = [], [], [], []
    for v in range(8):
        m = maps[(2, 1, 5, 3, 2, 0, 5, 0)[v]]  # (st on the sparse maps: its dilation closes the dense ones)
        free = np.argwhere(m == 0)
        s, g = free[rng.integers(0, len(free))], free[rng.integers(0, len(free))]
        jobs.append((10 + v, m, (int(s[0]), int(s[1])), (int(g[0]), int(g[1])), 1 - v % 2, v % 2))  # (ifa: st 1, ccst 0)
        pos.append([0.25 * s[0] - 2.0, 0.25 * s[1] + 1.0, 1.0])
        goals.append([0.25 * g[0] - 2.0, 0.25 * g[1] + 1.0, 1.5 + 0.25 * (v % 3)])
        home.append([-2.0 + 0.5 * v, 1.0])
    jobs[5] = (15, cross, (0, 0), (2, 1), 0, 1)
    home[2] = goals[2][:2]
    return jobs, np.array(pos), np.array(goals), np.array(home)


def four_calls(p, jobs, pos, goals, home, reso, map_o):
    """INTEGRATION.md section 3d by hand.  -> (live, outs, (offsets, cells, status), the queries as `expect` takes them,
    publish_slots' result)"""
    import fuxi_planner_amd as fx
    outs = p.prepare_slots(jobs)
    live = [v for v in range(len(jobs)) if outs[v][5]]
    slots = [jobs[v][0] for v in live]
    off, cells, cost, st = p.plan_batch_slots(slots, [outs[v][0] for v in live], [outs[v][1] for v in live], 2)
    cs = []
    for i, v in enumerate(live):
        GRIDS[jobs[v][0]] = p.get_grid_slot(jobs[v][0])
        cs.append(query(jobs[v][5], jobs[v][0], cells[off[i]:off[i + 1]].tolist(), reso=reso, origin=fx.Planner.shifted_origin(map_o, outs[v][2], reso),
                        pos=pos[v], goal=goals[v], home=home[v], end_occu=outs[v][4], map_start=outs[v][0]))
    return live, outs, (off, cells, st), cs, p.publish_slots(slots, msg=True, image_channels=1)


def test_resident_paths_two_contexts_and_fleet_tick(planner, golden):
    import fuxi_planner_amd as fx
    jobs, pos, goals, home = fleet(golden)
    reso, map_o = 0.25, (-2.0, 1.0)
    live, outs, (off, cells, st), cs, pub = four_calls(planner, jobs, pos, goals, home, reso, map_o)
    assert live == [0, 1, 2, 3, 4, 6, 7] and (st > 0).sum() >= 4
    exp = [expect(c) for c in cs]
    res = call(planner, cs, paths="resident", offsets=off)            # the paths the batch left on the device, its slot ids
    for q in range(len(cs)):
        check(res, q, exp[q], "resident")
    assert same(flat(call(planner, cs)), flat(res))                    # ... and the same paths handed over
    from fuxi_planner_amd import waypoints
    old = waypoints.select_slots_batch(planner, [c["variant"] for c in cs], [c["map_start"] for c in cs], reso, [c["origin"] for c in cs],
                                       [c["pos"] for c in cs], [c["goal"] for c in cs], [c["end_occu"] for c in cs], paths=(off, None), return_kept=True)
    assert same(list(old), list(res[:5]) + [res[9]]) and res[4].sum() > 0
    recs = planner.fleet_tick(jobs, pos, goals, home, reso, map_o, publish=True, image_channels=1)
    assert len(recs) == 8 and recs[5]["ok"] is False and recs[5]["wp"] is None and recs[5]["status"] is None
    for i, v in enumerate(live):
        r = recs[v]
        assert r["ok"] and r["status"] == st[i] and r["start"] == outs[v][0] and r["end_occu"] == outs[v][4] and r["origin"] == cs[i]["origin"]
        one = (r["wp"], r["goal_out"], np.array([r["ang_wp"]]), r["point"], r["path"], r["dir_path"], r["msg"], r["image"])
        ref = (res[0][i, :res[1][i]], res[2][i], res[3][i:i + 1], res[5][i], res[6][i], res[7][i], pub[i][0], pub[i][2])
        assert same(one, ref) and r["dim"] == res[1][i] and r["n_kept"] == res[4][i] and r["dir_back"] == res[8][i], v
    with fx.Planner([0, 0]) as p2:                                     # two contexts on device 0: a shard each
        live2, _, (off2, _, _), cs2, _ = four_calls(p2, jobs, pos, goals, home, reso, map_o)
        assert live2 == live and off2.tolist() == off.tolist()
        res2 = call(p2, cs2, paths="resident", offsets=off2)
        per = [t["queries"] for t in p2.timing_per_context()]
        assert sum(per) == len(live) and min(per) > 0, per
        assert same(flat(res2), flat(res))                             # (the kept cells of the second shard included: they start behind the first's)
        for q in range(len(cs2)):
            check(res2, q, exp[q], "two contexts")


def test_st_rule_on_host_threads(planner, golden, monkeypatch):
    """FXJPS_WAYPOINT_ST_HOST=1 (what a table of angles that does not fit falls back to): the st queries' waypoints, Points and
    path3 come from host threads, the ccst queries still from the device, in one mixed batch.  Same bytes as the device form and
    as the host reference, on explicit and on resident paths."""
    cs = shapes_case(planner)
    jobs, pos, goals, home = fleet(golden)
    live, outs, (off, cells, st), fs, _ = four_calls(planner, jobs, pos, goals, home, 0.25, (-2.0, 1.0))
    exp, fexp = [expect(c) for c in cs], [expect(c) for c in fs]
    assert {c["variant"] for c in cs} == {0, 1} and {c["variant"] for c in fs} == {0, 1}
    dev_resident = call(planner, fs, paths="resident", offsets=off)
    dev_explicit = call(planner, cs)
    monkeypatch.setenv("FXJPS_WAYPOINT_ST_HOST", "1")
    host_resident = call(planner, fs, paths="resident", offsets=off)
    host_explicit = call(planner, cs)
    monkeypatch.delenv("FXJPS_WAYPOINT_ST_HOST")
    assert same(flat(host_explicit), flat(dev_explicit)) and same(flat(host_resident), flat(dev_resident))
    for q in range(len(cs)):
        check(host_explicit, q, exp[q], "host form")
    for q in range(len(fs)):
        check(host_resident, q, fexp[q], "host form, resident")
    rc, full = raw(planner, cs[:13])
    monkeypatch.setenv("FXJPS_WAYPOINT_ST_HOST", "1")
    rc2, host = raw(planner, cs[:13])
    assert rc == 0 and rc2 == 0 and all(host[k].tobytes() == full[k].tobytes() for k in full)


def raw(p, cs, **over):
    """The C call itself.  over: argument name -> array / None / int.  -> (rc, the arrays it may have written)"""
    from fuxi_planner_amd import _lib
    n = len(cs)
    off, cells = csr([c["path"] for c in cs])
    tot = int(off[-1])
    a = dict(offsets=off, cells_xy=cells if tot else np.zeros((1, 2), np.int32), grid_ids=np.array([c["map"] for c in cs], np.int32),
             rule=np.array([c["variant"] for c in cs], np.int32), map_start=np.array([c["map_start"] for c in cs], np.int32),
             reso=np.array([c["reso"] for c in cs]), origin=np.array([c["origin"] for c in cs]), pos=np.array([c["pos"] for c in cs]),
             goal=np.array([c["goal"] for c in cs]), end_occu=np.array([c["end_occu"] for c in cs], np.int32), prev_wp=None, prev_dim=None,
             home_xy=np.array([c["home"] for c in cs]), out_wp=np.full((n, 3), 7.5), out_dim=np.full(n, 77, np.int32), out_goal=np.full((n, 3), 7.5),
             out_ang_wp=np.full(n, 7.5), out_n_kept=np.full(n, 77, np.int32), out_kept_cells=np.full((tot + 1, 2), 77, np.int32), kept_capacity=tot,
             out_point=np.full((n, 3), 7.5), out_path_xyz=np.full((tot + 1, 3), 7.5), path_capacity=tot, out_dir_xyz=np.full((tot + 2 * n + 1, 3), 7.5),
             out_dir_n=np.full(n, 77, np.int32), out_dir_back=np.full(n, 77, np.int32), dir_capacity=tot + 2 * n)
    a.update(over)
    order = ["offsets", "cells_xy", "grid_ids", "rule", "map_start", "reso", "origin", "pos", "goal", "end_occu", 2.0, float(np.pi / 4), "prev_wp", "prev_dim",
             "home_xy", "out_wp", "out_dim", "out_goal", "out_ang_wp", "out_n_kept", "out_kept_cells", "kept_capacity", "out_point", "out_path_xyz",
             "path_capacity", "out_dir_xyz", "out_dir_n", "out_dir_back", "dir_capacity"]
    types = p._L.fxjps_tick_outputs_slots.argtypes[2:]
    args = []
    for k, t in zip(order, types):
        v = a[k] if isinstance(k, str) else k
        args.append(v.ctypes.data_as(t) if isinstance(v, np.ndarray) else v)
    rc = p._L.fxjps_tick_outputs_slots(p._h, n, *args, 0)
    return rc, {k: v for k, v in a.items() if k.startswith("out_") and isinstance(v, np.ndarray)}


def test_optional_outputs_and_refusals(planner):
    from fuxi_planner_amd import _lib
    cs = shapes_case(planner)[:13]
    rc, full = raw(planner, cs)
    assert rc == 0 and (full["out_kept_cells"][-1] == 77).all() and (full["out_path_xyz"][-1] == 7.5).all() and (full["out_dir_xyz"][-1] == 7.5).all()
    exp = [expect(c) for c in cs]
    assert full["out_dir_n"].tolist() == [len(e["dir"]) for e in exp] and u64(full["out_point"]).tolist() == u64([e["point"] for e in exp]).tolist()
    off = csr([c["path"] for c in cs])[0]
    for q, e in enumerate(exp):  # the kept cells, behind the two sections of triples in the staged output
        got = full["out_kept_cells"][off[q]:off[q + 1]]
        assert full["out_n_kept"][q] == len(e["kept"]) and got[:len(e["kept"])].tolist() == e["kept"].tolist(), q
        assert (got[len(e["kept"]):] == 77).all(), q
    assert full["out_n_kept"].sum() > 20
    # every optional output in turn, and all of them, left out: the others are what they were
    opt = ["out_dim", "out_goal", "out_ang_wp", "out_n_kept", "out_kept_cells", "out_point", "out_path_xyz", "out_dir_xyz", "out_dir_n", "out_dir_back"]
    for drop in [[k] for k in opt] + [opt, ["out_point", "home_xy"], ["out_dir_xyz", "out_kept_cells"], ["out_path_xyz", "out_dir_xyz", "out_kept_cells"]]:
        rc, got = raw(planner, cs, **{k: None for k in drop})
        assert rc == 0, (drop, planner._L.fxjps_last_error(planner._h))
        assert set(got) == set(full) - set(drop) and all(got[k].tobytes() == full[k].tobytes() for k in got), drop
    # refusals: judged before anything is written, the text names the query
    n, tot = len(cs), sum(len(c["path"]) for c in cs)
    bad = [(dict(home_xy=None), "home_xy"), (dict(path_capacity=tot - 1), "query 12"), (dict(dir_capacity=tot + 2 * n - 1), "query 12"),
           (dict(dir_capacity=3), "query 1:"), (dict(kept_capacity=tot - 1), "out_kept_cells"), (dict(out_wp=None), "bad waypoint"),
           (dict(rule=np.array([0, 1] * 6 + [3], np.int32)), "query 12"), (dict(grid_ids=np.array([EMPTY] * 5 + [200] + [EMPTY] * 7, np.int32)), "query 5"),
           (dict(prev_wp=np.zeros((n, 3))), "prev_wp")]
    for over, text in bad:
        rc, got = raw(planner, cs, **over)
        msg = planner._L.fxjps_last_error(planner._h).decode()
        assert rc == _lib.E_ARG and text in msg, (over.keys(), rc, msg)
        for k, v in got.items():
            assert (v == (77 if v.dtype == np.int32 else 7.5)).all(), (list(over), k)
    rc, again = raw(planner, cs)  # the handle works on, and nothing it holds has changed
    assert rc == 0 and all(again[k].tobytes() == full[k].tobytes() for k in full)
    for s, g in GRIDS.items():
        if s in (EMPTY, SERP):
            assert planner.get_grid_slot(s).tobytes() == g.tobytes()
