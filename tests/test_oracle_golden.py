"""CPU suite: the C oracle (oracle/jps_oracle.c) against the golden vectors captured from the real
jps1.py (tests/golden/make_golden.py), and the synthetic-input generators against each other."""
import hashlib

import numpy as np
import pytest

from conftest import grid_from_bits, load_golden, pairs


def check(oracle, grid, rec, literal=True):
    path, cost, st = oracle.plan(grid, rec["start"], rec["goal"], rec["hchoice"], literal=literal)
    if rec["path"] is None:
        assert path == 0
    else:
        assert path == pairs(rec["path"])
        if rec["start"] != rec["goal"]:
            assert cost.hex() == rec["cost_hex"]            # bit-exact float64
            assert repr(cost) == rec["printed"]             # what jps1.py:207 prints
        else:
            assert rec["printed"] == "0" and cost == 0.0
    if literal and "cells" in rec:
        assert (st["cells"], st["pushes"], st["pops"]) == (rec["cells"], rec["pushes"], rec["pops"])


def test_known_answers(oracle):
    recs = load_golden("known_answers.json")
    assert len(recs) >= 15
    for rec in recs:
        grid = np.array(rec["grid"], dtype=np.float64).reshape(rec["shape"])
        check(oracle, grid, rec)
        check(oracle, grid, rec, literal=False)


def test_start_out_of_bounds_is_an_error(oracle):
    with pytest.raises(ValueError):
        oracle.plan(np.zeros((5, 5)), (5, 5), (1, 1))
    with pytest.raises(ValueError):
        oracle.plan(np.zeros((5, 5)), (-1, 0), (1, 1))
    with pytest.raises(ValueError):
        oracle.plan(np.zeros((5, 5)), (0, 0), (1, 1), hchoice=3)


def test_random_small(oracle):
    recs = load_golden("random_small.json")
    assert len(recs) == 400
    for rec in recs:
        grid = grid_from_bits(rec["grid_bits"], rec["shape"])
        check(oracle, grid, rec)
        check(oracle, grid, rec, literal=False)


FAMILIES = ("empty 60x45", "empty 150x110", "sparse 120x90", "rooms 65x65", "serpentine 34x34", "line 1x200", "line 200x1", "strip 2x90",
            "checkerboard 30x30", "diagonal wall 50x50", "thick diagonal wall 50x50")


def test_families(oracle):
    """The map families the GPU suite leans on (tests/golden/make_golden_families.py): wide-open and 1 % maps, rooms with a
    sealed pocket, the notched serpentine, one- and two-cell-wide grids, a checkerboard, diagonal walls -- path, cost and,
    in literal mode, the reference's cells / pushes / pops on every record."""
    fams = load_golden("families.json")["families"]
    assert tuple(f["family"] for f in fams) == FAMILIES
    n = nopath = 0
    for f in fams:
        grid = grid_from_bits(f["grid_bits"], f["shape"])
        assert len(f["records"]) >= 24 and {r["hchoice"] for r in f["records"]} == {1, 2}, f["family"]
        for rec in f["records"]:
            assert "cells" in rec
            check(oracle, grid, rec)
            check(oracle, grid, rec, literal=False)
            n += 1
            nopath += rec["path"] is None
    assert n == 268 and nopath >= 20, (n, nopath)


def test_reference_maps(oracle, map_grids):
    recs = load_golden("maps_png.json")
    assert len({r["map"] for r in recs}) == 35
    for rec in recs:
        bits = np.unpackbits(map_grids[rec["map"]])
        if "canvas" in rec:
            # BASELINE config 1: the 147x112 snapshot pasted into a zero 256x256 canvas
            occ = np.zeros((256, 256), dtype=np.uint8)
            occ[:147, :112] = bits[:147 * 112].reshape(147, 112)
        else:
            W, H = rec["shape"]
            occ = bits[:W * H].reshape(W, H)
        assert hashlib.sha256(np.ascontiguousarray(occ, dtype=np.uint8).tobytes()).hexdigest() == rec["sha256"]
        check(oracle, occ, rec)


def test_config1_vector_from_survey(oracle, map_grids):
    """(0,0)->(146,111) on the canvas: 37 points, cost 195.49242404917496."""
    rec = [r for r in load_golden("maps_png.json") if "canvas" in r and r["start"] == [0, 0] and r["goal"] == [146, 111]][0]
    assert len(rec["path"]) // 2 == 37 and rec["printed"] == "195.49242404917496"


def test_synth1024(oracle):
    g = load_golden("synth1024.json")
    occ = oracle.synth_grid(g["W"], g["H"], g["grid_seed"], g["p"])
    assert hashlib.sha256(occ.tobytes()).hexdigest() == g["grid_sha256"]
    s, t = oracle.synth_queries(occ, g["qseed"], len(g["queries"]))
    assert hashlib.sha256(s.tobytes()).hexdigest() == g["starts_sha256"]
    assert hashlib.sha256(t.tobytes()).hexdigest() == g["goals_sha256"]
    for i, rec in enumerate(g["queries"]):
        assert rec["start"] == list(map(int, s[i])) and rec["goal"] == list(map(int, t[i]))
        check(oracle, occ, rec)


def test_batch_api_matches_single(oracle):
    occ = oracle.synth_grid(96, 80, 7, 0.25)
    s, t = oracle.synth_queries(occ, 3, 200)
    for lit in (False, True):
        cells, ln, cost, st = oracle.plan_batch(occ, s, t, 2, literal=lit, max_len=512, nthreads=4, want_stats=True)
        for q in range(0, 200, 17):
            path, c, _ = oracle.plan(occ, s[q], t[q], 2, literal=lit)
            if path == 0:
                assert ln[q] == 0
            else:
                assert [tuple(x) for x in cells[q, :ln[q]]] == path and cost[q] == c


def test_fast_mode_counts_equal_the_literal_ones(oracle):
    """The non-literal mode (stale duplicates of closed nodes skipped as the no-ops they are) is what the GPU tests take
    their expected pops and pushes from; only the literal mode's counts are pinned to jps1.py above.  Same pops, pushes
    and open_peak -- and the same paths and costs -- on the inputs of test_search_work_gpu and on synth1024."""
    from fuxi_planner_amd import synth
    cases = [(synth.synth_grid(96, 80, 7, 0.25), 3, 600), (synth.synth_grid(300, 200, 11, 0.02), 11, 400)]
    g = load_golden("synth1024.json")
    cases.append((oracle.synth_grid(g["W"], g["H"], g["grid_seed"], g["p"]), g["qseed"], 24))
    for occ, qseed, n in cases:
        s, t = synth.synth_queries(occ, qseed, n)
        for h in (2, 1):
            lit = oracle.plan_batch(occ, s, t, h, literal=True, max_len=1024, nthreads=8, want_stats=True)
            fast = oracle.plan_batch(occ, s, t, h, literal=False, max_len=1024, nthreads=8, want_stats=True)
            for k in ("pops", "pushes", "open_peak"):
                assert np.array_equal(lit[3][k], fast[3][k]), (occ.shape, h, k)
            assert lit[3]["pops"].sum() > 0 and (lit[3]["cells"] >= fast[3]["cells"]).all()
            assert np.array_equal(lit[1], fast[1]) and lit[2].tobytes() == fast[2].tobytes() and np.array_equal(lit[0], fast[0])


def test_generators_agree(oracle):
    from fuxi_planner_amd import synth
    for W, H, seed, p in [(1024, 1024, 1, 0.2), (100, 37, 5, 0.33), (3, 3, 9, 0.5)]:
        a = synth.synth_grid(W, H, seed, p)
        b = oracle.synth_grid(W, H, seed, p)
        assert np.array_equal(a, b)
        if (a == 0).sum() >= 2:
            sa, ga = synth.synth_queries(a, seed + 1, 300, first=12345)
            sb, gb = oracle.synth_queries(b, seed + 1, 300, first=12345)
            assert np.array_equal(sa, sb) and np.array_equal(ga, gb)
            assert (a[sa[:, 0], sa[:, 1]] == 0).all() and (a[ga[:, 0], ga[:, 1]] == 0).all()
            assert ((sa != ga).any(axis=1)).all()


def test_splitmix_known_values(oracle):
    from fuxi_planner_amd import synth
    L = oracle.lib()
    for x in (0, 1, 2, 0xDEADBEEF, 2**64 - 1):
        assert int(synth.splitmix64(np.array([x], dtype=np.uint64))[0]) == L.fxo_splitmix64(x)
    assert L.fxo_splitmix64(0) == 0xE220A8397B1DCDAF  # published splitmix64 test vector
