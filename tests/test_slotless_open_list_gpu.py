"""GPU suite (-m gpu): the slotless open list of the untracked searches on cell-indexed tables.

On those tables a node's table slot is a function of its cell, so the open list carries no slot: not in the register tier,
not in LDS, and a far-tier entry holds {f, (x, y, direction), cell info} (DESIGN.md sections 2 and 3.1).  A slot derived
wrongly, or a cell info that a far entry brings back wrongly, changes a relaxation: the cells, the cost, or at the least
the number of pops and pushes.  So one small grid whose queries provably spill into the far tier is planned

  * on cell-indexed tables, both heuristics (hchoice 1 is the tie-heavy one: it fills the open list and keeps the commit's
    collision detector and the second round's sieve busy), against the oracle: cells, lengths, float64 cost bytes, per-query
    pops, the batch's pops and pushes -- and for each of the far-tier queries planned alone, ITS pops and pushes;
  * in a second child process with FXJPS_DIRECT=0 (hashed tables: the carrying layout), the same queries, the same checks;
  * as one batch of 4 608 short queries, so that the head launch runs with the block's new LDS size.

The helpers (the reference, the identity pops_gpu == pops_ref, pushes_gpu == pushes_ref - 1, the scenario runner) are those
of test_search_work_gpu.py; FXJPS_QSTAT=1 switches the single-call path off for a whole process, hence the children.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_search_work_gpu as work
from test_search_work_gpu import MPL, TIERS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE, P_OCC, GRID_SEED = 192, 0.10, 21  # the reference meets far_queries() >= 8 here (64 and 62 of the 64 queries): not grown
NQ, CORNER = 64, 12                      # corner-to-corner queries: starts and goals within CORNER cells of opposite corners
NHEAD, REACH = 4608, 12                  # the head-launch batch: goals within REACH cells of their start
MIN_FAR = 8


def grid():
    from fuxi_planner_amd import synth
    return synth.synth_grid(SIDE, SIDE, GRID_SEED, P_OCC)


def corner_queries(occ):
    """NQ queries from free cells near (0, 0) to free cells near (W - 1, H - 1), every second one the other way round."""
    W, H = occ.shape
    rng = np.random.default_rng(5)
    lo = np.argwhere(occ[:CORNER, :CORNER] == 0)
    hi = np.argwhere(occ[W - CORNER:, H - CORNER:] == 0) + [W - CORNER, H - CORNER]
    s = lo[rng.integers(0, len(lo), NQ)].astype(np.int32)
    g = hi[rng.integers(0, len(hi), NQ)].astype(np.int32)
    s[1::2], g[1::2] = g[1::2].copy(), s[1::2].copy()
    return s, g


def short_queries(occ):
    """NHEAD queries between free cells at most REACH cells apart on either axis."""
    W, H = occ.shape
    rng = np.random.default_rng(6)
    free = np.argwhere(occ == 0)
    s = free[rng.integers(0, len(free), NHEAD)]
    g = s.copy()
    todo = np.arange(NHEAD)
    while len(todo):  # (a goal that falls on an obstacle or off the grid is drawn again)
        c = s[todo] + rng.integers(-REACH, REACH + 1, (len(todo), 2))
        ok = (c >= 0).all(axis=1) & (c[:, 0] < W) & (c[:, 1] < H)
        ok[ok] = occ[c[ok, 0], c[ok, 1]] == 0
        g[todo[ok]] = c[ok]
        todo = todo[~ok]
    return s.astype(np.int32), g.astype(np.int32)


def register_inputs():
    """The two batches under names of their own in test_search_work_gpu's table of inputs."""
    occ = grid()
    work._inputs.setdefault("slotless corners", (occ,) + corner_queries(occ))
    work._inputs.setdefault("slotless short", (occ,) + short_queries(occ))


def far_queries(ref):
    """Queries whose open list at the goal is provably beyond the two fast tiers: pushes_ref - pops_ref > R + M."""
    return np.flatnonzero(ref["searched"] & (ref["ref_pushes"] - ref["ref_pops"] > TIERS))


def check_far_condition(oracle):
    """The condition the grid was chosen by, from the reference alone -- for both heuristics."""
    register_inputs()
    out = {}
    for h in (2, 1):
        ref = work.expected(oracle, "slotless corners", h)
        far = far_queries(ref)
        assert len(far) >= MIN_FAR, ("the far tier is not provably used", h, len(far),
                                     np.sort(ref["ref_pushes"] - ref["ref_pops"])[-MIN_FAR:].tolist())
        assert ref["searched"].all(), h
        out[h] = far
    return out


# (test_search_work_gpu's scenario records: name, inputs, kind, environment, heuristics, far tier, retries, path slot)
def scenarios(hashed):
    env = {"FXJPS_DIRECT": "0"} if hashed else {}
    tag = "hashed " if hashed else ""
    sc = [("%sslotless corners %dx%d" % (tag, SIDE, SIDE), "slotless corners", "batch", env, (2, 1), False, False, MPL)]
    if not hashed:
        sc.append(("slotless head launch %dx%d" % (SIDE, SIDE), "slotless short", "head", env, (2, 1), False, False, MPL))
    return sc


def child_main(hashed):
    """One process under FXJPS_QSTAT=1: the scenarios, then every far-tier query alone.  One line each."""
    assert os.environ.get("FXJPS_QSTAT") == "1" and (os.environ.get("FXJPS_DIRECT") == "0") == hashed
    import fuxi_planner_amd as fx
    from oracle import oracle
    oracle.build()
    far = check_far_condition(oracle)
    failed = 0
    for sc in scenarios(hashed):
        for h in sc[4]:
            line, bad = work.run_scenario(fx, oracle, sc, h)
            if not hashed and "table_direct 0" in line:
                bad.append("the tables are not indexed by the cell")
            print(("work ok  " if not bad else "work BAD ") + line, flush=True)
            for b in bad:
                print("    " + b, flush=True)
            failed += bool(bad)
    occ, s, g = work.inputs("slotless corners")
    with fx.Planner([0]) as p:
        p.set_grid_occ(occ)
        for h in (2, 1):
            ref = work.expected(oracle, "slotless corners", h)
            wrong = []
            for q in far[h]:
                p.plan_batch(s[q:q + 1], g[q:q + 1], h, MPL)
                t = p.timing()
                got, want = (t["pops"], t["pushes"]), (int(ref["pops"][q]), int(ref["pushes"][q]))
                if got != want or t["retried"] != 0:
                    wrong.append((int(q), got, want, t["retried"]))
            print("%s h=%d: %d far-tier queries alone, (pops, pushes) differ on %d %s" % (
                "alone ok " if not wrong else "alone BAD", h, len(far[h]), len(wrong), wrong[:4]), flush=True)
            failed += bool(wrong)
    if failed:
        sys.exit("%d checks failed" % failed)


def run_child(hashed):
    env = dict(os.environ, FXJPS_QSTAT="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    env.pop("FXJPS_DIRECT", None)
    if hashed:
        env["FXJPS_DIRECT"] = "0"
    r = subprocess.run([sys.executable, "-c", "import test_slotless_open_list_gpu as t; t.child_main(%r)" % hashed], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=240)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stdout[-6000:], r.stderr[-4000:])
    for sc in scenarios(hashed):
        for h in sc[4]:
            assert "work ok  %s h=%d:" % (sc[0], h) in r.stdout, (sc[0], h, r.stdout[-6000:])
    for h in (2, 1):
        assert "alone ok  h=%d:" % h in r.stdout, (h, r.stdout[-6000:])


def test_the_far_tier_is_provably_used(oracle):
    """From the reference alone: for at least 8 queries of the batch the open list at the goal holds more than R + M
    entries, under either heuristic -- so a later change of the generator cannot hollow the tests below out."""
    far = check_far_condition(oracle)
    print({h: len(v) for h, v in far.items()})


def test_cell_indexed_tables_against_the_oracle():
    """The slotless layout: results, per-query pops, batch sums, the far-tier queries' own pops and pushes, and the head
    launch (two launches, the block with its new LDS size beside the 36 KB pad) on 4 608 short queries."""
    run_child(hashed=False)


def test_hashed_tables_give_the_same():
    """FXJPS_DIRECT=0 in a child process: the carrying layout on the same queries, against the same reference."""
    run_child(hashed=True)
