"""GPU suite (-m gpu): the planner on EVERY grid of every small shape, every start and every goal, against the real jps1.py.

tests/golden/exhaustive.npz holds digests of the reference's own answers (make_golden_exhaustive.py; the host suite
test_exhaustive_small_host.py ties the C oracle to the same file).  Here the planner's (offsets, cells, cost, status) go
through the same digest functions (exhaustive_cases.py) and must give the same numbers: the planner against jps1.py with no
oracle in between, on all 2^(W*H) grids of the 35 shapes with W * H <= 12 -- goals on the grid and on the ring one cell
outside it -- and all 65 536 grids of 4 x 4, both heuristics.  The kernel answers these from precomputed jump-distance
records with the goal handled on the fly; every 3 x 3 neighbourhood at every border and corner, every goal position
relative to every ray and every occupied start is in there.

The oracle is used for two things only: the pop and push sums of test_search_work_gpu's identity, and to NAME the first
differing query once a digest has differed.  Nothing here reads the reference.
"""
import numpy as np
import pytest

import exhaustive_cases as ex
from test_gpu_fullsize import assert_same, oracle_csr, with_env
from test_search_work_gpu import searched

pytestmark = pytest.mark.gpu
SLOTS = 256  # FXJPS_MAX_GRID_SLOTS: a load is 16 blocks


@pytest.fixture(scope="module")
def fixture():
    return ex.load_fixture()


@pytest.fixture(scope="module")
def planner():
    import fuxi_planner_amd as fx
    p = fx.Planner([0])
    yield p
    p.close()


def grid_part(res, j, nq):
    """(length, cells, cost) of the j-th grid of a call that carried nq queries per grid, grid after grid."""
    off, cells, cost, st = res
    q0, q1 = j * nq, (j + 1) * nq
    return st[q0:q1], cells[off[q0]:off[q1]], cost[q0:q1]


def locate(oracle, W, H, block, h, parts):
    """A block's digest differed: the first query on which the planner and the oracle differ, or that they agree."""
    for code, part in zip(ex.block_codes(W, H, block), parts):
        ol, oc, ocost, _ = ex.oracle_grid(oracle, W, H, code, h)
        msg = ex.first_difference(W, H, code, h, part, (ol, oc, ocost))
        if msg:
            return "planner (got) against oracle (want): " + msg
    return "planner and oracle agree on every query of the block: both differ from the reference"


def check_parts(oracle, arrays, W, H, block, h, parts, what):
    want = int(arrays[ex.array_name("r", W, H, h)][block])
    if ex.result_digest(parts) != want:
        raise AssertionError("%s: result digest of %dx%d hchoice %d block %d (grid codes %d..%d) differs from the reference's; %s"
                             % (what, W, H, h, block, ex.block_codes(W, H, block)[0], ex.block_codes(W, H, block)[-1],
                                locate(oracle, W, H, block, h, parts)))


def run_slots(p, oracle, arrays, W, H, blocks, direct=1):
    """The slots path on `blocks`: 256 grids a load, one call per heuristic with every query of every grid of the load.
    -> (queries sent per heuristic, blocks compared per heuristic)."""
    s1, g1 = ex.queries(W, H)
    nq = len(s1)
    blocks = list(blocks)
    per = len(ex.block_codes(W, H, 0))
    sent, compared = {h: 0 for h in ex.HCHOICES}, {h: 0 for h in ex.HCHOICES}
    for i in range(0, len(blocks), SLOTS // ex.BLOCK):
        load = blocks[i:i + SLOTS // ex.BLOCK]
        codes = [c for b in load for c in ex.block_codes(W, H, b)]
        occs = [ex.grid(W, H, c) for c in codes]
        assert len(codes) <= SLOTS
        p.set_grid_slots(list(enumerate(occs)))  # (the next load overwrites the same slots at equal extents)
        ids = np.repeat(np.arange(len(codes), dtype=np.int32), nq)
        s, g = np.tile(s1, (len(codes), 1)), np.tile(g1, (len(codes), 1))
        is_searched = [searched(occ, s1, g1) for occ in occs]
        for h in ex.HCHOICES:
            res = p.plan_batch_slots(ids, s, g, h, ex.MAX_LEN)
            t = p.timing()
            assert len(res[3]) == len(ids) and len(res[0]) == len(ids) + 1
            sent[h] += len(ids)
            for k, b in enumerate(load):
                check_parts(oracle, arrays, W, H, b, h, [grid_part(res, k * per + j, nq) for j in range(per)], "slots path")
                compared[h] += 1
            assert t["table_direct"] == direct, (W, H, h, t)
            # the work identity of test_search_work_gpu: pops_ref where a query is searched, pushes_ref - 1 there
            assert t["retried"] == 0, (W, H, h, t)
            ref = ex.oracle_blocks(oracle, W, H, load, h)
            stats = [gr[3] for b in load for gr in ref[b]]
            pops = sum(int(st["pops"][m].sum()) for st, m in zip(stats, is_searched))
            pushes = sum(int((st["pushes"][m] - 1).sum()) for st, m in zip(stats, is_searched))
            assert (t["pops"], t["pushes"]) == (pops, pushes), (W, H, h, load[0], load[-1], (t["pops"], t["pushes"]), (pops, pushes))
    return sent, compared


@pytest.mark.parametrize("W,H,chunk", [c[1:] for c in ex.case_ids()], ids=[c[0] for c in ex.case_ids()])
def test_slots_path_equals_the_reference_on_every_grid(planner, oracle, fixture, W, H, chunk):
    arrays, _ = fixture
    blocks = ex.chunk_blocks(W, H, chunk)
    sent, compared = run_slots(planner, oracle, arrays, W, H, blocks)
    if chunk is None:
        want, nb = 2 ** (W * H) * W * H * (W + 2) * (H + 2), ex.n_blocks(W, H)
    else:
        want, nb = 65536 * 256 // ex.CHUNKS_4X4, 4096 // ex.CHUNKS_4X4
    assert sent == {1: want, 2: want} and compared == {1: nb, 2: nb}, (sent, compared, want, nb)


def test_one_mixed_batch_over_every_shape(planner, oracle):
    """36 slots, one grid of each shape (alternating free and occupied cells in flat order), all their queries in one
    shuffled call: the table extents of the batch come from different slots.  Per query against the oracle."""
    grids = {k: ex.grid(W, H, (2 ** (W * H) - 1) // 3) for k, (W, H) in enumerate(ex.SHAPES)}
    planner.set_grid_slots(list(grids.items()))
    ids = np.concatenate([np.full(ex.n_queries(W, H), k, np.int32) for k, (W, H) in enumerate(ex.SHAPES)])
    s = np.concatenate([ex.queries(W, H)[0] for W, H in ex.SHAPES])
    g = np.concatenate([ex.queries(W, H)[1] for W, H in ex.SHAPES])
    perm = np.random.default_rng(20261020).permutation(len(ids))
    ids, s, g = ids[perm], s[perm], g[perm]
    assert len(ids) == sum(ex.n_queries(W, H) for W, H in ex.SHAPES) == 8044
    from test_grid_slots_gpu import subset
    for h in ex.HCHOICES:
        res = planner.plan_batch_slots(ids, s, g, h, ex.MAX_LEN)
        assert planner.timing()["table_direct"] == 1
        n = 0
        for k, occ in grids.items():
            idx = np.flatnonzero(ids == k)
            assert_same(subset(res, idx), oracle_csr(oracle, occ, s[idx], g[idx], h, ex.MAX_LEN, 1))
            n += len(idx)
        assert n == len(ids)


def run_resident(p, oracle, arrays, single):
    """The resident-grid path (k_search without a grid per query) on the 3 x 3 family: each of the 512 grids made resident,
    one plan_batch with its 225 queries per heuristic; with `single`, every 8th grid also sends query code % 225 through
    the one-query call.  -> (queries sent, blocks compared, one-query calls)."""
    W = H = 3
    s1, g1 = ex.queries(W, H)
    sent = compared = singles = 0
    for b in range(ex.n_blocks(W, H)):
        parts = {h: [] for h in ex.HCHOICES}
        for code in ex.block_codes(W, H, b):
            p.set_grid_occ(ex.grid(W, H, code))
            for h in ex.HCHOICES:
                res = p.plan_batch(s1, g1, h, ex.MAX_LEN)
                parts[h].append(grid_part(res, 0, len(s1)))
                sent += len(s1)
                if single and code % 8 == 0:
                    q = code % 225
                    path = p.plan(tuple(s1[q]), tuple(g1[q]), h)
                    off = res[0]
                    assert path == [tuple(c) for c in res[1][off[q]:off[q + 1]].tolist()], (code, q, h, path)
                    assert np.float64(p.last_cost).tobytes() == res[2][q].tobytes(), (code, q, h, p.last_cost, res[2][q])
                    singles += 1
        for h in ex.HCHOICES:
            check_parts(oracle, arrays, W, H, b, h, parts[h], "resident-grid path")
            compared += 1
    return sent, compared, singles


def test_resident_grid_path_on_3x3(planner, oracle, fixture):
    sent, compared, singles = run_resident(planner, oracle, fixture[0], single=True)
    assert (sent, compared, singles) == (2 * 512 * 225, 2 * 32, 2 * 64)


def test_resident_grid_path_streaming_results_on_3x3(oracle, fixture):
    """FXJPS_STREAM_RESULTS=1: the search kernel leaves every finished path in host memory."""
    import fuxi_planner_amd as fx
    with with_env(FXJPS_STREAM_RESULTS=1):
        with fx.Planner([0]) as p:
            sent, compared, _ = run_resident(p, oracle, fixture[0], single=False)
    assert (sent, compared) == (2 * 512 * 225, 2 * 32)


def test_hashed_tables_on_3x3(oracle, fixture):
    """FXJPS_DIRECT=0: the slots path on hashed visited tables."""
    import fuxi_planner_amd as fx
    with with_env(FXJPS_DIRECT=0):
        with fx.Planner([0]) as p:
            sent, compared = run_slots(p, oracle, fixture[0], 3, 3, range(ex.n_blocks(3, 3)), direct=0)
    assert sent == {1: 512 * 225, 2: 512 * 225} and compared == {1: 32, 2: 32}


def test_derived_maps_of_every_3x3_grid(planner):
    """The 512 grids of 3 x 3 in slots (padded extents PW = PH = 5): every derived map against the host computation."""
    from oracle import derived_maps as dm
    n = 0
    for first in range(0, 512, SLOTS):
        occs = [ex.grid(3, 3, c) for c in range(first, first + SLOTS)]
        planner.set_grid_slots(list(enumerate(occs)))
        for slot, occ in enumerate(occs):
            dev = planner.debug_slot_maps(slot)
            msg = dm.first_difference(dev, dm.reference_maps(occ))
            assert msg is None, (first + slot, occ.tolist(), msg)
            msg = dm.component_problem(dev["comp"], occ, exact=True)
            assert msg is None, (first + slot, occ.tolist(), "comp", msg)
            n += 1
    assert n == 512
