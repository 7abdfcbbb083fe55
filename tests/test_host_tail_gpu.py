"""GPU suite (-m gpu): the host tail -- the first queries of a batch's longest-first order searched by host threads beside
the device search (FXJPS_HOST_TAIL=64, set per call).

Every batch here has 4 096 queries, the smallest at which the tail (and the head launch it rides on) is on.  Offsets, cells,
float64 cost bytes and status must be byte for byte those of the same call under FXJPS_HOST_TAIL=0 and those of the CPU
oracle; timing()'s pops and pushes must be equal on both sides; host_tail_queries must be 64 with the tail and 0 without."""
import numpy as np
import pytest

from test_gpu_fullsize import assert_same, oracle_csr, with_env

pytestmark = pytest.mark.gpu
NTHREADS = 16
NQ = 4096
ON, OFF = {"FXJPS_HOST_TAIL": 64}, {"FXJPS_HOST_TAIL": 0}


@pytest.fixture(scope="module")
def planner():
    import fuxi_planner_amd as fx
    p = fx.Planner([0])
    yield p
    p.close()


def make(W, H, seed, p):
    from fuxi_planner_amd import synth
    occ = synth.synth_grid(W, H, seed, p)
    s, g = synth.synth_queries(occ, seed, NQ)
    return occ, s.astype(np.int32).copy(), g.astype(np.int32).copy()


@pytest.fixture(scope="module")
def dense():
    return make(96, 80, 31, 0.20)


@pytest.fixture(scope="module")
def sparse():
    return make(300, 200, 32, 0.02)


def both(planner, s, g, h, max_len):
    """The batch with the tail and without: -> (result, timing) of each, after the checks that hold for every batch."""
    with with_env(**ON):
        on = planner.plan_batch(s, g, h, max_len)
        t_on = planner.timing()
    with with_env(**OFF):
        off = planner.plan_batch(s, g, h, max_len)
        t_off = planner.timing()
    assert_same(on, off)
    assert t_on["host_tail_queries"] == 64 and t_off["host_tail_queries"] == 0, (t_on, t_off)
    assert t_on["host_tail_ms"] > 0 and t_off["host_tail_ms"] == 0, (t_on, t_off)
    assert t_on["table_direct"] == 1 and t_on["search_launches"] == t_off["search_launches"], (t_on, t_off)
    assert t_on["retried"] == 0 and t_off["retried"] == 0, (t_on, t_off)
    assert (t_on["pops"], t_on["pushes"]) == (t_off["pops"], t_off["pushes"]), (t_on, t_off)
    return on, t_on


@pytest.mark.parametrize("name,h", [("dense", 2), ("sparse", 2), ("dense", 1)])
def test_same_bytes_as_without_and_as_the_oracle(planner, oracle, request, name, h):
    occ, s, g = request.getfixturevalue(name)
    planner.set_grid_occ(occ)
    on, _ = both(planner, s, g, h, 512)
    assert_same(on, oracle_csr(oracle, occ, s, g, h, 512, NTHREADS))
    assert (on[3] > 1).sum() > NQ // 2


def test_cell_update_between_two_batches(planner, oracle, dense):
    """The second batch runs on the updated grid: host maps of the first batch's generation would give other paths."""
    occ, s, g = dense
    planner.set_grid_occ(occ)
    both(planner, s, g, 2, 512)
    rng = np.random.default_rng(33)
    xy = np.stack([rng.integers(0, occ.shape[0], 600), rng.integers(0, occ.shape[1], 600)], -1).astype(np.int32)
    _, first = np.unique(xy[:, 0] * occ.shape[1] + xy[:, 1], return_index=True)
    xy = xy[np.sort(first)]
    val = (1 - occ[xy[:, 0], xy[:, 1]]).astype(np.uint8)  # every named cell toggles
    occ2 = occ.copy()
    occ2[xy[:, 0], xy[:, 1]] = val
    before = oracle_csr(oracle, occ, s, g, 2, 512, NTHREADS)
    want = oracle_csr(oracle, occ2, s, g, 2, 512, NTHREADS)
    key = 2 * np.maximum(abs(s - g)[:, 0], abs(s - g)[:, 1]) + np.minimum(abs(s - g)[:, 0], abs(s - g)[:, 1])
    head = np.argsort(-key, kind="stable")[:64]  # the host's queries
    assert (before[3][head] != want[3][head]).any() or (before[2][head] != want[2][head]).any()
    planner.update_cells(xy, val)
    on, _ = both(planner, s, g, 2, 512)
    assert_same(on, want)
    planner.update_cells(xy, 1 - val, rebuild=False)  # ... and back, the maps rebuilt by the batch itself
    on, _ = both(planner, s, g, 2, 512)
    assert_same(on, before)


def test_special_outcomes_in_the_host_share(planner, oracle, sparse):
    """The first 64 of the order hold: a start off the grid, goals off the grid, an occupied goal, a goal nothing leads to,
    paths longer than their slot, and -- all but 40 queries of the batch being start == goal, which sort last -- start ==
    goal on free cells and on an obstacle."""
    occ, s, g = sparse
    occ = occ.copy()
    W, H = occ.shape
    occ[W - 4:W - 1, H - 4:H - 1] = 1
    occ[W - 3, H - 3] = 0  # a free cell nothing leads to
    occ[0, 0] = 0
    occ[W - 1, H - 1] = 1
    s, g = s.copy(), g.copy()
    s[40:] = g[40:]
    wall = np.argwhere(occ == 1)
    s[41], g[41] = wall[0], wall[0]
    s[0], g[0] = [0, 0], [W - 3, H - 3]
    s[1], g[1] = [0, 0], [W - 1, H - 1]
    s[2], g[2] = [0, 0], [W, H - 1]
    s[3], g[3] = [0, 0], [-1, H + 7]
    s[4], g[4] = [-1, 3], [W - 2, 5]
    planner.set_grid_occ(occ)
    for max_len in (512, 3):
        on, _ = both(planner, s, g, 2, max_len)
        assert_same(on, oracle_csr(oracle, occ, s, g, 2, max_len, NTHREADS))  # (a start off the grid: -2 on both sides)
        st = on[3]
        assert st[0] == 0 and st[1] == 0 and st[2] == 0 and st[3] == 0 and st[4] == -2 and st[41] == 1 and (st[40:] == 1).all()
        if max_len == 3:
            assert (st[5:40] == -1).any()

