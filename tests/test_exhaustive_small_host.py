"""CPU suite: the C oracle on EVERY grid of every small shape, every start and every goal, against the real jps1.py.

tests/golden/exhaustive.npz (make_golden_exhaustive.py) holds, per block of 16 grids and per heuristic, a digest of the
reference's paths and costs and a digest of its (grid reads, pushes, pops).  Here the oracle runs the same queries --
all 2^(W*H) grids of the 35 shapes with W * H <= 12, goals on the grid and on the ring one cell outside it, and all 65 536
grids of 4 x 4 -- and must reproduce every digest: results in memoised and in literal mode, the three counts in literal
mode (the mode that reads the grid as the reference does); memoised pushes and pops must equal the literal ones.  Every
3 x 3 neighbourhood at every border and corner, every goal position relative to every ray, every occupied start is in
there, with no sampling.  Enumeration and digests come from exhaustive_cases.py, shared with the generator and the GPU suite.
"""
import numpy as np
import pytest

import exhaustive_cases as ex


@pytest.fixture(scope="module")
def fixture():
    return ex.load_fixture()


def test_fixture_is_complete(fixture):
    arrays, meta = fixture
    assert [tuple(s) for s in meta["shapes"]] == list(ex.SHAPES) and len(ex.SHAPES) == 36
    assert meta["recipe"] == ex.RECIPE and meta["block"] == ex.BLOCK and tuple(meta["hchoices"]) == ex.HCHOICES
    names = set()
    for W, H in ex.SHAPES:
        nm = ex.shape_name(W, H)
        assert meta["blocks"][nm] == ex.n_blocks(W, H) and meta["queries_per_grid"][nm] == ex.n_queries(W, H)
        assert meta["queries"][nm] == ex.shape_queries(W, H)
        for h in ex.HCHOICES:
            assert 0 < meta["no_path"]["%s_h%d" % (nm, h)] < ex.shape_queries(W, H)
            for kind in "rw":
                a = arrays[ex.array_name(kind, W, H, h)]
                assert a.dtype == np.dtype("<u8") and a.shape == (ex.n_blocks(W, H),), (kind, nm, h, a.dtype, a.shape)
                assert len(np.unique(a)) == len(a), (kind, nm, h)  # (no two blocks of a shape hold the same records)
                names.add(ex.array_name(kind, W, H, h))
    assert names == set(arrays)
    assert meta["queries"]["4x4"] == 16777216 and sum(meta["queries"].values()) * 2 == 61604804


def check_oracle(oracle, arrays, W, H, blocks):
    """-> (queries digested per heuristic, no-path records per heuristic)."""
    nq, nopath = {}, {}
    for h in ex.HCHOICES:
        memo = ex.oracle_blocks(oracle, W, H, blocks, h, literal=False)
        lit = ex.oracle_blocks(oracle, W, H, blocks, h, literal=True)
        want_r, want_w = arrays[ex.array_name("r", W, H, h)], arrays[ex.array_name("w", W, H, h)]
        nq[h] = nopath[h] = 0
        for b in blocks:
            where = "%dx%d hchoice %d block %d (grid codes %d..%d)" % (W, H, h, b, ex.block_codes(W, H, b)[0], ex.block_codes(W, H, b)[-1])
            assert ex.result_digest(g[:3] for g in memo[b]) == int(want_r[b]), "memoised oracle, result digest of " + where
            assert ex.result_digest(g[:3] for g in lit[b]) == int(want_r[b]), "literal oracle, result digest of " + where
            assert ex.work_digest((g[3]["cells"], g[3]["pushes"], g[3]["pops"]) for g in lit[b]) == int(want_w[b]), \
                "literal oracle, work digest of " + where
            for m, l in zip(memo[b], lit[b]):
                assert np.array_equal(m[3]["pushes"], l[3]["pushes"]) and np.array_equal(m[3]["pops"], l[3]["pops"]), where
                nq[h] += len(m[0])
                nopath[h] += int((m[0] == 0).sum())
    return nq, nopath


@pytest.mark.parametrize("W,H,chunk", [c[1:] for c in ex.case_ids()], ids=[c[0] for c in ex.case_ids()])
def test_oracle_equals_the_reference_on_every_grid(oracle, fixture, W, H, chunk):
    arrays, meta = fixture
    blocks = ex.chunk_blocks(W, H, chunk)
    nq, nopath = check_oracle(oracle, arrays, W, H, blocks)
    if chunk is None:
        want = 2 ** (W * H) * W * H * (W + 2) * (H + 2)
        assert len(blocks) == ex.n_blocks(W, H)
        for h in ex.HCHOICES:
            assert nopath[h] == meta["no_path"]["%s_h%d" % (ex.shape_name(W, H), h)]
    else:
        want = 65536 * 256 // ex.CHUNKS_4X4
        assert (W, H) == (4, 4) and len(blocks) == 256
    assert nq == {1: want, 2: want}, (nq, want)


def test_python_restatement_equals_the_oracle_on_3x3(oracle):
    """oracle/jps_python.py (the benchmark's CPU baseline) on all 512 grids of 3 x 3, the ring goals included, both
    heuristics: path, cost bits, pushes and pops equal the C oracle's, which the test above ties to the reference."""
    from oracle import jps_python as jp
    W = H = 3
    s, g = ex.queries(W, H)
    starts, goals = [tuple(v) for v in s.tolist()], [tuple(v) for v in g.tolist()]
    n = 0
    for h in ex.HCHOICES:
        ref = ex.oracle_blocks(oracle, W, H, range(ex.n_blocks(W, H)), h, literal=True)
        for b in range(ex.n_blocks(W, H)):
            for code, (ol, oc, ocost, ost) in zip(ex.block_codes(W, H, b), ref[b]):
                m = ex.grid(W, H, code).astype(np.float64)
                off = np.concatenate([[0], np.cumsum(ol)])
                for q in range(len(starts)):
                    st = {}
                    path, cost, _ = jp.search(m, starts[q], goals[q], h, st)
                    want = [tuple(c) for c in oc[off[q]:off[q + 1]].tolist()]
                    where = (code, starts[q], goals[q], h)
                    assert (path if path != 0 else []) == want and (path == 0) == (ol[q] == 0), (where, path, want)
                    assert np.float64(0.0 if path == 0 else cost).tobytes() == ocost[q].tobytes(), (where, cost, float(ocost[q]))
                    assert (st["pushes"], st["pops"]) == (int(ost["pushes"][q]), int(ost["pops"][q])), (where, st)
                    n += 1
    assert n == 2 * 512 * 9 * 25
