"""CPU suite: the host side of tests/test_search_work_gpu.py -- the predicate that says which queries the kernel searches,
against the oracle's own counts and results, and what every scenario must be before a GPU is asked."""
import numpy as np
import pytest

from test_search_work_gpu import EDGE_CLASSES, SCENARIOS, check_oracle_side, components, edge_classes, expected, inputs, searched


def test_flood_fill_equals_the_oracles_components(oracle):
    for name in ("small", "rooms"):
        occ = inputs(name)[0]
        a, b = components(occ), oracle.components(occ)
        assert np.array_equal(a >= 0, b >= 0)
        # (the same partition under two numberings)
        pairs = np.unique(np.stack([a[a >= 0], b[b >= 0]], 1), axis=0)
        assert len(pairs) == len(np.unique(a[a >= 0])) == len(np.unique(b[b >= 0]))
    occ = np.array([[0, 1, 0], [1, 1, 0], [0, 0, 0]], dtype=np.uint8)
    lab = components(occ)
    assert lab[0, 0] != lab[0, 2] and lab[0, 2] == lab[2, 0] == lab[1, 2] and lab[0, 1] == -1


def test_searched_predicate_on_the_edge_batch(oracle):
    """A query the predicate leaves out and whose start is in the grid has no path or start == goal; a searched query pops
    at least once; the classes are what they are called."""
    occ, s, g = inputs("edge")
    W, H = occ.shape
    cls = edge_classes(occ, s, g)
    assert tuple(cls) == EDGE_CLASSES
    for h in (2, 1):
        ref = expected(oracle, "edge", h)
        m, ln = ref["searched"], ref["csr"][3]
        check_oracle_side("edge", ref, edge=True)
        s_in = (s[:, 0] >= 0) & (s[:, 0] < W) & (s[:, 1] >= 0) & (s[:, 1] < H)
        same = (s == g).all(axis=1)
        assert ((ln[~m & s_in] <= 0) | same[~m & s_in]).all()
        assert (ln[~s_in] == -2).all() and (ref["ref_pops"][~s_in] == 0).all()
        assert (ref["ref_pops"][m] >= 1).all()
        assert np.array_equal(m, cls["occupied start"] & ~same)  # (the one searched class of this batch)
        assert (ln[same & s_in] == 1).all() and (ln[cls["goal in another component"]] == 0).all()
        assert (ln[cls["occupied start"]] > 0).sum() >= 10  # (an occupied start is a start like any other)
        assert (ref["pops"][~m] == 0).all() and (ref["pushes"][~m] == 0).all()


@pytest.mark.parametrize("inp", sorted({sc[1] for sc in SCENARIOS} - {"edge"}))
def test_scenarios_are_what_the_gpu_test_needs(oracle, inp):
    """The conditions test_search_work_gpu checks in front of every scenario, on the CPU alone."""
    for sc in SCENARIOS:
        if sc[1] == inp:
            for h in sc[4]:
                check_oracle_side(inp, expected(oracle, inp, h, sc[7]), far=sc[5])
    if inp == "rooms":
        occ, s, g = inputs(inp)
        m = searched(occ, s, g)
        assert not m[:30].any() and m[30:].sum() >= 760  # (goals into the sealed pocket, starts out of it)
