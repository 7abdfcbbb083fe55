"""GPU suite (-m gpu): what the planning calls refuse, in which order, and what a refused call leaves alone.

fxjps_plan_batch, fxjps_plan_batch_csr, fxjps_plan_batch_slots_csr, fxjps_replan_slots and fxjps_set_queries are driven
through the raw ctypes bindings, so that NULL arrays and counts the Python wrappers never pass reach the library.  Every
refusal is pinned by its code AND by a fragment of its text (fxjps_last_error): where an input is wrong in two ways the text
says which of the two the call judged first -- a slots call its ids before its query arrays, a resident call the missing
grid before anything else.  The expected codes and texts are what the library gave before the planning calls were folded
onto one request record (the file passes against that build, loaded through FXJPS_LIB).

The grids: 8 x 8 with one wall (resident), 12 x 5 with one wall (slot 0); at most four queries."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_fullsize import assert_same, oracle_csr

pytestmark = pytest.mark.gpu
MPL = 64
EMPTY_SLOT = 5
I32, I64, F64 = C.c_int32, C.c_int64, C.c_double


def grid8():
    g = np.zeros((8, 8), np.uint8)
    g[4, 0:6] = 1
    return g


def grid12x5():
    g = np.zeros((12, 5), np.uint8)
    g[6, 1:5] = 1
    return g


RES_S = np.array([(0, 0), (1, 2), (7, 7), (0, 7)], np.int32)
RES_G = np.array([(7, 0), (6, 3), (0, 0), (7, 7)], np.int32)
SLOT_S = np.array([(0, 4), (11, 0), (2, 2)], np.int32)
SLOT_G = np.array([(11, 4), (0, 0), (9, 3)], np.int32)
SLOT_IDS = np.zeros(3, np.int32)
CALLS = ("plan_batch", "plan_batch_csr", "plan_batch_slots_csr", "replan_slots", "set_queries")
SLOT_CALLS = ("plan_batch_slots_csr", "replan_slots")
RESIDENT_CALLS = ("plan_batch", "plan_batch_csr")


@pytest.fixture(scope="module")
def planner():
    import fuxi_planner_amd as fx
    p = fx.Planner([0])
    p.set_grid(grid8())
    p.set_grid_slot(0, grid12x5())
    yield p
    p.close()


def raw_call(p, call, nq, hchoice, mpl, ids=SLOT_IDS, s=None, g=None, outs=True):
    """One planning entry point with exactly these arguments (None: NULL) -> (return code, fxjps_last_error's text)."""
    from fuxi_planner_amd import _lib
    L, h = p._L, p._h
    slots = call in SLOT_CALLS
    if s is None:
        s, g = (SLOT_S, SLOT_G) if slots else (RES_S, RES_G)
    ptr = lambda a, ty: None if a is None or a is False else _lib.ptr(a, ty)  # noqa: E731
    off, ln, cost, reused = np.zeros(8, np.int64), np.zeros(8, np.int32), np.zeros(8), np.zeros(8, np.int32)
    o_off, o_len, o_cost = (off, ln, cost) if outs else (None, None, None)
    if call == "plan_batch":  # (no cells array: the dense form of a (1 << 20) + 1 slot would be the test's to allocate)
        rc = L.fxjps_plan_batch(h, ptr(s, I32), ptr(g, I32), nq, hchoice, mpl, None, ptr(o_len, I32), ptr(o_cost, F64), None)
    elif call == "plan_batch_csr":
        rc = L.fxjps_plan_batch_csr(h, ptr(s, I32), ptr(g, I32), nq, hchoice, mpl, ptr(o_off, I64), None, 0, ptr(o_len, I32), ptr(o_cost, F64), None)
    elif call == "plan_batch_slots_csr":
        rc = L.fxjps_plan_batch_slots_csr(h, ptr(ids, I32), ptr(s, I32), ptr(g, I32), nq, hchoice, mpl, ptr(o_off, I64), None, 0, ptr(o_len, I32),
                                          ptr(o_cost, F64), None)
    elif call == "replan_slots":
        rc = L.fxjps_replan_slots(h, ptr(ids, I32), ptr(s, I32), ptr(g, I32), nq, hchoice, mpl, ptr(o_off, I64), None, 0, ptr(o_len, I32),
                                  ptr(o_cost, F64), ptr(reused, I32), None)
    else:
        rc = L.fxjps_set_queries(h, ptr(s, I32), ptr(g, I32), nq, hchoice, mpl)
    return rc, (L.fxjps_last_error(h) or b"").decode()


def refusals():
    """(call, keyword arguments of raw_call, the text's fragment); every one of them is FXJPS_E_ARG."""
    ids_with = lambda bad: np.array([0, bad, 0], np.int32)  # noqa: E731
    t = []
    for call in CALLS:
        n = 3 if call in SLOT_CALLS else 4
        for h in (0, 3):
            t.append((call, dict(nq=n, hchoice=h, mpl=MPL), "hchoice must be 1 or 2"))
        for m in (0, (1 << 20) + 1):
            t.append((call, dict(nq=n, hchoice=2, mpl=m), "max_path_len out of range"))
        t.append((call, dict(nq=-1, hchoice=2, mpl=MPL), "bad query arrays"))
        t.append((call, dict(nq=1, hchoice=2, mpl=MPL, s=False, g=RES_G), "bad query arrays"))
        t.append((call, dict(nq=1, hchoice=2, mpl=MPL, s=RES_S, g=False), "bad query arrays"))
        # wrong in two ways: the arrays before the heuristic, the heuristic before the length
        t.append((call, dict(nq=1, hchoice=3, mpl=MPL, s=False, g=RES_G), "bad query arrays"))
        t.append((call, dict(nq=-1, hchoice=0, mpl=0), "bad query arrays"))
        t.append((call, dict(nq=n, hchoice=3, mpl=0), "hchoice must be 1 or 2"))
        if call != "set_queries":  # ... and a call's own output arrays before all of them
            t.append((call, dict(nq=n, hchoice=3, mpl=MPL, outs=False), "NULL output array"))
    for call in RESIDENT_CALLS:  # (refused before an array is read; a slots call reads its ids first, fxjps_set_queries copies)
        t.append((call, dict(nq=0x7FFFFFF1, hchoice=2, mpl=MPL), "too many queries in one batch"))
    for call in SLOT_CALLS:
        t.append((call, dict(nq=3, hchoice=2, mpl=MPL, ids=ids_with(EMPTY_SLOT)), "query 1 names grid slot 5, which is empty"))
        for bad in (-1, 256):
            t.append((call, dict(nq=3, hchoice=2, mpl=MPL, ids=ids_with(bad)), "query 1 names grid slot %d, which is out of range" % bad))
        t.append((call, dict(nq=1, hchoice=2, mpl=MPL, ids=None), "NULL grid_ids"))
        # wrong in two ways: the ids before the query arrays and before the heuristic
        t.append((call, dict(nq=3, hchoice=2, mpl=MPL, ids=ids_with(EMPTY_SLOT), s=False, g=SLOT_G), "names grid slot 5"))
        t.append((call, dict(nq=3, hchoice=3, mpl=0, ids=ids_with(256)), "names grid slot 256"))
        t.append((call, dict(nq=1, hchoice=3, mpl=MPL, ids=None, s=False, g=SLOT_G), "NULL grid_ids"))
    return t


def test_refusal_table(planner, oracle):
    from fuxi_planner_amd import _lib
    want_res = oracle_csr(oracle, grid8(), RES_S, RES_G, 2, MPL, 1)
    want_slot = oracle_csr(oracle, grid12x5(), SLOT_S, SLOT_G, 2, MPL, 1)
    table = refusals()
    assert len(table) == 5 * 10 + 4 + 2 + 2 * 7
    for call, kw, text in table:
        rc, err = raw_call(planner, call, **kw)
        print(call, kw.get("nq"), kw.get("hchoice"), kw.get("mpl"), "->", rc, err)
        assert rc == _lib.E_ARG and text in err, (call, kw, rc, err)
    # the handle goes on, on both kinds of grid
    assert_same(planner.plan_batch(RES_S, RES_G, 2, MPL), want_res)
    assert_same(planner.plan_batch_slots(SLOT_IDS, SLOT_S, SLOT_G, 2, MPL), want_slot)


def test_no_grid_is_judged_first_and_only_on_the_resident_grid(oracle):
    """A handle that has a slot but never had a resident grid: the resident calls refuse with FXJPS_E_NOGRID whatever else
    is wrong with their arguments; the slots calls plan; fxjps_set_queries stores (it is the frame that needs the grid)."""
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import _lib
    want_slot = oracle_csr(oracle, grid12x5(), SLOT_S, SLOT_G, 2, MPL, 1)
    with fx.Planner([0]) as p:
        p.set_grid_slot(0, grid12x5())
        for call in RESIDENT_CALLS:
            for kw in (dict(nq=4, hchoice=2, mpl=MPL), dict(nq=4, hchoice=3, mpl=MPL), dict(nq=1, hchoice=2, mpl=0, s=False, g=RES_G),
                       dict(nq=-1, hchoice=2, mpl=MPL)):
                rc, err = raw_call(p, call, **kw)
                print(call, kw.get("nq"), kw.get("hchoice"), kw.get("mpl"), "->", rc, err)
                assert rc == _lib.E_NOGRID and "before fxjps_set_grid" in err, (call, kw, rc, err)
        rc, err = raw_call(p, "plan_batch_csr", nq=4, hchoice=2, mpl=MPL, outs=False)  # (but its own output arrays before the grid)
        assert rc == _lib.E_ARG and "NULL output array" in err, (rc, err)
        for call in SLOT_CALLS:
            assert raw_call(p, call, nq=3, hchoice=2, mpl=MPL)[0] == _lib.OK, call
            assert_same((p.replan_slots if call == "replan_slots" else p.plan_batch_slots)(SLOT_IDS, SLOT_S, SLOT_G, 2, MPL)[:4], want_slot)
        assert raw_call(p, "set_queries", nq=4, hchoice=2, mpl=MPL)[0] == _lib.OK
        # an empty slots batch may pass no array at all
        assert raw_call(p, "plan_batch_slots_csr", nq=0, hchoice=2, mpl=MPL, ids=None, s=False, g=False, outs=False)[0] == _lib.OK


def as_bytes(res):
    return [np.ascontiguousarray(a).tobytes() for a in res]


def test_a_refused_call_changes_nothing(planner):
    from fuxi_planner_amd import _lib, waypoints
    ccst = lambda n: waypoints.select_ccst_batch(planner, n, 0.1, (0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 0.0))  # noqa: E731
    for n in (4, 1):  # (a batch, and the single call, whose paths stay in the pinned host buffers)
        planner.plan_batch(RES_S[:n], RES_G[:n], 2, MPL)
        before = as_bytes(ccst(n))
        for kw in (dict(nq=n, hchoice=3, mpl=MPL), dict(nq=n, hchoice=2, mpl=0), dict(nq=n, hchoice=2, mpl=MPL, s=False, g=RES_G)):
            for call in RESIDENT_CALLS + ("set_queries",):
                assert raw_call(planner, call, **kw)[0] == _lib.E_ARG
        assert as_bytes(ccst(n)) == before
    # ... and a slots batch that fxjps_replan_slots stored
    sel = lambda: waypoints.select_slots_batch(planner, ["st", "ccst", "st"], (1, 1), 0.1, (0.0, 0.0), (0.0, 0.0, 0.0), (1.0, 0.4, 0.0))  # noqa: E731
    first = planner.replan_slots(SLOT_IDS, SLOT_S, SLOT_G, 2, MPL)
    assert not first[4].any()
    before = as_bytes(sel())
    bad_ids = np.array([0, EMPTY_SLOT, 0], np.int32)
    for kw in (dict(nq=3, hchoice=3, mpl=MPL), dict(nq=3, hchoice=2, mpl=0), dict(nq=3, hchoice=2, mpl=MPL, ids=bad_ids),
               dict(nq=3, hchoice=2, mpl=MPL, s=False, g=SLOT_G), dict(nq=3, hchoice=2, mpl=MPL, outs=False)):
        for call in SLOT_CALLS:
            assert raw_call(planner, call, **kw)[0] == _lib.E_ARG
    assert as_bytes(sel()) == before
    again = planner.replan_slots(SLOT_IDS, SLOT_S, SLOT_G, 2, MPL)
    assert again[4].all() and planner.timing()["reused"] == 3
    assert_same(again[:4], first[:4])


def test_extents_belong_to_the_request(planner, oracle):
    """resident, slots, resident on one handle: each batch is sized by its own grid (8 x 8, 12 x 5, 8 x 8)."""
    import fuxi_planner_amd as fx
    alone = {}
    with fx.Planner([0]) as p:
        p.set_grid(grid8())
        p.plan_batch(RES_S, RES_G, 2, MPL)
        alone["resident"] = p.timing()["table_direct"]
    with fx.Planner([0]) as p:
        p.set_grid_slot(0, grid12x5())
        p.plan_batch_slots(SLOT_IDS, SLOT_S, SLOT_G, 2, MPL)
        alone["slots"] = p.timing()["table_direct"]
    a = planner.plan_batch(RES_S, RES_G, 2, MPL)
    ta = planner.timing()["table_direct"]
    b = planner.plan_batch_slots(SLOT_IDS, SLOT_S, SLOT_G, 2, MPL)
    tb = planner.timing()["table_direct"]
    c = planner.plan_batch(RES_S, RES_G, 2, MPL)
    tc = planner.timing()["table_direct"]
    assert as_bytes(a) == as_bytes(c)
    assert_same(a, oracle_csr(oracle, grid8(), RES_S, RES_G, 2, MPL, 1))
    assert_same(b, oracle_csr(oracle, grid12x5(), SLOT_S, SLOT_G, 2, MPL, 1))
    assert (b[3] > 0).all() and (b[1][:, 0] >= 8).any()  # (paths that leave the resident grid's 8 columns)
    assert (ta, tb, tc) == (alone["resident"], alone["slots"], alone["resident"])
