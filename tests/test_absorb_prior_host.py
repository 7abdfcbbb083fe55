"""CPU suite of fxjps_absorb_prior: worldprep.absorb_host -- the host form, and what the GPU suite
compares the device with -- pinned to the canvases of tests/golden/worldprep.json, which come from executing the reference's
own slice assignments; the three modes on hand-made cases; the header, the binding and the library agree; every whole-call
refusal fires in fxjps_absorb_check, the call's argument check without a handle.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from worldprep_cases import cases, placements

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def args(c, **kw):
    return dict(dict(prior=c["prior"], ori_pre=c["ori_pre"], raw=c["raw"], map_o=c["map_o"], map_reso=c["reso"]), **kw)


def test_overwrite_is_the_reference_canvas_cut_to_the_prior():
    from fuxi_planner_amd import worldprep
    done = changing = off_by_one = 0
    for i, c in enumerate(cases()):
        if c["raises"] or c["prior"] is None:
            continue
        at = [int(q) for q in placements(c)]
        pw, ph = c["prior"].shape
        want = c["canvas"][at[2]:at[2] + pw, at[3]:at[3] + ph]
        new, inside, outside, changed = worldprep.absorb_host(**args(c))
        assert new.dtype == np.uint8 and new.shape == (pw, ph) and np.array_equal(new, want), i
        assert inside + outside == c["raw"].size and inside >= 0 and outside >= 0, i
        assert changed == int(np.count_nonzero((new != 0) != (c["prior"] != 0))), i
        # the message form of the same detected map
        m = c["raw"]
        msg = np.where(m == 1, 100, m).astype(np.int8).T.reshape(-1)
        again = worldprep.absorb_host(**args(c, raw=(msg, m.shape[0], m.shape[1])))
        assert np.array_equal(again[0], new) and again[1:] == (inside, outside, changed), i
        done += 1
        changing += changed > 0
        off_by_one += any(int(q) != int(round(q)) for q in placements(c))
    assert done == 88 and changing >= 30 and off_by_one >= 30, (done, changing, off_by_one)


def test_cases_whose_canvas_raises_are_still_absorbed():
    from fuxi_planner_amd import worldprep
    seen = 0
    for i, c in enumerate(cases()):
        if not c["raises"] or c["prior"] is None:
            continue
        try:
            new, inside, outside, changed = worldprep.absorb_host(**args(c))
        except ValueError:
            # only what absorb_prior refuses as well: a quotient outside int32, a non-finite origin, a bad resolution
            o1 = [min(c["map_o"][k], c["ori_pre"][k]) for k in range(2)]
            q = placements(c)
            assert not all(np.isfinite(q)) or max(abs(v) for v in q) >= 2147483648.0 or not (np.isfinite(c["reso"]) and c["reso"] > 0), (i, o1)
            continue
        assert inside + outside == c["raw"].size and 0 <= inside <= c["prior"].size, i
        assert new.shape == c["prior"].shape, i
        seen += 1
    assert seen >= 5


def test_modes_on_hand_made_cases():
    from fuxi_planner_amd.worldprep import absorb_host
    prior = np.array([[0, 1, 255, 0], [1, 0, 0, 100], [0, 0, 1, 1], [255, 1, 0, 0], [0, 0, 0, 7]], dtype=np.uint8)  # 5 x 4
    ori = (0.0, 0.0)
    # job A: 3 x 3 at prior cell (1, 0); job B: 3 x 3 at (2, 1), over A's lower right
    A = np.array([[1, 0, 1], [0, 0, 1], [1, 1, 0]], dtype=np.uint8)
    B = np.array([[1, 0, 0], [1, 0, 0], [0, 0, 1]], dtype=np.uint8)
    oA, oB = (1.0, 0.0), (2.0, 1.0)
    # ---- overwrite: the later job wins where both cover; an untouched 255 survives; changed counts flips, not byte changes
    p1, ins, out, ch = absorb_host(prior, ori, A, oA, 1.0)
    assert (ins, out) == (9, 0)
    want = prior.copy()
    want[1:4, 0:3] = A
    assert np.array_equal(p1, want) and p1[0, 2] == 255 and p1[3, 0] == 1   # (3, 0): 255 -> 1 is a byte change ...
    assert ch == int(np.count_nonzero((want != 0) != (prior != 0))) and (prior[3, 0] != 0) == (p1[3, 0] != 0)  # ... and no flip
    p2, ins, out, ch2 = absorb_host(p1, ori, B, oB, 1.0)
    assert (ins, out) == (9, 0)
    want2 = want.copy()
    want2[2:5, 1:4] = B
    assert np.array_equal(p2, want2)
    # the other order gives another result where the two overlap and differ
    q1 = absorb_host(prior, ori, B, oB, 1.0)[0]
    q2 = absorb_host(q1, ori, A, oA, 1.0)[0]
    assert not np.array_equal(q2, p2) and np.array_equal(q2[1:4, 0:3], A)
    # a rectangle sticking out: dropped cells are counted, the prior does not grow
    p3, ins, out, _ = absorb_host(prior, ori, np.ones((3, 3), dtype=np.uint8), (3.0, 2.0), 1.0)
    assert (ins, out) == (4, 5) and p3.shape == prior.shape and np.array_equal(p3[3:5, 2:4], np.ones((2, 2)))
    p4, ins, out, ch = absorb_host(prior, ori, np.ones((3, 3), dtype=np.uint8), (9.0, 9.0), 1.0)
    assert (ins, out, ch) == (0, 9, 0) and np.array_equal(p4, prior)
    # lo / win: only the named rectangle of raw, whose origin map_o is
    p5, ins, out, _ = absorb_host(prior, ori, A, (0.0, 0.0), 1.0, lo=(1, 1), win=(2, 2))
    want5 = prior.copy()
    want5[0:2, 0:2] = A[1:3, 1:3]
    assert (ins, out) == (4, 0) and np.array_equal(p5, want5)
    # ---- occupied never clears, and leaves the bytes of occupied cells it does not set
    p6, _, _, ch = absorb_host(prior, ori, A, oA, 1.0, mode="occupied")
    want6 = prior.copy()
    want6[1:4, 0:3][A > 0] = 1
    assert np.array_equal(p6, want6) and np.all((p6 != 0) >= (prior != 0)) and p6[1, 3] == 100
    assert ch == int(np.count_nonzero((p6 != 0) & (prior == 0)))
    # ---- known: -1 cells of a message are skipped, so an earlier job's value (or the prior's byte) stays
    mA = np.array([[100, 0, -1], [-1, 0, 100], [100, -1, 0]], dtype=np.int8)  # [x][y] of a 3 x 3 message
    msgA = (mA.T.reshape(-1), 3, 3)
    mB = np.array([[-1, 100, -1], [0, -1, -1], [-1, -1, 0]], dtype=np.int8)
    msgB = (mB.T.reshape(-1), 3, 3)
    k1 = absorb_host(prior, ori, msgA, oA, 1.0, mode="known")[0]
    want7 = prior.copy()
    sub = want7[1:4, 0:3]
    sub[mA != -1] = (mA > 0)[mA != -1]
    assert np.array_equal(k1, want7) and k1[3, 1] == prior[3, 1] and k1[1, 2] == prior[1, 2]
    k2 = absorb_host(k1, ori, msgB, oB, 1.0, mode="known")[0]
    want8 = want7.copy()
    sub = want8[2:5, 1:4]
    sub[mB != -1] = (mB > 0)[mB != -1]
    assert np.array_equal(k2, want8)
    assert k2[2, 1] == k1[2, 1] == 0 and mB[0, 0] == -1 and mA[1, 1] == 0    # B unknown there: A's value stands
    assert k2[4, 3] == 0 and prior[4, 3] == 7                               # a known free cell clears a 7
    # overwrite on a message: unknown counts as free
    w1 = absorb_host(prior, ori, msgA, oA, 1.0)[0]
    assert np.array_equal(w1[1:4, 0:3], (mA > 0).astype(np.uint8))
    # a matrix has no unknown cells: known is overwrite there
    assert np.array_equal(absorb_host(prior, ori, A, oA, 1.0, mode="known")[0], p1)


def test_absorb_host_refuses_what_the_library_refuses():
    from fuxi_planner_amd.worldprep import absorb_host
    ok = dict(prior=np.zeros((6, 6), dtype=np.uint8), ori_pre=[-2.0, -2.0], raw=np.ones((4, 5), dtype=np.uint8), map_o=[-1.0, -1.0], map_reso=0.5)
    absorb_host(**ok)
    for bad in (dict(mode="union"), dict(map_reso=0.0), dict(map_reso=-1.0), dict(map_reso=float("nan")), dict(map_reso=float("inf")),
                dict(map_o=[float("nan"), 0.0]), dict(ori_pre=[0.0, float("inf")]), dict(map_o=[4e9, 0.0]), dict(ori_pre=[0.0, -4e9]),
                dict(lo=(0, 0), win=(0, 3)), dict(lo=(-1, 0), win=(2, 2)), dict(lo=(2, 2), win=(3, 2)), dict(lo=(0, 4), win=(1, 2)),
                dict(raw=np.zeros((0, 3))), dict(raw=np.zeros((8191, 1), dtype=np.uint8)), dict(raw=(np.zeros(5, dtype=np.int8), 2, 3)),
                dict(prior=np.zeros((0, 2)))):
        with pytest.raises(ValueError):
            absorb_host(**dict(ok, **bad))


def test_header_binding_and_library_agree():
    import __graft_entry__
    from fuxi_planner_amd import _lib
    __graft_entry__.build()
    hdr = open(os.path.join(ROOT, "include", "fxjps.h")).read()
    version = int(re.search(r"#define FXJPS_VERSION (\d+)", hdr).group(1))
    assert version >= 850 and _lib.VERSION == version
    assert re.search(r"^ \*\s+850\s+fxjps_absorb_prior", hdr, re.M), "no changelog line for version 850"
    for name, val in (("OVERWRITE", 0), ("OCCUPIED", 1), ("KNOWN", 2)):
        assert int(re.search(r"#define FXJPS_ABSORB_%s\s+(\d+)" % name, hdr).group(1)) == val == getattr(_lib, "ABSORB_" + name)
    L = C.CDLL(_lib.LIB_PATH)
    assert L.fxjps_version() == version
    assert L.fxjps_absorb_job_size() == C.sizeof(_lib.AbsorbJob) == 104
    for name in ("fxjps_absorb_prior", "fxjps_absorb_check", "fxjps_absorb_job_size"):
        assert re.search(r"\bint %s\s*\(" % name, hdr) and hasattr(L, name) and name in _lib.SYMBOLS, name
    # the struct field by field
    body = re.search(r"typedef struct fxjps_absorb_job \{(.*?)\} fxjps_absorb_job_t;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.match(r"\s*(\w+)", nm).group(1) for _, decl in re.findall(r"(const void\*|int32_t|int64_t|double)\s+([^;]+);", body) for nm in decl.split(",")]
    assert names == [f[0] for f in _lib.AbsorbJob._fields_]
    src = open(os.path.join(ROOT, "fuxi-planner_amd", "csrc", "fxjps_maps.hip.inc")).read()
    assert re.search(r"__global__[^\n]*\bvoid k_prior_absorb\(", src)
    # a NULL handle is refused before anything else
    L.fxjps_absorb_prior.restype = C.c_int
    L.fxjps_absorb_prior.argtypes = [C.c_void_p, C.POINTER(_lib.AbsorbJob), C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
    assert L.fxjps_absorb_prior(None, None, 0, 0, None) == _lib.E_ARG


def make_job(buf, **kw):
    from fuxi_planner_amd import _lib
    j = _lib.AbsorbJob()
    j.raw, j.layout, j.W0, j.H0 = buf.ctypes.data, 0, 6, 8
    j.lo[0], j.lo[1], j.win[0], j.win[1] = 0, 0, 6, 8
    j.prior, j.map_reso = 2, 0.5
    j.map_o[0], j.map_o[1], j.ori_pre[0], j.ori_pre[1] = 1.0, -1.0, 0.0, 0.0
    for k, v in kw.items():
        if isinstance(v, tuple):
            for i, x in enumerate(v):
                getattr(j, k)[i] = x
        else:
            setattr(j, k, v)
    return j


def test_every_refusal_fires_in_the_argument_check():
    import __graft_entry__
    from fuxi_planner_amd import _lib
    __graft_entry__.build()
    L = _lib.load()
    raw = np.zeros((6, 8), dtype=np.uint8)
    wh = np.zeros(2 * _lib.MAX_PRIOR_MAPS, dtype=np.int32)
    wh[4:6] = (10, 12)   # prior 2 is set
    wh[6:8] = (8190, 8190)
    p_wh = _lib.ptr(wh, C.c_int32)
    msg = C.create_string_buffer(400)

    def check(jobs, n=None, mode=0, extents=p_wh):
        arr = (_lib.AbsorbJob * max(len(jobs), 1))(*jobs)
        rc = L.fxjps_absorb_check(arr if jobs is not None else None, len(jobs) if n is None else n, mode, extents, msg, len(msg))
        return rc, msg.value.decode(), arr

    rc, text, arr = check([make_job(raw), make_job(raw, map_o=(-2.0, 5.0)), make_job(raw, map_o=(40.0, 0.0))])
    assert rc == 0 and text == ""
    # 6 x 8 at prior cell (2, -2): y 0 .. 5 of 8 inside; at (-4, 10): x 0 .. 1, y 10 .. 11; at (80, 0): disjoint, no error
    assert [(a.inside, a.outside) for a in arr] == [(36, 12), (4, 44), (0, 48)]
    assert check([], 0)[0] == 0
    nan, inf = float("nan"), float("inf")
    bad = [("n", dict(n=-1)), ("n", dict(n=257)), ("mode", dict(mode=3)), ("mode", dict(mode=-1)), ("extents", dict(extents=None)),
           ("raw", dict(raw=None)), ("layout", dict(layout=2)), ("layout", dict(layout=-1)), ("extents", dict(W0=0)), ("extents", dict(H0=8191)),
           ("rectangle", dict(win=(0, 8))), ("rectangle", dict(win=(6, -1))), ("rectangle", dict(lo=(-1, 0))), ("rectangle", dict(lo=(1, 0))),
           ("rectangle", dict(lo=(0, 3), win=(2, 6))), ("rectangle", dict(lo=(2147483647, 0), win=(2147483647, 1))),
           ("prior", dict(prior=-1)), ("prior", dict(prior=16)), ("not set", dict(prior=5)),
           ("non-finite", dict(map_o=(nan, 0.0))), ("non-finite", dict(map_o=(0.0, inf))), ("non-finite", dict(ori_pre=(-inf, 0.0))),
           ("map_reso", dict(map_reso=0.0)), ("map_reso", dict(map_reso=-0.5)), ("map_reso", dict(map_reso=nan)), ("map_reso", dict(map_reso=inf)),
           ("int32", dict(map_o=(2e9, 0.0))), ("int32", dict(ori_pre=(0.0, 1.5e9)))]
    for word, kw in bad:
        call = {k: kw.pop(k) for k in ("n", "mode", "extents") if k in kw}
        good = make_job(raw)
        jobs = [good, make_job(raw, **kw)] if kw else [good, good]
        before = [(j.inside, j.outside) for j in jobs]
        rc, text, arr = check(jobs, **call)
        assert rc == _lib.E_ARG and word in text, (word, kw, call, rc, text)
        assert text.startswith("job 1:" if kw else "job 0:"), text
        assert [(a.inside, a.outside) for a in arr] == before  # a refused call writes nothing
    # more than 2^30 staged bytes: 17 rectangles of 8190 x 8190 that meet their prior (the raw is never read by the check)
    big = np.zeros(1, dtype=np.uint8)
    jobs = [make_job(big, W0=8190, H0=8190, win=(8190, 8190), prior=3, map_o=(0.0, 0.0)) for _ in range(17)]
    rc, text, _ = check(jobs)
    assert rc == _lib.E_ARG and "2^30" in text and text.startswith("job 16:"), text
    # ... and none when they miss it: nothing is staged for a rectangle wholly outside
    rc, text, arr = check([make_job(big, W0=8190, H0=8190, win=(8190, 8190), prior=3, map_o=(5000.0, 0.0)) for _ in range(17)])
    assert rc == 0 and all(a.inside == 0 and a.outside == 8190 * 8190 for a in arr)
    # the check and absorb_host place a rectangle alike, off-by-one truncations included
    from fuxi_planner_amd import worldprep
    n = 0
    for c in cases():
        if c["prior"] is None or c["raises"]:
            continue
        m = np.ascontiguousarray(c["raw"] > 0, dtype=np.uint8)
        ext = np.zeros(2 * _lib.MAX_PRIOR_MAPS, dtype=np.int32)
        ext[0:2] = c["prior"].shape
        j = make_job(m, W0=m.shape[0], H0=m.shape[1], win=m.shape, prior=0, map_reso=c["reso"], map_o=tuple(c["map_o"]), ori_pre=tuple(c["ori_pre"]))
        rc, text, arr = check([j], extents=_lib.ptr(ext, C.c_int32))
        assert rc == 0, text
        assert (arr[0].inside, arr[0].outside) == worldprep.absorb_host(c["prior"], c["ori_pre"], c["raw"], c["map_o"], c["reso"])[1:3]
        n += 1
    assert n == 88
