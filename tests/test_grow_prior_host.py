"""CPU suite of fxjps_absorb_prior_grow: worldprep.grow_host -- the host form of one job, and what
the GPU suite folds to compare the device with -- pinned to the canvases of tests/golden/worldprep.json, which come from
executing the reference's own lines; the three modes, a shift on both axes and a fold whose order matters on hand-made
cases; fxjps_grow_check, the call's geometry and refusals without a handle, against the grow_host fold on random job lists;
every whole-call refusal; the header, the binding and the library agree.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from worldprep_cases import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def args(c, **kw):
    return dict(dict(prior=c["prior"], ori_pre=c["ori_pre"], raw=c["raw"], map_o=c["map_o"], map_reso=c["reso"], map_t=c["map_t"]), **kw)


def host_fold(before, jobs, mode, crops=None):
    """grow_host job by job on copies of `before` ({prior: bytes}); jobs are world jobs as Planner.absorb_prior_grow takes
    them, ori_pre the origin BEFORE the fold.  -> (after, origin, shift, at, changed): per named prior the grown bytes, the
    new origin, where old cell (0, 0) lies and the cells whose occupancy differs from the old byte at that place (counted
    directly, on the old prior laid into the final frame); per job where its cell (0, 0) lies in the final frame."""
    from fuxi_planner_amd import worldprep
    cur = {k: np.array(v, dtype=np.uint8) for k, v in before.items()}
    origin, shift, at = {}, {}, []
    for v, wj in enumerate(jobs):
        raw, map_o, reso, prior, ori_pre = wj[1], wj[2], wj[3], wj[8], wj[9]
        map_t = wj[10] if len(wj) > 10 else None
        rec = crops[v] if crops is not None else None
        lo, win = (None, None) if rec is None else (rec["lo"], rec["win"])
        if rec is not None:
            map_o, map_t = rec["map_o"], rec["map_t"]
        new, o1, sh, a, _ = worldprep.grow_host(cur[prior], origin.get(prior, ori_pre), raw, map_o, reso, mode, lo=lo, win=win, map_t=map_t)
        for i, earlier in enumerate(jobs[:v]):  # (the earlier rectangles move with the old prior)
            if earlier[8] == prior:
                at[i] = (at[i][0] + sh[0], at[i][1] + sh[1])
        s = shift.get(prior, (0, 0))
        shift[prior] = (s[0] + sh[0], s[1] + sh[1])
        cur[prior], origin[prior] = new, list(o1)
        at.append((a[0], a[1]))
    changed = {}
    for k in origin:
        old = np.zeros(cur[k].shape, dtype=np.uint8)
        w, h = before[k].shape
        old[shift[k][0]:shift[k][0] + w, shift[k][1]:shift[k][1] + h] = before[k]
        changed[k] = int(np.count_nonzero((cur[k] != 0) != (old != 0)))
    return cur, origin, shift, at, changed


def as_message(m):
    m = np.asarray(m)
    return (np.where(m == 1, 100, m).astype(np.int8).T.reshape(-1), m.shape[0], m.shape[1])


def test_overwrite_is_the_reference_canvas():
    from fuxi_planner_amd import worldprep
    done = growing = 0
    for i, c in enumerate(cases()):
        if c["raises"] or c["prior"] is None:
            continue
        for form in (c["raw"], as_message(c["raw"])):  # the matrix and the message of the same detected map
            new, o1, shift, at, changed = worldprep.grow_host(**args(c, raw=form))
            assert new.dtype == np.uint8 and new.shape == tuple(c["canvas_shape"]), (i, new.shape, c["canvas_shape"])
            assert np.array_equal(new, c["canvas"]), i
            assert [float(x) for x in o1] == c["canvas_o"], (i, o1, c["canvas_o"])
            pw, ph = c["prior"].shape
            old = np.zeros(new.shape, dtype=np.uint8)
            old[shift[0]:shift[0] + pw, shift[1]:shift[1] + ph] = c["prior"]
            assert changed == int(np.count_nonzero((new != 0) != (old != 0))), i
            rw, rh = c["raw"].shape
            assert np.array_equal(new[at[0]:at[0] + rw, at[1]:at[1] + rh], c["raw"] > 0), i
        done += 1
        growing += new.shape != c["prior"].shape
    assert done == 88 and growing >= 60, (done, growing)


def test_cases_whose_canvas_raises_still_grow():
    from fuxi_planner_amd import worldprep
    seen = bigger = 0
    for i, c in enumerate(cases()):
        if not c["raises"] or c["prior"] is None:
            continue
        new, o1, shift, at, _ = worldprep.grow_host(**args(c))
        reso = c["reso"]
        for k in range(2):  # size as the issue defines it, written out once more
            o, op, W, win = c["map_o"][k], c["ori_pre"][k], c["prior"].shape[k], c["raw"].shape[k]
            m = min(o, op)
            ref = int((max(op + reso * W, c["map_t"][k]) - m) / reso)
            assert at[k] == int((o - m) / reso) and shift[k] == int((op - m) / reso) and o1[k] == m, (i, k)
            assert new.shape[k] == max(ref, shift[k] + W, at[k] + win), (i, k)
        pw, ph = c["prior"].shape
        rw, rh = c["raw"].shape
        assert np.array_equal(new[at[0]:at[0] + rw, at[1]:at[1] + rh], c["raw"] > 0), i
        outside = np.ones(new.shape, dtype=bool)
        outside[at[0]:at[0] + rw, at[1]:at[1] + rh] = False
        old = np.zeros(new.shape, dtype=np.uint8)
        old[shift[0]:shift[0] + pw, shift[1]:shift[1] + ph] = c["prior"]
        assert np.array_equal(new[outside], old[outside]), i
        seen += 1
        bigger += any(new.shape[k] > int((max(c["ori_pre"][k] + reso * c["prior"].shape[k], c["map_t"][k]) - o1[k]) / reso) for k in range(2))
    assert seen == 16 and bigger >= 1, (seen, bigger)


def test_inside_cases_keep_shape_and_origin():
    from fuxi_planner_amd import worldprep
    seen = 0
    for i, c in enumerate(cases()):
        if c["prior"] is None or c["raises"] or c["arrange"] != "inside":
            continue
        for mode in ("overwrite", "occupied", "known"):
            new, o1, shift, at, changed = worldprep.grow_host(**args(c, mode=mode))
            want, inside, outside, want_changed = worldprep.absorb_host(c["prior"], c["ori_pre"], c["raw"], c["map_o"], c["reso"], mode)
            assert outside == 0 and new.shape == c["prior"].shape and [float(x) for x in o1] == c["ori_pre"] and tuple(shift) == (0, 0), i
            assert np.array_equal(new, want) and changed == want_changed, (i, mode)
        seen += 1
    assert seen == 10


def test_modes_shifts_and_a_255_on_hand_made_cases():
    from fuxi_planner_amd.worldprep import grow_host
    prior = np.array([[0, 1, 255, 0], [1, 0, 0, 100], [0, 0, 1, 1]], dtype=np.uint8)  # 3 x 4 at (0, 0), reso 1
    ori = (0.0, 0.0)
    # ---- growth on the low side of both axes at once: a 2 x 3 rectangle at world (-2, -1)
    A = np.array([[1, 0, 1], [0, 1, 1]], dtype=np.uint8)
    new, o1, shift, at, changed = grow_host(prior, ori, A, (-2.0, -1.0), 1.0)
    assert list(o1) == [-2.0, -1.0] and tuple(shift) == (2, 1) and tuple(at) == (0, 0) and new.shape == (5, 5)
    want = np.zeros((5, 5), dtype=np.uint8)
    want[2:5, 1:5] = prior
    placed = want.copy()
    want[0:2, 0:3] = A
    assert np.array_equal(new, want)
    assert new[2, 3] == 255 and new[3, 4] == 100                 # a 255 carried through the shift, byte for byte
    assert changed == int(np.count_nonzero((want != 0) != (placed != 0))) == 4
    # ---- growth on the high side: shift stays 0, the rectangle lands at its offset
    new, o1, shift, at, _ = grow_host(prior, ori, A, (2.0, 3.0), 1.0)
    assert list(o1) == [0.0, 0.0] and tuple(shift) == (0, 0) and tuple(at) == (2, 3) and new.shape == (4, 6)
    assert np.array_equal(new[:3, :4][np.array([[1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 0]], dtype=bool)],
                          prior[np.array([[1, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 0]], dtype=bool)]) and new[2, 3] == 1
    # ---- the three modes with -1 cells: a 3 x 3 message at world (1, 2), over the prior's upper right and beyond
    m = np.array([[100, 0, -1], [-1, 0, 100], [0, -1, 100]], dtype=np.int8)  # [x][y]
    msg = (m.T.reshape(-1), 3, 3)
    base = np.zeros((4, 5), dtype=np.uint8)
    base[:3, :4] = prior
    w = grow_host(prior, ori, msg, (1.0, 2.0), 1.0, "overwrite")[0]
    want = base.copy()
    want[1:4, 2:5] = m > 0                                       # unknown counts as free
    assert w.shape == (4, 5) and np.array_equal(w, want) and w[1, 3] == 0 and prior[1, 3] == 100
    o = grow_host(prior, ori, msg, (1.0, 2.0), 1.0, "occupied")[0]
    want = base.copy()
    want[1:4, 2:5][m > 0] = 1
    assert np.array_equal(o, want) and o[1, 3] == 100 and o[0, 2] == 255     # occupied never clears, nor touches what it does not set
    k = grow_host(prior, ori, msg, (1.0, 2.0), 1.0, "known")[0]
    want = base.copy()
    want[1:4, 2:5][m != -1] = (m > 0)[m != -1]
    assert np.array_equal(k, want) and k[2, 2] == 1 and m[1, 0] == -1 and k[1, 3] == 0   # -1 keeps the byte, a known free cell clears a 100
    assert k[3, 3] == 0 and m[2, 1] == -1                        # -1 over a cell the old prior did not have: 0
    # a matrix has no unknown cells: known is overwrite there
    assert np.array_equal(grow_host(prior, ori, A, (-2.0, -1.0), 1.0, "known")[0], grow_host(prior, ori, A, (-2.0, -1.0), 1.0)[0])
    # lo / win: only the named rectangle of raw, whose origin map_o is
    new, _, shift, at, _ = grow_host(prior, ori, np.ones((5, 5), dtype=np.uint8), (3.0, 0.0), 1.0, lo=(1, 2), win=(2, 2))
    assert new.shape == (5, 4) and tuple(at) == (3, 0) and new[3:5, 0:2].all() and new.sum() == prior.astype(int).sum() + 4
    # map_t beyond the rectangle grows the prior as the reference's canvas does
    assert grow_host(prior, ori, A, (0.0, 0.0), 1.0, map_t=(7.0, 2.0))[0].shape == (7, 4)


def test_a_fold_of_three_jobs_whose_order_matters():
    prior = np.zeros((4, 4), dtype=np.uint8)
    one, nil = np.ones((3, 3), dtype=np.uint8), np.zeros((3, 3), dtype=np.uint8)

    def wj(raw, x, y):
        return (0, raw, (float(x), float(y)), 1.0, (0.0, 0.0), (0.0, 0.0), 0, 1, 0, (0.0, 0.0))

    a, b, c = wj(one, -2, 1), wj(nil, -1, 2), wj(one, 3, -2)
    got = {}
    for name, order in (("abc", (a, b, c)), ("bac", (b, a, c)), ("cab", (c, a, b))):
        after, origin, shift, at, changed = host_fold({0: prior}, list(order), "overwrite")
        got[name] = after[0]
        assert after[0].shape == (8, 7) and origin[0] == [-2.0, -2.0] and shift[0] == (2, 2), name
        for (job, where) in zip(order, at):  # every rectangle's final placement: its world origin minus the final origin
            assert where == (int(job[2][0] + 2), int(job[2][1] + 2)), (name, where)
        assert changed[0] == int(np.count_nonzero(after[0])), name
    assert got["abc"][1:3, 4:6].sum() == 0 and got["bac"][1:3, 4:6].sum() == 4   # where a and b overlap the later one wins
    assert np.array_equal(got["abc"], got["cab"]) and not np.array_equal(got["abc"], got["bac"])
    # occupied does not depend on the order
    assert np.array_equal(host_fold({0: prior}, [a, b, c], "occupied")[0][0], host_fold({0: prior}, [b, a, c], "occupied")[0][0])


def test_grow_host_refuses_what_the_library_refuses():
    from fuxi_planner_amd.worldprep import grow_host
    ok = dict(prior=np.zeros((6, 6), dtype=np.uint8), ori_pre=[-2.0, -2.0], raw=np.ones((4, 5), dtype=np.uint8), map_o=[-1.0, -1.0], map_reso=0.5)
    grow_host(**ok)
    for bad in (dict(mode="union"), dict(map_reso=0.0), dict(map_reso=-1.0), dict(map_reso=float("nan")), dict(map_reso=float("inf")),
                dict(map_o=[float("nan"), 0.0]), dict(ori_pre=[0.0, float("inf")]), dict(map_o=[4e9, 0.0]), dict(ori_pre=[0.0, -4e9]),
                dict(map_t=[float("nan"), 0.0]), dict(map_t=[0.0, float("inf")]), dict(map_t=[4e9, 0.0]), dict(map_o=[5000.0, 0.0]),
                dict(lo=(0, 0), win=(0, 3)), dict(lo=(-1, 0), win=(2, 2)), dict(lo=(2, 2), win=(3, 2)), dict(lo=(0, 4), win=(1, 2)),
                dict(raw=np.zeros((0, 3))), dict(raw=np.zeros((8191, 1), dtype=np.uint8)), dict(raw=(np.zeros(5, dtype=np.int8), 2, 3)),
                dict(prior=np.zeros((0, 2)))):
        with pytest.raises(ValueError):
            grow_host(**dict(ok, **bad))


def test_header_binding_and_library_agree():
    import __graft_entry__
    from fuxi_planner_amd import _lib
    __graft_entry__.build()
    hdr = open(os.path.join(ROOT, "include", "fxjps.h")).read()
    version = int(re.search(r"#define FXJPS_VERSION (\d+)", hdr).group(1))
    assert version >= 860 and _lib.VERSION == version
    assert re.search(r"^ \*\s+860\s+fxjps_absorb_prior_grow", hdr, re.M), "no changelog line for version 860"
    L = C.CDLL(_lib.LIB_PATH)
    assert L.fxjps_version() == version
    assert L.fxjps_grow_job_size() == C.sizeof(_lib.GrowJob) == 128
    assert L.fxjps_prior_grown_size() == C.sizeof(_lib.PriorGrown) == 48
    for name in ("fxjps_absorb_prior_grow", "fxjps_grow_check", "fxjps_grow_job_size", "fxjps_prior_grown_size"):
        assert re.search(r"\bint %s\s*\(" % name, hdr) and hasattr(L, name) and name in _lib.SYMBOLS, name
    # the structs field by field; the grow job begins with the absorb job's fields
    for struct, binding in (("grow_job", _lib.GrowJob), ("prior_grown", _lib.PriorGrown)):
        body = re.search(r"typedef struct fxjps_%s \{(.*?)\} fxjps_%s_t;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [re.match(r"\s*(\w+)", nm).group(1) for _, decl in re.findall(r"(const void\*|int32_t|int64_t|double)\s+([^;]+);", body) for nm in decl.split(",")]
        assert names == [f[0] for f in binding._fields_], (struct, names)
    n = len(_lib.AbsorbJob._fields_)
    assert _lib.GrowJob._fields_[:n] == _lib.AbsorbJob._fields_ and [f[0] for f in _lib.GrowJob._fields_[n:]] == ["map_t", "at"]
    for f in _lib.AbsorbJob._fields_:
        assert getattr(_lib.GrowJob, f[0]).offset == getattr(_lib.AbsorbJob, f[0]).offset, f[0]
    src = open(os.path.join(ROOT, "fuxi-planner_amd", "csrc", "fxjps_maps.hip.inc")).read()
    assert re.search(r"__global__[^\n]*\bvoid k_prior_grow\(", src)
    # a NULL handle is refused before anything else
    L.fxjps_absorb_prior_grow.restype = C.c_int
    L.fxjps_absorb_prior_grow.argtypes = [C.c_void_p, C.POINTER(_lib.GrowJob), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(_lib.PriorGrown)]
    assert L.fxjps_absorb_prior_grow(None, None, 0, 0, None, None) == _lib.E_ARG


def make_job(buf, **kw):
    """A 6 x 8 matrix on prior 2 (10 x 12 at (0, 0), reso 0.5), at world (1, -1): prior cell (2, -2)."""
    from fuxi_planner_amd import _lib
    j = _lib.GrowJob()
    j.raw, j.layout, j.W0, j.H0 = buf.ctypes.data, 0, 6, 8
    j.lo[0], j.lo[1], j.win[0], j.win[1] = 0, 0, 6, 8
    j.prior, j.map_reso = 2, 0.5
    j.map_o[0], j.map_o[1], j.ori_pre[0], j.ori_pre[1] = 1.0, -1.0, 0.0, 0.0
    j.map_t[0], j.map_t[1] = 4.0, 3.0
    for k, v in kw.items():
        if isinstance(v, tuple):
            for i, x in enumerate(v):
                getattr(j, k)[i] = x
        else:
            setattr(j, k, v)
    return j


def outputs(arr, out):
    return ([(a.inside, a.outside, a.at[0], a.at[1]) for a in arr],
            [(g.named, g.W, g.H, g.shift[0], g.shift[1], g.origin[0], g.origin[1], g.changed) for g in out])


def checker():
    import __graft_entry__
    from fuxi_planner_amd import _lib
    __graft_entry__.build()
    L = _lib.load()
    msg = C.create_string_buffer(400)

    def check(jobs, wh, n=None, mode=0, limit=None, no_extents=False, no_out=False):
        arr = (_lib.GrowJob * max(len(jobs), 1))(*jobs)
        out = (_lib.PriorGrown * _lib.MAX_PRIOR_MAPS)()
        for g in out:
            g.changed = -7  # (the check leaves it alone)
        before = outputs(arr, out)
        lim = None if limit is None else _lib.ptr(np.array(limit, dtype=np.int32), C.c_int32)
        ext = np.ascontiguousarray(wh, dtype=np.int32)
        rc = L.fxjps_grow_check(arr, len(jobs) if n is None else n, mode, None if no_extents else _lib.ptr(ext, C.c_int32), lim,
                                None if no_out else out, msg, len(msg))
        return rc, msg.value.decode(), arr, out, before
    return check


def extents(**set_priors):
    from fuxi_planner_amd import _lib
    wh = np.zeros(2 * _lib.MAX_PRIOR_MAPS, dtype=np.int32)
    for k, s in set_priors.items():
        wh[2 * int(k[1:]):2 * int(k[1:]) + 2] = s
    return wh


def test_every_refusal_fires_in_the_check_and_writes_nothing():
    from fuxi_planner_amd import _lib
    check = checker()
    raw = np.zeros((6, 8), dtype=np.uint8)
    wh = extents(p2=(10, 12), p3=(8190, 8190))
    rc, text, arr, out, _ = check([make_job(raw), make_job(raw, map_o=(-2.0, 5.0), map_t=(1.0, 9.0))], wh)
    assert rc == 0 and text == ""
    # job 0: cell (2, -2) of the 10 x 12 prior -> grows to 10 x 14, shift (0, 2); job 1 at world (-2, 5): x -4 -> 14 x 20 in all
    assert (out[2].named, out[2].W, out[2].H, out[2].shift[0], out[2].shift[1], out[2].origin[0], out[2].origin[1]) == (1, 14, 20, 4, 2, -2.0, -1.0)
    assert [(a.inside, a.outside, a.at[0], a.at[1]) for a in arr] == [(48, 0, 6, 0), (48, 0, 0, 12)]
    assert all(g.changed == -7 for g in out) and [g.named for g in out] == [0, 0, 1] + [0] * 13
    assert (out[3].W, out[3].H) == (8190, 8190) and (out[0].W, out[0].H) == (0, 0)
    rc, text, _, out, _ = check([], wh, 0)
    assert rc == 0 and not any(g.named for g in out)
    nan, inf = float("nan"), float("inf")
    bad = [("n", dict(n=-1)), ("n", dict(n=257)), ("mode", dict(mode=3)), ("mode", dict(mode=-1)), ("extents", dict(no_extents=True)),
           ("NULL out", dict(no_out=True)), ("limit", dict(limit=(0, 100))), ("limit", dict(limit=(100, 8191))), ("limit", dict(limit=(-5, 8190))),
           ("raw", dict(raw=None)), ("layout", dict(layout=2)), ("layout", dict(layout=-1)), ("extents", dict(W0=0)), ("extents", dict(H0=8191)),
           ("rectangle", dict(win=(0, 8))), ("rectangle", dict(win=(6, -1))), ("rectangle", dict(lo=(-1, 0))), ("rectangle", dict(lo=(1, 0))),
           ("rectangle", dict(lo=(0, 3), win=(2, 6))), ("rectangle", dict(lo=(2147483647, 0), win=(2147483647, 1))),
           ("prior", dict(prior=-1)), ("prior", dict(prior=16)), ("not set", dict(prior=5)),
           ("non-finite", dict(map_o=(nan, 0.0))), ("non-finite", dict(map_o=(0.0, inf))), ("non-finite", dict(ori_pre=(-inf, 0.0))),
           ("non-finite map_t", dict(map_t=(nan, 0.0))), ("non-finite map_t", dict(map_t=(0.0, -inf))),
           ("map_reso", dict(map_reso=0.0)), ("map_reso", dict(map_reso=-0.5)), ("map_reso", dict(map_reso=nan)), ("map_reso", dict(map_reso=inf)),
           ("int32", dict(map_o=(2e9, 0.0))), ("int32", dict(map_o=(0.0, -1.5e9))), ("int32", dict(map_t=(2e9, 0.0))),
           ("bit-equal", dict(ori_pre=(0.0, 1e-300))), ("bit-equal", dict(ori_pre=(-0.0, 0.0))), ("bit-equal", dict(map_reso=0.5000000000000001)),
           ("above the limit", dict(map_o=(4200.0, 0.0))), ("above the limit", dict(map_t=(0.0, 4100.0)))]
    for word, kw in bad:
        call = {k: kw.pop(k) for k in ("n", "mode", "limit", "no_extents", "no_out") if k in kw}
        good = make_job(raw)
        jobs = [good, make_job(raw, **kw)] if kw else [good, good]
        rc, text, arr, out, before = check(jobs, wh, **call)
        assert rc == _lib.E_ARG and word in text, (word, kw, call, rc, text)
        assert text.startswith("job 1:" if kw else "job 0:"), text
        assert outputs(arr, out) == before, word  # a refused call writes nothing
    # the same ori_pre and resolution on ANOTHER prior are not compared
    assert check([make_job(raw), make_job(raw, prior=3, ori_pre=(5.0, 5.0), map_reso=0.25, map_o=(6.0, 6.0), map_t=(7.0, 7.0))], wh)[0] == 0
    # more than 2^30 staged bytes: 17 rectangles of 8190 x 8190 (the raw is never read by the check)
    big = np.zeros(1, dtype=np.uint8)
    jobs = [make_job(big, W0=8190, H0=8190, win=(8190, 8190), prior=3, map_o=(0.0, 0.0), map_t=(4095.0, 4095.0)) for _ in range(17)]
    rc, text, arr, out, before = check(jobs, wh)
    assert rc == _lib.E_ARG and "2^30" in text and text.startswith("job 16:") and outputs(arr, out) == before, text
    assert check(jobs[:16], wh)[0] == 0


def test_argument_faults_are_refused_alike_by_the_absorb_check_and_the_grow_check():
    """One per-job argument check serves both calls: what both refuse, both refuse with the same words, writing nothing.
    (Left out: an int32 overflow on axis 0 with a non-finite value on axis 1, where either fault may be the one named.)"""
    from fuxi_planner_amd import _lib
    check = checker()
    L = _lib.load()
    msg = C.create_string_buffer(400)
    raw = np.zeros((6, 8), dtype=np.uint8)
    wh = extents(p2=(10, 12))
    nan, inf = float("nan"), float("inf")
    n_prefix = C.sizeof(_lib.AbsorbJob)
    bad = [("n", dict(n=257)), ("mode", dict(mode=3)), ("extents", dict(no_extents=True)), ("raw", dict(raw=None)), ("layout", dict(layout=2)),
           ("extents", dict(W0=0)), ("extents", dict(W0=8191)), ("rectangle", dict(win=(0, 8))), ("rectangle", dict(lo=(1, 0))),
           ("rectangle", dict(lo=(0, 3), win=(2, 6))), ("prior", dict(prior=16)), ("not set", dict(prior=5)), ("map_reso", dict(map_reso=0.0)),
           ("map_reso", dict(map_reso=nan)), ("non-finite", dict(map_o=(nan, 0.0))), ("non-finite", dict(map_o=(0.0, inf))),
           ("non-finite", dict(ori_pre=(-inf, 0.0))), ("non-finite", dict(ori_pre=(0.0, nan)))]
    for word, kw in bad:
        call = {k: kw.pop(k) for k in ("n", "mode", "no_extents") if k in kw}
        jobs = [make_job(raw), make_job(raw, **kw)]
        rc, text, arr, out, before = check(jobs, wh, **call)
        assert rc == _lib.E_ARG and word in text and text.startswith("job 1:" if kw else "job 0:"), (word, kw, call, rc, text)
        assert outputs(arr, out) == before, word
        absorb = (_lib.AbsorbJob * 2)()    # the same two jobs: the absorb job is the grow job's prefix
        for a, g in zip(absorb, jobs):
            C.memmove(C.addressof(a), C.addressof(g), n_prefix)
            a.inside, a.outside = -3, -5
        rc = L.fxjps_absorb_check(absorb, call.get("n", 2), call.get("mode", 0), None if call.get("no_extents") else _lib.ptr(wh, C.c_int32), msg, len(msg))
        assert rc == _lib.E_ARG and msg.value.decode() == text, (word, rc, msg.value.decode(), text)
        assert [(a.inside, a.outside) for a in absorb] == [(-3, -5)] * 2, word


def test_the_limit_holds_exactly_at_the_edge():
    from fuxi_planner_amd import _lib
    check = checker()
    raw = np.zeros((6, 8), dtype=np.uint8)
    wh = extents(p2=(10, 12))
    # the 6 x 8 rectangle at prior cell (7, 9) of the 10 x 12 prior: grows to exactly 13 x 17
    job = make_job(raw, map_o=(3.5, 4.5), map_t=(6.5, 8.5))
    rc, _, _, out, _ = check([job], wh)
    assert rc == 0 and (out[2].W, out[2].H) == (13, 17)
    assert check([job], wh, limit=(13, 17))[0] == 0
    for limit, axis in (((12, 17), 0), ((13, 16), 1), ((12, 16), 0)):
        rc, text, arr, out, before = check([job], wh, limit=limit)
        assert rc == _lib.E_ARG and "axis %d" % axis in text and "above the limit" in text and outputs(arr, out) == before, (limit, text)
    # ... and on the low side, where the prior moves instead: cell (-3, -5) -> 13 x 17 as well
    low = make_job(raw, map_o=(-1.5, -2.5), map_t=(1.5, 1.5))
    rc, _, _, out, _ = check([low], wh, limit=(13, 17))
    assert rc == 0 and (out[2].W, out[2].H, out[2].shift[0], out[2].shift[1]) == (13, 17, 3, 5)
    assert check([low], wh, limit=(13, 16))[0] == _lib.E_ARG and check([low], wh, limit=(12, 17))[0] == _lib.E_ARG
    # the default is 8190: a side of 8190 passes, 8191 is refused; so does a fold whose SECOND job crosses it
    edge = make_job(raw, map_o=(4092.0, 0.0), map_t=(4095.0, 4.0))      # x cell 8184 + 6 = 8190
    over = make_job(raw, map_o=(4092.5, 0.0), map_t=(4095.5, 4.0))      # 8185 + 6 = 8191
    rc, _, _, out, _ = check([edge], wh)
    assert rc == 0 and out[2].W == 8190
    rc, text, _, _, _ = check([edge, over], wh)
    assert rc == _lib.E_ARG and text.startswith("job 1:") and "8191" in text, text
    # map_t alone can carry a side over the limit, as it sizes the reference's canvas
    assert check([make_job(raw, map_t=(4.0, 20.0))], wh, limit=(100, 41))[0] == _lib.E_ARG
    assert check([make_job(raw, map_t=(4.0, 20.0))], wh, limit=(100, 42))[0] == 0


def test_the_check_is_the_grow_host_fold_on_random_job_lists():
    check = checker()
    rng = np.random.default_rng(860)
    lists = jobs_seen = folded = moved = 0
    for trial in range(300):
        reso = float(rng.choice([0.05, 0.1, 0.17, 0.25]))
        priors = sorted(int(p) for p in rng.choice(16, size=int(rng.integers(1, 4)), replace=False))
        shapes = {p: (int(rng.integers(1, 60)), int(rng.integers(1, 60))) for p in priors}
        ori = {p: (float(rng.uniform(-5, 5)), float(rng.uniform(-5, 5))) for p in priors}     # off the cell lattice
        before = {p: np.zeros(shapes[p], dtype=np.uint8) for p in priors}
        world, cjobs, keep = [], [], []
        for _ in range(int(rng.integers(1, 7))):
            p = int(rng.choice(priors))
            w, h = int(rng.integers(1, 40)), int(rng.integers(1, 40))
            raw = np.zeros((w, h), dtype=np.uint8)
            keep.append(raw)
            map_o = (ori[p][0] + float(rng.uniform(-8, 8)), ori[p][1] + float(rng.uniform(-8, 8)))
            sub = rng.random() < 0.3 and w > 2 and h > 2
            lo, win = ((1, 1), (w - 2, h - 2)) if sub else ((0, 0), (w, h))
            map_t = (map_o[0] + win[0] * reso, map_o[1] + win[1] * reso) if rng.random() < 0.7 else (map_o[0] + float(rng.uniform(0, 6)),
                                                                                                       map_o[1] + float(rng.uniform(0, 6)))
            world.append(((0, raw, map_o, reso, (0.0, 0.0), (0.0, 0.0), 0, 1, p, ori[p], map_t), {"lo": list(lo), "win": list(win), "map_o": list(map_o),
                                                                                                 "map_t": list(map_t)}))
            cjobs.append(make_job(raw, W0=w, H0=h, lo=lo, win=win, prior=p, map_reso=reso, map_o=map_o, ori_pre=ori[p], map_t=map_t))
        wh = extents(**{"p%d" % p: shapes[p] for p in priors})
        rc, text, arr, out, _ = check(cjobs, wh, mode=int(rng.integers(0, 3)))
        assert rc == 0, (trial, text)
        after, origin, shift, at, _ = host_fold(before, [w[0] for w in world], "overwrite", crops=[w[1] for w in world])
        for p in range(16):
            g = out[p]
            if p in origin:
                assert (g.named, g.W, g.H) == (1,) + after[p].shape and (g.shift[0], g.shift[1]) == shift[p], (trial, p)
                assert [g.origin[0], g.origin[1]] == origin[p], (trial, p)
                moved += shift[p] != (0, 0)
            else:
                assert (g.named, g.W, g.H) == ((0,) + shapes[p] if p in shapes else (0, 0, 0)), (trial, p)
        assert [(a.at[0], a.at[1]) for a in arr] == at, (trial, at)
        assert all(a.inside == a.win[0] * a.win[1] and a.outside == 0 for a in arr)
        lists += 1
        jobs_seen += len(cjobs)
        folded += any(sum(1 for w in world if w[0][8] == p) > 1 for p in priors)
    assert lists == 300 and jobs_seen > 900 and folded > 150 and moved > 150, (lists, jobs_seen, folded, moved)
