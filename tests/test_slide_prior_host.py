"""CPU suite of fxjps_absorb_prior_slide: fxjps_slide_check, the call's geometry and refusals
without a handle, against worldprep.slide_host on random job lists; slide_host itself against the grow fold of
tests/test_grow_prior_host.py sliced with numpy; no window, and a window that contains the grown frame, against
fxjps_grow_check field by field (the 88 reference-made cases of tests/golden/worldprep.json among them); every refusal,
each writing nothing; the over-limit rule exactly at the edge; infinite bounds, a window of one cell, one that holds no
cell of the old prior and one that excludes a whole rectangle; the header, the binding and the library agree; and the
census of what a moved origin costs in placement, which is printed and not gated.  No GPU needed."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from test_grow_prior_host import extents, host_fold, make_job
from worldprep_cases import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
USES = ("none", "always", "over_limit")


def grown_fields(g):
    return (g.named, g.W, g.H, g.shift[0], g.shift[1], g.origin[0], g.origin[1], g.changed)


def slid_fields(g):
    return grown_fields(g) + (g.trimmed, g.grown_wh[0], g.grown_wh[1], g.cut_lo[0], g.cut_lo[1], g.cut_hi[0], g.cut_hi[1])


def outputs(arr, out):
    return [(a.inside, a.outside, a.at[0], a.at[1]) for a in arr], [slid_fields(g) for g in out]


def keeps(windows):
    """{prior: (use, lo_xy, hi_xy)} -> fxjps_prior_keep_t[16]."""
    from fuxi_planner_amd import _lib
    arr = (_lib.PriorKeep * _lib.MAX_PRIOR_MAPS)()
    for p, (use, lo, hi) in windows.items():
        arr[p].use = _lib.KEEP_USES[use] if isinstance(use, str) else use
        for k in range(2):
            arr[p].lo[k], arr[p].hi[k] = lo[k], hi[k]
    return arr


def checker():
    import __graft_entry__
    from fuxi_planner_amd import _lib
    __graft_entry__.build()
    L = _lib.load()
    msg = C.create_string_buffer(400)

    def check(jobs, wh, windows=None, n=None, mode=0, limit=None, no_extents=False, no_out=False):
        arr = (_lib.GrowJob * max(len(jobs), 1))(*jobs)
        out = (_lib.PriorSlid * _lib.MAX_PRIOR_MAPS)()
        for g in out:
            g.changed = -7  # (the check leaves it alone)
        before = outputs(arr, out)
        lim = None if limit is None else _lib.ptr(np.array(limit, dtype=np.int32), C.c_int32)
        ext = np.ascontiguousarray(wh, dtype=np.int32)
        rc = L.fxjps_slide_check(arr, len(jobs) if n is None else n, mode, None if no_extents else _lib.ptr(ext, C.c_int32), lim,
                                 None if windows is None else keeps(windows), None if no_out else out, msg, len(msg))
        return rc, msg.value.decode(), arr, out, before
    return check


def grow_checker():
    from fuxi_planner_amd import _lib
    L = _lib.load()
    msg = C.create_string_buffer(400)

    def check(jobs, wh, mode=0, limit=None):
        arr = (_lib.GrowJob * max(len(jobs), 1))(*jobs)
        out = (_lib.PriorGrown * _lib.MAX_PRIOR_MAPS)()
        for g in out:
            g.changed = -7
        lim = None if limit is None else _lib.ptr(np.array(limit, dtype=np.int32), C.c_int32)
        rc = L.fxjps_grow_check(arr, len(jobs), mode, _lib.ptr(np.ascontiguousarray(wh, dtype=np.int32), C.c_int32), lim, out, msg, len(msg))
        return rc, msg.value.decode(), arr, out
    return check


def test_header_binding_and_library_agree():
    import __graft_entry__
    from fuxi_planner_amd import _lib
    __graft_entry__.build()
    hdr = open(os.path.join(ROOT, "include", "fxjps.h")).read()
    version = int(re.search(r"#define FXJPS_VERSION (\d+)", hdr).group(1))
    assert version >= 870 and _lib.VERSION == version
    assert re.search(r"^ \*\s+870\s+fxjps_absorb_prior_slide", hdr, re.M), "no changelog line for version 870"
    L = C.CDLL(_lib.LIB_PATH)
    assert L.fxjps_version() == version
    assert L.fxjps_prior_keep_size() == C.sizeof(_lib.PriorKeep) == 40
    assert L.fxjps_prior_slid_size() == C.sizeof(_lib.PriorSlid) == 72
    assert L.fxjps_grow_job_size() == C.sizeof(_lib.GrowJob) == 128 and L.fxjps_prior_grown_size() == C.sizeof(_lib.PriorGrown) == 48
    for name in ("fxjps_absorb_prior_slide", "fxjps_slide_check", "fxjps_prior_keep_size", "fxjps_prior_slid_size"):
        assert re.search(r"\bint %s\s*\(" % name, hdr) and hasattr(L, name) and name in _lib.SYMBOLS, name
    for word, value in (("NONE", 0), ("ALWAYS", 1), ("OVER_LIMIT", 2)):
        assert int(re.search(r"#define FXJPS_KEEP_%s\s+(\d+)" % word, hdr).group(1)) == value == _lib.KEEP_USES[word.lower()]
    for struct, binding in (("prior_keep", _lib.PriorKeep), ("prior_slid", _lib.PriorSlid)):
        body = re.search(r"typedef struct fxjps_%s \{(.*?)\} fxjps_%s_t;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [re.match(r"\s*(\w+)", nm).group(1) for _, decl in re.findall(r"(int32_t|int64_t|double)\s+([^;]+);", body) for nm in decl.split(",")]
        assert names == [f[0] for f in binding._fields_], (struct, names)
    # the slid record begins as the grown record does, `trimmed` where that one has its reserved word
    for f in ("named", "W", "H", "shift", "origin", "changed"):
        assert getattr(_lib.PriorSlid, f).offset == getattr(_lib.PriorGrown, f).offset, f
    assert _lib.PriorSlid.trimmed.offset == _lib.PriorGrown.reserved_.offset
    src = open(os.path.join(ROOT, "fuxi-planner_amd", "csrc", "fxjps_maps.hip.inc")).read()
    assert re.search(r"template <bool WINDOW> __global__[^\n]*\bvoid k_prior_grow\(", src)   # one template, the window a compile-time flag
    L.fxjps_absorb_prior_slide.restype = C.c_int
    L.fxjps_absorb_prior_slide.argtypes = [C.c_void_p, C.POINTER(_lib.GrowJob), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(_lib.PriorKeep),
                                           C.POINTER(_lib.PriorSlid)]
    assert L.fxjps_absorb_prior_slide(None, None, 0, 0, None, None, None) == _lib.E_ARG


def test_window_host_and_slide_host_are_a_slice_of_the_grow_fold():
    from fuxi_planner_amd.worldprep import slide_host, window_host
    rng = np.random.default_rng(870)
    prior = rng.integers(0, 2, size=(10, 8)).astype(np.uint8)
    prior[3, 2] = 255
    # ---- window_host: reso 0.5 at (-1, 2): world x 0.6 is cell 3 (1.6 / 0.5 = 3.2), x 3.2 is cell 8 (4.2 / 0.5 = 8.4)
    cut, origin, cut_lo, cut_hi = window_host(prior, (-1.0, 2.0), 0.5, (0.6, -INF), (3.2, 4.99))
    assert np.array_equal(cut, prior[3:8, 0:5]) and origin == [-1.0 + 0.5 * 3.0, 2.0] and (cut_lo, cut_hi) == ([3, 0], [2, 3])
    cut, origin, cut_lo, cut_hi = window_host(prior, (-1.0, 2.0), 0.5, (-INF, -INF), (INF, INF))
    assert np.array_equal(cut, prior) and origin == [-1.0, 2.0] and (cut_lo, cut_hi) == ([0, 0], [0, 0])
    for lo, hi in (((float("nan"), 0.0), (1.0, 3.0)), ((0.0, 0.0), (1.0, float("nan"))), ((2.0, 0.0), (1.0, 9.0)), ((0.0, 2.1), (3.0, 2.4)),
                   ((9.0, 0.0), (12.0, 9.0)), ((-9.0, 0.0), (-1.0, 9.0))):
        with pytest.raises(ValueError):
            window_host(prior, (-1.0, 2.0), 0.5, lo, hi)
    # ---- slide_host: the grow fold of the grow suite, sliced
    one = np.ones((4, 3), dtype=np.uint8)
    jobs = [(0, one, (-3.0, 3.0), 0.5, (0.0, 0.0), (0.0, 0.0), 0, 1, 4, (-1.0, 2.0)), (0, one, (3.0, 1.0), 0.5, (0.0, 0.0), (0.0, 0.0), 0, 1, 4, (-1.0, 2.0))]
    full, origin, shift, at, _ = host_fold({4: prior}, jobs, "overwrite")
    assert full[4].shape == (16, 10) and origin[4] == [-3.0, 1.0] and shift[4] == (4, 2) and at == [(0, 4), (12, 0)]
    old = np.zeros((16, 10), dtype=np.uint8)
    old[4:14, 2:10] = prior
    for use, limit, trimmed in (("always", None, True), ("over_limit", 13, True), ("over_limit", 16, False), ("none", None, False)):
        after, recs, per_job = slide_host({4: prior}, jobs, "overwrite", limit=limit, keep={4: ((-2.4, 1.6), (2.9, 5.0))}, use=use)
        r = recs[4]
        if trimmed:     # cells 1 .. 11 (0.6 / 0.5 = 1.2, 5.9 / 0.5 = 11.8) and 1 .. 8 (0.6 / 0.5, 4.0 / 0.5)
            want = full[4][1:11, 1:8]
            assert (r["W"], r["H"], r["shift"], r["cut_lo"], r["cut_hi"]) == (10, 7, (3, 1), (1, 1), (5, 2)) and r["origin"] == [-3.0 + 0.5 * 1.0, 1.0 + 0.5 * 1.0]
            assert per_job == [((-1, 3), 9, 3), ((11, -1), 0, 12)]
            assert r["changed"] == int(np.count_nonzero((want != 0) != (old[1:11, 1:8] != 0)))
        else:
            want = full[4]
            assert (r["W"], r["H"], r["shift"], r["cut_lo"], r["cut_hi"]) == (16, 10, (4, 2), (0, 0), (0, 0)) and r["origin"] == [-3.0, 1.0]
            assert per_job == [((0, 4), 12, 0), ((12, 0), 12, 0)]
        assert r["trimmed"] is trimmed and r["grown_wh"] == (16, 10)
        assert after[4].dtype == np.uint8 and np.array_equal(after[4], want) and (after[4] == 255).any()
    with pytest.raises(ValueError):
        slide_host({4: prior}, jobs, "overwrite", limit=13, keep={4: ((-2.4, 1.6), (2.9, 5.0))}, use="none")    # held to the limit job after job
    with pytest.raises(ValueError):
        slide_host({4: prior}, jobs, "overwrite", limit=9, keep={4: ((-2.4, 1.6), (2.9, 5.0))}, use="always")   # a window of 10 above 9
    with pytest.raises(ValueError):
        slide_host({4: prior, 5: prior}, jobs, "overwrite", keep={5: ((0.0, 0.0), (1.0, 1.0))}, use="always")   # no job names prior 5


def random_list(rng, keep_all=False):
    """-> (world jobs with their crop records, ctypes jobs, prior extents, {prior: bytes}, windows {prior: (use, lo, hi)},
    limit)."""
    reso = float(rng.choice([0.05, 0.1, 0.17, 0.25]))
    priors = sorted(int(p) for p in rng.choice(16, size=int(rng.integers(1, 4)), replace=False))
    shapes = {p: (int(rng.integers(1, 60)), int(rng.integers(1, 60))) for p in priors}
    ori = {p: (float(rng.uniform(-5, 5)), float(rng.uniform(-5, 5))) for p in priors}     # off the cell lattice
    before = {p: np.zeros(shapes[p], dtype=np.uint8) for p in priors}
    world, cjobs, named = [], [], set()
    for _ in range(int(rng.integers(1, 7))):
        p = int(rng.choice(priors))
        named.add(p)
        w, h = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        raw = np.zeros((w, h), dtype=np.uint8)
        map_o = (ori[p][0] + float(rng.uniform(-8, 8)), ori[p][1] + float(rng.uniform(-8, 8)))
        sub = rng.random() < 0.3 and w > 2 and h > 2
        lo, win = ((1, 1), (w - 2, h - 2)) if sub else ((0, 0), (w, h))
        map_t = (map_o[0] + win[0] * reso, map_o[1] + win[1] * reso) if rng.random() < 0.7 else (map_o[0] + float(rng.uniform(0, 6)),
                                                                                                   map_o[1] + float(rng.uniform(0, 6)))
        world.append(((0, raw, map_o, reso, (0.0, 0.0), (0.0, 0.0), 0, 1, p, ori[p], map_t), {"lo": list(lo), "win": list(win), "map_o": list(map_o),
                                                                                             "map_t": list(map_t)}))
        cjobs.append(make_job(raw, W0=w, H0=h, lo=lo, win=win, prior=p, map_reso=reso, map_o=map_o, ori_pre=ori[p], map_t=map_t))
    windows = {}
    for p in sorted(named):
        use = USES[int(rng.integers(1, 3))] if keep_all else USES[int(rng.integers(0, 3))]
        c = (ori[p][0] + float(rng.uniform(-6, 8)), ori[p][1] + float(rng.uniform(-6, 8)))
        half = (float(rng.uniform(0.3, 9)), float(rng.uniform(0.3, 9)))
        lo = [c[0] - half[0], c[1] - half[1]]
        hi = [c[0] + half[0], c[1] + half[1]]
        for side in (lo, hi):
            for k in range(2):
                if rng.random() < 0.1:
                    side[k] = -INF if side is lo else INF
        windows[p] = (use, tuple(lo), tuple(hi))
    limit = (int(rng.integers(30, 400)), int(rng.integers(30, 400)))
    return world, cjobs, extents(**{"p%d" % p: shapes[p] for p in priors}), before, shapes, windows, limit


def test_the_check_is_the_slide_host_fold_on_random_job_lists():
    from fuxi_planner_amd import _lib
    from fuxi_planner_amd.worldprep import slide_host
    check = checker()
    rng = np.random.default_rng(871)
    passed = refused = trimmed = spared = dropped = negative = 0
    seen = {u: 0 for u in USES}
    for trial in range(400):
        world, cjobs, wh, before, shapes, windows, limit = random_list(rng)
        mode = int(rng.integers(0, 3))
        rc, text, arr, out, was = check(cjobs, wh, windows, mode=mode, limit=limit)
        try:
            after, recs, per_job = slide_host(before, [w[0] for w in world], ("overwrite", "occupied", "known")[mode], crops=[w[1] for w in world], limit=limit,
                                              keep={p: (w[1], w[2]) for p, w in windows.items()}, use={p: w[0] for p, w in windows.items()})
        except ValueError:
            assert rc == _lib.E_ARG and text and outputs(arr, out) == was, (trial, rc, text)   # both refuse, and nothing is written
            refused += 1
            continue
        assert rc == 0, (trial, text)
        for p in range(16):
            g = out[p]
            if p in recs:
                r = recs[p]
                assert (g.named, g.W, g.H) == (1,) + after[p].shape == (1, r["W"], r["H"]) and (g.shift[0], g.shift[1]) == r["shift"], (trial, p)
                assert [g.origin[0], g.origin[1]] == r["origin"], (trial, p, g.origin[0], g.origin[1], r["origin"])
                assert ((g.grown_wh[0], g.grown_wh[1]), (g.cut_lo[0], g.cut_lo[1]), (g.cut_hi[0], g.cut_hi[1])) == (r["grown_wh"], r["cut_lo"], r["cut_hi"]), (trial, p)
                assert bool(g.trimmed) is r["trimmed"] and g.W <= limit[0] and g.H <= limit[1], (trial, p)
                trimmed += r["trimmed"]
                spared += windows[p][0] == "over_limit" and not r["trimmed"]
                negative += r["shift"][0] < 0 or r["shift"][1] < 0
                seen[windows[p][0]] += 1
            else:
                assert slid_fields(g) == ((0,) + shapes[p] if p in shapes else (0, 0, 0)) + (0, 0, 0.0, 0.0, -7, 0) + (shapes.get(p, (0, 0))) + (0, 0, 0, 0), (trial, p)
            assert g.changed == -7
        assert [((a.at[0], a.at[1]), a.inside, a.outside) for a in arr] == per_job, (trial, per_job)
        dropped += any(j[2] > 0 for j in per_job)
        passed += 1
    # the census of what the lists exercised: every use, cuts, windows spared by the limit rule, dropped cells, negative shifts
    assert passed > 200 and refused > 20 and trimmed > 100 and spared > 20 and dropped > 100 and negative > 20 and min(seen.values()) > 50, \
        (passed, refused, trimmed, spared, dropped, negative, seen)


def same_as_grow(trial, sl, gr, n):
    (rc, text, arr, out, _), (grc, gtext, garr, gout) = sl, gr
    assert (rc, text) == (grc, gtext), (trial, rc, text, grc, gtext)
    if rc:
        return False
    for p in range(16):
        assert slid_fields(out[p])[:8] == grown_fields(gout[p]), (trial, p)
        assert (out[p].grown_wh[0], out[p].grown_wh[1]) == (gout[p].W, gout[p].H), (trial, p)
        assert slid_fields(out[p])[11:] == (0, 0, 0, 0), (trial, p)
    assert [(a.inside, a.outside, a.at[0], a.at[1]) for a in arr[:n]] == [(a.inside, a.outside, a.at[0], a.at[1]) for a in garr[:n]], trial
    return True


def test_no_window_and_a_window_around_everything_are_the_grow_check():
    check, grow = checker(), grow_checker()
    rng = np.random.default_rng(872)
    ok = 0
    for trial in range(150):
        world, cjobs, wh, before, shapes, windows, limit = random_list(rng, keep_all=True)
        limit = limit if trial % 3 else None    # (a list the limit refuses is refused alike, word for word)
        gr = grow(cjobs, wh, limit=limit)
        ok += same_as_grow(trial, check(cjobs, wh, None, limit=limit), gr, len(cjobs))
        ok += same_as_grow(trial, check(cjobs, wh, {p: ("none", (5.0, 5.0), (-5.0, float("nan"))) for p in windows}, limit=limit), gr, len(cjobs))  # not read
        if gr[0] == 0:
            # ... a window that contains the grown frame: nothing is cut, whatever the use; the bounds finite, infinite and mixed
            for use in ("always", "over_limit"):
                for lo, hi in (((-1e6, -1e6), (1e6, 1e6)), ((-INF, -INF), (INF, INF)), ((-INF, -100.0), (100.0, INF))):
                    sl = check(cjobs, wh, {p: (use, lo, hi) for p in windows}, limit=limit)
                    assert same_as_grow((trial, use, lo), sl, gr, len(cjobs))
                    assert all(bool(sl[3][p].trimmed) == (use == "always") for p in windows)
    assert ok > 150, ok
    # the 88 cases whose canvases come from executing the reference's lines
    done = 0
    for i, c in enumerate(cases()):
        if c["raises"] or c["prior"] is None:
            continue
        raw = np.ascontiguousarray(c["raw"], dtype=np.uint8)
        w, h = raw.shape
        job = make_job(raw, W0=w, H0=h, win=(w, h), prior=7, map_reso=c["reso"], map_o=tuple(c["map_o"]), ori_pre=tuple(c["ori_pre"]), map_t=tuple(c["map_t"]))
        wh = extents(p7=c["prior"].shape)
        gr = grow([job], wh)
        assert gr[0] == 0 and (gr[3][7].W, gr[3][7].H) == tuple(c["canvas_shape"]) and [gr[3][7].origin[0], gr[3][7].origin[1]] == c["canvas_o"], i
        assert same_as_grow(i, check([job], wh, None), gr, 1)
        top = [c["canvas_o"][k] + c["reso"] * (c["canvas_shape"][k] + 2) for k in range(2)]
        assert same_as_grow(i, check([job], wh, {7: ("always", (c["canvas_o"][0] - 1.0, c["canvas_o"][1] - 1.0), tuple(top))}), gr, 1)
        done += 1
    assert done == 88


def test_every_refusal_fires_in_the_check_and_writes_nothing():
    from fuxi_planner_amd import _lib
    check = checker()
    raw = np.zeros((6, 8), dtype=np.uint8)
    wh = extents(p2=(10, 12), p3=(20, 20))
    nan = float("nan")
    # the 6 x 8 rectangle at cell (2, -2) of the 10 x 12 prior at (0, 0), reso 0.5: grown 10 x 14 at (0, -1), shift (0, 2)
    good = {2: ("always", (1.0, 0.0), (4.0, 5.0))}
    rc, text, arr, out, _ = check([make_job(raw)], wh, good)
    assert rc == 0 and text == "" and slid_fields(out[2]) == (1, 6, 10, -2, 0, 1.0, 0.0, -7, 1, 10, 14, 2, 2, 2, 2), slid_fields(out[2])
    assert [(a.inside, a.outside, a.at[0], a.at[1]) for a in arr] == [(6 * 6, 48 - 36, 0, -2)]
    assert (out[3].named, out[3].W, out[3].H, out[3].grown_wh[0], out[3].grown_wh[1], out[3].trimmed) == (0, 20, 20, 20, 20, 0)
    bad = [("keep.use", {2: (3, (1.0, 0.0), (4.0, 5.0))}), ("keep.use", {2: (-1, (1.0, 0.0), (4.0, 5.0))}), ("keep.use", {9: (7, (0.0, 0.0), (1.0, 1.0))}),
           ("NaN", {2: ("always", (nan, 0.0), (4.0, 5.0))}), ("NaN", {2: ("over_limit", (1.0, 0.0), (4.0, nan))}),
           ("above its hi", {2: ("always", (4.5, 0.0), (4.0, 5.0))}), ("above its hi", {2: ("over_limit", (1.0, INF), (4.0, 9.0))}), 
           ("holds no cell", {2: ("always", (1.0, INF), (4.0, INF))}),
           ("holds no cell", {2: ("always", (1.0, 0.1), (4.0, 0.4))}),        # lo and hi in one cell: k1 == k0
           ("holds no cell", {2: ("always", (5.0, 0.0), (9.0, 5.0))}),        # right of the grown frame: both clamp to 10
           ("holds no cell", {2: ("always", (-9.0, 0.0), (-0.5, 5.0))}),      # left of it: both clamp to 0
           ("holds no cell", {2: ("always", (1.0, -INF), (4.0, -INF))}),
           ("no job names", {2: good[2], 3: ("always", (0.0, 0.0), (1.0, 1.0))}), ("no job names", {2: good[2], 11: ("over_limit", (0.0, 0.0), (1.0, 1.0))})]
    for word, windows in bad:
        rc, text, arr, out, before = check([make_job(raw)], wh, windows)
        assert rc == _lib.E_ARG and word in text and text.startswith("prior %d:" % max(windows)), (word, rc, text)
        assert outputs(arr, out) == before, word
    # the window above the limit names the prior and the axis
    for limit, axis in (((5, 10), 0), ((6, 9), 1)):
        rc, text, arr, out, before = check([make_job(raw)], wh, good, limit=limit)
        assert rc == _lib.E_ARG and text.startswith("prior 2: axis %d:" % axis) and "above the limit" in text and outputs(arr, out) == before, text
    assert check([make_job(raw)], wh, good, limit=(6, 10))[0] == 0
    # what fxjps_grow_check refuses is refused here with its words, a window or none
    for windows in (None, good):
        for word, kw, call in (("n", {}, dict(n=257)), ("mode", {}, dict(mode=3)), ("extents", {}, dict(no_extents=True)), ("NULL out", {}, dict(no_out=True)),
                               ("limit", {}, dict(limit=(0, 100))), ("raw", dict(raw=None), {}), ("rectangle", dict(win=(0, 8)), {}),
                               ("prior", dict(prior=16), {}), ("not set", dict(prior=5), {}), ("non-finite map_t", dict(map_t=(nan, 0.0)), {}),
                               ("map_reso", dict(map_reso=0.0), {}), ("int32", dict(map_o=(2e9, 0.0)), {}), ("bit-equal", dict(ori_pre=(0.0, 1e-300)), {})):
            jobs = [make_job(raw), make_job(raw, **kw)]
            rc, text, arr, out, before = check(jobs, wh, windows, **call)
            assert rc == _lib.E_ARG and word in text and text.startswith("job 1:" if kw else "job 0:"), (word, rc, text)
            assert outputs(arr, out) == before, word
    # a prior WITHOUT a window is held to the limit job after job, as ever; one with a window is not
    far = make_job(raw, map_o=(60.0, 0.0), map_t=(63.0, 4.0))       # x cell 120: 126 cells
    rc, text, arr, out, before = check([far], wh, None, limit=(100, 100))
    assert rc == _lib.E_ARG and text.startswith("job 0:") and "above the limit" in text and outputs(arr, out) == before
    rc, text, arr, out, before = check([far], wh, {2: ("none", (0.0, 0.0), (1.0, 1.0))}, limit=(100, 100))
    assert rc == _lib.E_ARG and text.startswith("job 0:") and "above the limit" in text and outputs(arr, out) == before
    rc, text, arr, out, _ = check([far], wh, {2: ("over_limit", (55.0, -INF), (INF, INF))}, limit=(100, 100))
    assert rc == 0 and (out[2].W, out[2].H, out[2].grown_wh[0], out[2].cut_lo[0], out[2].shift[0], out[2].origin[0]) == (16, 12, 126, 110, -110, 0.0 + 0.5 * 110.0)
    # a grown side that does not fit int32 is refused even under a window
    rc, text, arr, out, before = check([make_job(raw), make_job(raw, map_o=(-1.0e9, 0.0), map_t=(1.0e9, 1.0))], wh, good)
    assert rc == _lib.E_ARG and "int32" in text and outputs(arr, out) == before, text


def test_over_limit_holds_exactly_at_the_edge():
    from fuxi_planner_amd import _lib
    check = checker()
    raw = np.zeros((6, 8), dtype=np.uint8)
    wh = extents(p2=(10, 12))
    job = make_job(raw, map_o=(3.5, 4.5), map_t=(6.5, 8.5))      # the 10 x 12 prior grows to exactly 13 x 17 (the grow suite's edge case)
    window = (1.0, 1.0), (6.0, 7.0)                               # cells 2 .. 12 and 2 .. 14: 10 x 12
    for limit, cut in (((13, 17), False), ((14, 18), False), ((12, 17), True), ((13, 16), True), ((12, 16), True)):
        rc, text, arr, out, _ = check([job], wh, {2: ("over_limit", window[0], window[1])}, limit=limit)
        assert rc == 0, (limit, text)
        g = out[2]
        if cut:     # limit + 1 on either axis: the WHOLE window applies, both axes
            assert slid_fields(g) == (1, 10, 12, -2, -2, 1.0, 1.0, -7, 1, 13, 17, 2, 2, 1, 3), (limit, slid_fields(g))
            assert (arr[0].at[0], arr[0].at[1], arr[0].inside, arr[0].outside) == (5, 7, 5 * 5, 48 - 25)
        else:       # an extent of `limit` is not cut
            assert slid_fields(g) == (1, 13, 17, 0, 0, 0.0, 0.0, -7, 0, 13, 17, 0, 0, 0, 0), (limit, slid_fields(g))
            assert (arr[0].at[0], arr[0].at[1], arr[0].inside, arr[0].outside) == (7, 9, 48, 0)
    # a window of limit + 1 cells is refused; of exactly limit it passes
    rc, text, arr, out, before = check([job], wh, {2: ("over_limit", (0.0, 1.0), (6.0, 7.0))}, limit=(11, 16))   # 12 x 12
    assert rc == _lib.E_ARG and text.startswith("prior 2: axis 0:") and "12 cells is above the limit of 11" in text and outputs(arr, out) == before, text
    rc, text, arr, out, before = check([job], wh, {2: ("over_limit", (0.0, 1.0), (6.0, 7.0))}, limit=(12, 11))
    assert rc == _lib.E_ARG and text.startswith("prior 2: axis 1:") and outputs(arr, out) == before, text
    rc, _, _, out, _ = check([job], wh, {2: ("over_limit", (0.0, 1.0), (6.0, 7.0))}, limit=(12, 12))
    assert rc == 0 and (out[2].W, out[2].H, out[2].trimmed) == (12, 12, 1)
    # "always" cuts below the limit as well
    rc, _, _, out, _ = check([job], wh, {2: ("always", window[0], window[1])}, limit=(13, 17))
    assert rc == 0 and (out[2].W, out[2].H, out[2].trimmed) == (10, 12, 1)


def test_infinite_bounds_one_cell_and_windows_that_miss():
    check = checker()
    raw = np.zeros((6, 8), dtype=np.uint8)
    wh = extents(p2=(10, 12))
    job = make_job(raw, map_o=(-4.0, -1.0), map_t=(-1.0, 3.0))    # cell (-8, -2): grown 18 x 14 at (-4, -1), shift (8, 2), the rectangle at (0, 0)
    rc, _, arr, out, _ = check([job], wh, None)
    assert rc == 0 and slid_fields(out[2])[:7] == (1, 18, 14, 8, 2, -4.0, -1.0) and (arr[0].at[0], arr[0].at[1]) == (0, 0)
    # ---- an infinite bound cuts nothing on its side
    rc, _, arr, out, _ = check([job], wh, {2: ("always", (-INF, 0.0), (2.0, INF))})
    assert rc == 0 and slid_fields(out[2]) == (1, 12, 12, 8, 0, -4.0, -1.0 + 0.5 * 2.0, -7, 1, 18, 14, 0, 2, 6, 0), slid_fields(out[2])
    assert (arr[0].at[0], arr[0].at[1], arr[0].inside, arr[0].outside) == (0, -2, 36, 12)
    # ---- a window of one cell: grown cell (9, 3), which is old cell (1, 1)
    rc, _, arr, out, _ = check([job], wh, {2: ("always", (0.5, 0.5), (1.0, 1.0))})
    assert rc == 0 and slid_fields(out[2]) == (1, 1, 1, -1, -1, -4.0 + 0.5 * 9.0, -1.0 + 0.5 * 3.0, -7, 1, 18, 14, 9, 3, 8, 10), slid_fields(out[2])
    assert (arr[0].at[0], arr[0].at[1], arr[0].inside, arr[0].outside) == (-9, -3, 0, 48)    # the whole rectangle is excluded
    # ---- a window that holds no cell of the old prior: x cells 0 .. 6, the old prior begins at 8
    rc, _, arr, out, _ = check([job], wh, {2: ("always", (-INF, -INF), (-1.0, INF))})
    assert rc == 0 and slid_fields(out[2]) == (1, 6, 14, 8, 2, -4.0, -1.0, -7, 1, 18, 14, 0, 0, 12, 0), slid_fields(out[2])
    assert (arr[0].inside, arr[0].outside) == (48, 0)
    # ---- two jobs, the window excludes one of them whole and cuts through the other
    other = make_job(raw, map_o=(3.0, 2.0), map_t=(6.0, 6.0))     # cell (6, 4) of the old prior: grown cell (14, 6)
    rc, _, arr, out, _ = check([job, other], wh, {2: ("always", (0.0, 0.0), (5.0, 4.0))})       # cells 8 .. 18, 2 .. 10
    assert rc == 0 and (out[2].W, out[2].H, out[2].grown_wh[0], out[2].grown_wh[1]) == (10, 8, 20, 14)
    assert [(a.at[0], a.at[1], a.inside, a.outside) for a in arr] == [(-8, -2, 0, 48), (6, 4, 4 * 4, 32)]


def test_the_jitter_a_moved_origin_costs_in_placement(capsys):
    """Not gated: after a slide the origin is og + reso * k0, and every later tick truncates (map_o - origin) / reso against
    it.  How often does a rectangle land off the cell where the unslid prior would have put it?  Origins and map origins of
    two decimals, the map within 60 m of the new origin on either side, k0 in 1 .. 600, the fixture's four resolutions; the
    figures are printed and recorded in DESIGN.md 3.22.  (Two cells happen where the map origin lies between the old and the
    new prior origin: the truncation toward zero changes side there, on top of the rounding of og + reso * k0.)"""
    rng = np.random.default_rng(873)
    figures = {}

    def placed(map_o, origin, reso):   # d of fxjps_absorb_prior: at_raw - at_pre (st:212-214)
        o1 = min(map_o, origin)
        return int((map_o - o1) / reso) - int((origin - o1) / reso)
    for reso in (0.05, 0.1, 0.2, 0.25):
        off = far = above = off_above = 0
        n = 20000
        for _ in range(n):
            og = round(float(rng.uniform(-50, 50)), 2)
            k0 = int(rng.integers(1, 601))
            moved = og + reso * float(k0)
            map_o = round(moved + float(rng.uniform(-60, 60)), 2)   # (a detected map on either side of the new origin)
            unslid = placed(map_o, og, reso) - k0
            slid = placed(map_o, moved, reso)
            off += unslid != slid
            far += abs(unslid - slid) > 1
            above += map_o >= moved
            off_above += map_o >= moved and unslid != slid
        figures[reso] = (100.0 * off / n, 100.0 * far / n, 100.0 * off_above / above)
    with capsys.disabled():
        print("\njitter census: after a slide a rectangle lands off the unslid placement in " +
              ", ".join("%.1f %% (two cells: %.2f %%; maps at or above the new origin alone: %.1f %%) at reso %g" % (figures[r] + (r,))
                        for r in sorted(figures)) + " of placements")
    assert all(math.isfinite(v) for pair in figures.values() for v in pair)
