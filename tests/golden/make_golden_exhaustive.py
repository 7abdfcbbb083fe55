#!/usr/bin/env python3
"""Generate tests/golden/exhaustive.npz by IMPORTING the real reference (as make_golden.py does: build container only).

Every grid of every small shape -- all (W, H) with W * H <= 12, and 4 x 4 -- with every cell as start and every cell as
goal (for W * H <= 12 also the ring of cells one step outside the grid), under both heuristics, through
make_golden.run_ref: jps1.method behind its counting grid and heap proxy.  Some 60 million records do not fit a data
file, so the file holds DIGESTS of them: per block of 16 consecutive grid codes and per heuristic one uint64 over the
paths and costs and one over the (cells, pushes, pops) counts.  Enumeration and digests are those of
tests/exhaustive_cases.py, which the host and GPU suites import as well.  No test runs this script.

    python tests/golden/make_golden_exhaustive.py [--procs N] [--out F]  writes exhaustive.npz (six minutes on 8 cores)
    python tests/golden/make_golden_exhaustive.py --explain WxH BLOCK H  prints the reference's records of one block

Arrays: r_<W>x<H>_h<h> and w_<W>x<H>_h<h>, uint64[blocks of the shape]; `meta`, a JSON string: shapes, queries per grid and
per shape, no-path records per shape and heuristic, the digest recipe.  The archive is written with fixed member order and
timestamps: the same reference gives the same bytes.
"""
import argparse
import io
import json
import multiprocessing as mp
import os
import sys
import zipfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

from make_golden import run_ref  # noqa: E402  (puts the reference and the repository root on sys.path)
import exhaustive_cases as ex  # noqa: E402

OUT = os.path.join(HERE, "exhaustive.npz")


def grid_records(W, H, code, h):
    """run_ref of every query of one grid -> (length, cells, cost, (cells read, pushes, pops), the records)."""
    m = ex.grid(W, H, code).astype(np.float64)
    s, g = ex.queries(W, H)
    recs = [run_ref(m, (int(a[0]), int(a[1])), (int(b[0]), int(b[1])), h) for a, b in zip(s, g)]
    length = np.array([0 if r["path"] is None else len(r["path"]) // 2 for r in recs], dtype=np.int32)
    flat = [v for r in recs if r["path"] is not None for v in r["path"]]
    cells = np.array(flat, dtype=np.int32).reshape(-1, 2)
    cost = np.array([0.0 if r["path"] is None else float(r["printed"]) for r in recs], dtype=np.float64)
    work = tuple(np.array([r[k] for r in recs], dtype=np.int64) for k in ("cells", "pushes", "pops"))
    return length, cells, cost, work, recs


def block_job(job):
    """-> (W, H, block, {h: (result digest, work digest, no-path records)})."""
    W, H, block = job
    out = {}
    for h in ex.HCHOICES:
        res, work, nopath = [], [], 0
        for code in ex.block_codes(W, H, block):
            length, cells, cost, counts, _ = grid_records(W, H, code, h)
            res.append((length, cells, cost))
            work.append(counts)
            nopath += int((length == 0).sum())
        out[h] = (ex.result_digest(res), ex.work_digest(work), nopath)
    return W, H, block, out


def write_npz(path, arrays):
    """np.savez with the members in the given order and a fixed timestamp (np.savez stamps each member with the clock)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, a in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main(procs, out=OUT):
    jobs = [(W, H, b) for W, H in ex.SHAPES for b in range(ex.n_blocks(W, H))]
    jobs.sort(key=lambda j: -ex.n_queries(j[0], j[1]))  # (the long blocks first; results are placed by index)
    dig = {(k, W, H, h): np.zeros(ex.n_blocks(W, H), dtype="<u8") for W, H in ex.SHAPES for h in ex.HCHOICES for k in "rw"}
    nopath = {(W, H, h): 0 for W, H in ex.SHAPES for h in ex.HCHOICES}
    with mp.Pool(procs) as pool:
        for n, (W, H, b, res) in enumerate(pool.imap_unordered(block_job, jobs, chunksize=4)):
            for h, (r, w, nop) in res.items():
                dig[("r", W, H, h)][b] = r
                dig[("w", W, H, h)][b] = w
                nopath[(W, H, h)] += nop
            if n % 500 == 0:
                print("%d of %d blocks" % (n, len(jobs)), flush=True)
    meta = {"shapes": [list(s) for s in ex.SHAPES], "block": ex.BLOCK, "hchoices": list(ex.HCHOICES),
            "blocks": {ex.shape_name(W, H): ex.n_blocks(W, H) for W, H in ex.SHAPES},
            "queries_per_grid": {ex.shape_name(W, H): ex.n_queries(W, H) for W, H in ex.SHAPES},
            "queries": {ex.shape_name(W, H): ex.shape_queries(W, H) for W, H in ex.SHAPES},
            "no_path": {"%s_h%d" % (ex.shape_name(W, H), h): nopath[(W, H, h)] for W, H in ex.SHAPES for h in ex.HCHOICES},
            "recipe": ex.RECIPE}
    arrays = [("meta", np.array(json.dumps(meta, sort_keys=True)))]
    arrays += [(ex.array_name(k, W, H, h), dig[(k, W, H, h)]) for W, H in ex.SHAPES for h in ex.HCHOICES for k in "rw"]
    write_npz(out, arrays)
    total = sum(ex.shape_queries(W, H) for W, H in ex.SHAPES) * len(ex.HCHOICES)
    print("wrote %s, %d bytes: %d shapes, %d blocks, %d records, %d without a path"
          % (out, os.path.getsize(out), len(ex.SHAPES), len(jobs), total, sum(nopath.values())))


def explain(shape, block, h):
    W, H = (int(v) for v in shape.lower().split("x"))
    assert (W, H) in ex.SHAPES and 0 <= block < ex.n_blocks(W, H) and h in ex.HCHOICES
    res, work = [], []
    for code in ex.block_codes(W, H, block):
        length, cells, cost, counts, recs = grid_records(W, H, code, h)
        res.append((length, cells, cost))
        work.append(counts)
        print("grid %d of %dx%d:" % (code, W, H))
        for row in ex.grid(W, H, code):
            print("    " + " ".join(str(int(v)) for v in row))
        for q, r in enumerate(recs):
            print("  q %d start %s goal %s h %d len %d cost %s cells %d pushes %d pops %d path %s"
                  % (q, tuple(r["start"]), tuple(r["goal"]), h, length[q], float(cost[q]).hex(), r["cells"], r["pushes"], r["pops"], r["path"]))
    print("result digest %d, work digest %d" % (ex.result_digest(res), ex.work_digest(work)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--procs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--out", default=OUT, help="where to write (to compare a second run with the committed file)")
    ap.add_argument("--explain", nargs=3, metavar=("WxH", "BLOCK", "H"))
    a = ap.parse_args()
    if a.explain:
        explain(a.explain[0], int(a.explain[1]), int(a.explain[2]))
    else:
        main(max(1, min(16, a.procs)), a.out)
