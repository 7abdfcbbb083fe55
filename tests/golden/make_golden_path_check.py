#!/usr/bin/env python3
"""Golden vectors for the path check (fxjps_check_path / fxjps_check_paths_slots), produced with the
reference's own code at generation time: the paths come from scripts/jps1.py's method(), and the expected verdict of every
case from its blocked() (jps1.py:14-31), called on each unit step of the path in order.  Only inputs and outputs are stored.

A case: a random grid G of 3 to 40 cells a side (0 / 1 bytes, density 0.05 to 0.35), a path of method() on G (or no path:
the empty path), then the grid G' the path is checked on -- G with a few cells toggled: some on the path, some beside a
diagonal step (both orthogonal neighbours: the squeeze), some nowhere near -- and a small shift that sometimes pushes the
path over an edge.  Whether a cell lies outside the grid is judged here (a step whose target is outside: OUTSIDE, as is a
first cell outside); every step inside is blocked()'s to judge.

    python tests/golden/make_golden_path_check.py
"""
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/scripts"
sys.path.insert(0, REF)
import jps1  # noqa: E402  (the reference's module itself)

VALID, EMPTY, BLOCKED, OUTSIDE, MALFORMED = 1, 0, 2, 3, -1
N_CASES = 300


def sgn(v):
    return (v > 0) - (v < 0)


def steps_of(path):
    """The unit steps of a jump-point path: (segment, cell, direction)."""
    out = []
    for i in range(len(path) - 1):
        (ax, ay), (bx, by) = path[i], path[i + 1]
        dx, dy = bx - ax, by - ay
        assert (dx, dy) != (0, 0) and (dx == 0 or dy == 0 or abs(dx) == abs(dy)), "method() returned a malformed path"
        u = (sgn(dx), sgn(dy))
        for k in range(max(abs(dx), abs(dy))):
            out.append((i, (ax + u[0] * k, ay + u[1] * k), u))
    return out


def expected(path, grid, shift):
    """-> (verdict, seg, cell) with the reference's blocked() on every step."""
    W, H = grid.shape
    if not path:
        return EMPTY, -1, (-1, -1)
    x0, y0 = path[0][0] + shift[0], path[0][1] + shift[1]
    if not (0 <= x0 < W and 0 <= y0 < H):
        return OUTSIDE, 0, (x0, y0)
    for i, (cx, cy), (ux, uy) in steps_of(path):
        cx, cy = cx + shift[0], cy + shift[1]
        tx, ty = cx + ux, cy + uy
        if not (0 <= tx < W and 0 <= ty < H):
            return OUTSIDE, i, (tx, ty)
        if jps1.blocked(cx, cy, ux, uy, grid):
            return BLOCKED, i, (tx, ty)
    return VALID, -1, (-1, -1)


def main():
    rng = np.random.default_rng(840)
    recs = []
    count = {VALID: 0, EMPTY: 0, BLOCKED: 0, OUTSIDE: 0}
    kinds = ("same", "on_path", "squeeze", "elsewhere", "shift_small", "shift_edge")
    t = 0
    while len(recs) < N_CASES or min(count.values()) < 20:
        kind = kinds[t % len(kinds)]
        t += 1
        W, H = int(rng.integers(3, 41)), int(rng.integers(3, 41))
        G = (rng.random((W, H)) < rng.uniform(0.05, 0.35)).astype(np.int64)
        free = np.argwhere(G == 0)
        if len(free) < 2:
            continue
        s, g = (tuple(int(v) for v in free[k]) for k in rng.choice(len(free), 2, replace=False))
        if rng.random() < 0.1:  # (the reference searches from an occupied start)
            G[s] = 1
        with contextlib.redirect_stdout(io.StringIO()):
            found = jps1.method(G, s, g, 2)[0]
        path = [] if found == 0 else [tuple(int(v) for v in c) for c in found]
        if len(recs) >= N_CASES and path:  # (only the empty class can still be short: its cases come from unreachable goals)
            if count[EMPTY] < 20:
                continue
        G2 = G.copy()
        shift = (0, 0)
        st = steps_of(path)
        walked = {(c[0] + u[0], c[1] + u[1]) for _, c, u in st} | ({path[0]} if path else set())
        beside = {(c[0] + u[0], c[1]) for _, c, u in st if u[0] and u[1]} | {(c[0], c[1] + u[1]) for _, c, u in st if u[0] and u[1]}
        if kind == "on_path" and st:
            for k in rng.choice(len(st), min(len(st), int(rng.integers(1, 3))), replace=False):
                _, c, u = st[k]
                G2[c[0] + u[0], c[1] + u[1]] ^= 1
        elif kind == "squeeze":
            diag = [k for k, (_, c, u) in enumerate(st) if u[0] and u[1]]
            if diag:
                _, c, u = st[diag[int(rng.integers(len(diag)))]]
                G2[c[0] + u[0], c[1]] = 1
                G2[c[0], c[1] + u[1]] = 1
            elif st:
                _, c, u = st[int(rng.integers(len(st)))]
                G2[c[0] + u[0], c[1] + u[1]] = 1
        elif kind == "elsewhere":
            far = [tuple(c) for c in np.argwhere(np.ones_like(G)) if tuple(c) not in walked and tuple(c) not in beside]
            for k in rng.choice(len(far), min(len(far), 4), replace=False) if far else []:
                G2[far[k]] ^= 1
        elif kind == "shift_small":
            shift = (int(rng.integers(-2, 3)), int(rng.integers(-2, 3)))
        elif kind == "shift_edge" and path:
            xs, ys = [p[0] for p in path], [p[1] for p in path]
            axis = int(rng.integers(4))  # over the edge by one or two cells on one side
            over = int(rng.integers(1, 3))
            shift = [(-(min(xs) + over), 0), (W - 1 - max(xs) + over, 0), (0, -(min(ys) + over)), (0, H - 1 - max(ys) + over)][axis]
            if rng.random() < 0.5:
                shift = (shift[0] + (axis >= 2) * int(rng.integers(-1, 2)), shift[1] + (axis < 2) * int(rng.integers(-1, 2)))
        verdict, seg, cell = expected(path, G2, shift)
        if kind == "same":
            assert verdict in (VALID, EMPTY), "a path of method() does not pass blocked() on its own grid"
        count[verdict] += 1
        recs.append({"kind": kind, "shape": [W, H], "grid_bits": np.packbits(G2.astype(np.uint8).reshape(-1)).tobytes().hex(),
                     "path": [v for c in path for v in c], "shift": list(shift), "verdict": verdict, "seg": seg, "cell": list(cell)})
    assert min(count.values()) >= 20, count
    assert all(r["verdict"] == VALID for r in recs if r["kind"] == "same" and r["path"])
    out = os.path.join(HERE, "path_check.json")
    with open(out, "w") as f:
        json.dump(recs, f, separators=(",", ":"))
    print(len(recs), "cases", {k: v for k, v in count.items()}, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
