#!/usr/bin/env python3
"""Golden vectors for the world-frame front of a tick, produced by EXECUTING the reference's
own lines, read from /root/reference at generation time, dedented and exec'ed on prepared inputs:
    the prior's far corner   scripts/global_planner_st.py:185-187   / scripts/global_planner_ccst.py:377-379
    merge + world -> cell    scripts/global_planner_st.py:210-227   / scripts/global_planner_ccst.py:395-412
    the preparation          scripts/global_planner_st.py:228-275   / scripts/global_planner_ccst.py:413-464
The merge and the preparation run as two pieces in one namespace, so that the canvas can be captured between them.
Only inputs and outputs are stored (tests/golden/worldprep.json): grids bit-packed, every float as float.hex().

    python tests/golden/make_golden_worldprep.py
"""
import json
import os
import textwrap

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/scripts"
RANGES = {0: ("global_planner_st.py", (185, 187), (210, 227), (228, 275)), 1: ("global_planner_ccst.py", (377, 379), (395, 412), (413, 464))}
PER_NODE = 60
RESOS = (0.05, 0.1, 0.2, 0.25)
ARRANGE = ("inside", "left", "below", "right", "above", "disjoint", "none")


def ref_block(variant, which):
    name = RANGES[variant][0]
    lo, hi = RANGES[variant][which]
    with open(os.path.join(REF, name), encoding="utf-8", errors="replace") as f:
        return compile(textwrap.dedent("".join(f.readlines()[lo - 1:hi])), "%s:%d-%d" % (name, lo, hi), "exec")


class _O(object):
    pass


def hexes(v):
    return [float(x).hex() for x in v]


def bits(a):
    return np.packbits(np.ascontiguousarray(a, dtype=np.uint8)).tobytes().hex()


def run_ref(variant, c):
    """-> the record's outputs.  c: the case's inputs as Python values."""
    planner = _O()
    planner.map_reso = c["reso"]
    planner.map_t = list(c["map_t"])
    raw = c["raw"]
    ns = {"np": np, "planner": planner, "map_pre": c["prior"], "ori_pre": list(c["ori_pre"]), "map_o": list(c["map_o"]), "map_reso": c["reso"],
          "mapu": raw.copy(), "map_c": raw.shape[0], "map_r": raw.shape[1], "global_goal": np.array([c["goal"][0], c["goal"][1], 1.5]),
          "px": c["pos"][0], "py": c["pos"][1], "ifa": c["ifa"]}
    if c["prior"] is not None:
        exec(ref_block(variant, 1), ns)
    try:
        exec(ref_block(variant, 2), ns)
    except ValueError:
        return {"raises": True}
    cv = np.asarray(ns["mapu"])
    out = {"raises": False, "canvas_shape": [int(cv.shape[0]), int(cv.shape[1])], "canvas_bits": bits(cv > 0), "canvas_o": hexes(ns["map_o"]),
           "start": [int(v) for v in ns["map_start"]], "goal": [int(v) for v in ns["map_goal"]]}
    assert (ns["map_c"], ns["map_r"]) == cv.shape
    try:
        exec(ref_block(variant, 3), ns)
        g = ns["mapu"]
        assert set(np.unique(g)) <= {0.0, 1.0}
        out["prep"] = {"grid_shape": list(g.shape), "grid_bits": bits(g == 1), "start_out": [int(v) for v in ns["map_start"]],
                       "goal_out": [int(v) for v in ns["map_goal"]], "map_d": [int(v) for v in ns["map_d"]], "end_occu": int(ns["end_occu"]),
                       "origin": hexes(ns["map_o"])}
    except (IndexError, ValueError):
        out["prep"] = None  # the reference itself fails on this input (st with ifa = 0, a goal with no free cell, ...)
    return out


def dec(k, reso, off=0.0):
    """The double nearest to the decimal k * reso + off: what a launch file or a message holds for an origin on the grid."""
    return float(repr(round(k * reso + off, 6)))


def make_case(rng, variant, arrange, aligned):
    reso = float(rng.choice(RESOS))
    l1, l2 = int(rng.integers(1, 17)), int(rng.integers(1, 15))
    W0, H0 = int(rng.integers(1, 13)), int(rng.integers(1, 13))
    kp = [int(rng.integers(-160, 40)), int(rng.integers(-160, 40))]  # the prior's origin, in cells
    a, b = int(rng.integers(0, 5)), int(rng.integers(0, 5))
    if arrange == "inside":
        l1, l2 = max(l1, W0 + a + 1), max(l2, H0 + b + 1)
        ko = [kp[0] + a, kp[1] + b]
    elif arrange == "left":
        ko = [kp[0] - 1 - a, kp[1] + b]
    elif arrange == "below":
        ko = [kp[0] + a, kp[1] - 1 - b]
    elif arrange == "right":
        ko = [kp[0] + l1 - 1 - min(a, l1 - 1), kp[1] - b]
        W0 += 1
    elif arrange == "above":
        ko = [kp[0] - a, kp[1] + l2 - 1 - min(b, l2 - 1)]
        H0 += 1
    else:  # disjoint (zeros between), or no prior at all
        ko = [kp[0] + l1 + 1 + a, kp[1] + l2 + 1 + b] if rng.random() < 0.5 else [kp[0] - W0 - 1 - a, kp[1] + b]
    off = [0.0, 0.0] if aligned else [float(rng.choice([0.03, 0.07, 0.013])), float(rng.choice([0.02, 0.041, 0.009]))]
    off_p = [0.0, 0.0] if aligned else [float(rng.choice([0.0, 0.01, 0.06])), float(rng.choice([0.0, 0.033, 0.017]))]
    map_o = [dec(ko[0], reso, off[0]), dec(ko[1], reso, off[1])]
    ori_pre = [dec(kp[0], reso, off_p[0]), dec(kp[1], reso, off_p[1])]
    raw = rng.choice(np.array([0, 0, 0, 0, 1, 1, 50, 99, 3], dtype=np.int64), size=(W0, H0))
    prior = None if arrange == "none" else (rng.random((l1, l2)) < 0.45).astype(np.uint8)
    if prior is not None and arrange != "disjoint":
        prior[rng.integers(0, l1), :] = 1  # (so that a free detected cell over an occupied prior cell is the rule)
    map_t = [map_o[0] + W0 * reso, map_o[1] + H0 * reso]  # st:24, the same expression
    # positions and goals in world coordinates: around both maps, every third case left of / below both
    lo = [min(map_o[0], ori_pre[0]), min(map_o[1], ori_pre[1])] if prior is not None else list(map_o)
    hi = [max(map_t[0], ori_pre[0] + l1 * reso), max(map_t[1], ori_pre[1] + l2 * reso)] if prior is not None else list(map_t)
    far = rng.random() < 0.34

    def point():
        u = rng.random(2)
        p = [lo[k] + u[k] * (hi[k] - lo[k] + 2 * reso) for k in range(2)]
        if far and rng.random() < 0.7:
            p[int(rng.integers(0, 2))] = lo[0 if rng.random() < 0.5 else 1] - float(rng.integers(1, 6)) * reso - 0.5 * reso
            p = [min(p[0], hi[0]), min(p[1], hi[1])]
        return [float(round(v, 4)) for v in p]
    return {"reso": reso, "map_o": map_o, "map_t": map_t, "ori_pre": ori_pre, "pos": point(), "goal": point(), "ifa": int(rng.integers(0, 3)),
            "raw": raw, "prior": prior}


def classify(c, out):
    """What the counted conditions need to know about a case (the test works them out again from the file)."""
    f = {"trunc_off": False, "free_over_occupied": False, "sticks_out": False}
    if c["prior"] is None:
        return f
    o1 = [min(c["map_o"][k], c["ori_pre"][k]) for k in range(2)]
    q = [(c["map_o"][k] - o1[k]) / c["reso"] for k in range(2)] + [(c["ori_pre"][k] - o1[k]) / c["reso"] for k in range(2)]
    f["trunc_off"] = any(int(v) != int(round(v)) for v in q)
    if not out["raises"]:
        at_raw, at_pre = [int(v) for v in q[:2]], [int(v) for v in q[2:]]
        cw = out["canvas_shape"]
        ext_r, ext_p = c["raw"].shape, c["prior"].shape
        f["sticks_out"] = any(at_raw[k] + ext_r[k] > cw[k] or at_pre[k] + ext_p[k] > cw[k] for k in range(2))
        if not f["sticks_out"]:
            only_prior = np.zeros(cw, dtype=np.uint8)
            only_prior[at_pre[0]:at_pre[0] + ext_p[0], at_pre[1]:at_pre[1] + ext_p[1]] = c["prior"]
            under = only_prior[at_raw[0]:at_raw[0] + ext_r[0], at_raw[1]:at_raw[1] + ext_r[1]]
            f["free_over_occupied"] = bool(((under > 0) & (c["raw"] <= 0)).any())
    return f


def main():
    rng = np.random.default_rng(20240611)
    cases, count = [], {"raises": 0, "trunc_off": 0, "free_over_occupied": 0}
    for variant in (0, 1):
        made = 0
        while made < PER_NODE:
            arrange = ARRANGE[made % len(ARRANGE)]
            aligned = (made // len(ARRANGE)) % 3 != 2  # two rounds of origins on the grid, one round off it
            c = make_case(rng, variant, arrange, aligned)
            out = run_ref(variant, c)
            f = classify(c, out)
            if f["sticks_out"]:
                continue  # the reference went on with a clipped rectangle (a side of 1 broadcast into 0): the library deviates there
            if aligned:  # (off the grid every truncation differs from the rounding: that says nothing)
                count["trunc_off"] += f["trunc_off"]
            count["raises"] += out["raises"]
            count["free_over_occupied"] += f["free_over_occupied"]
            rec = {"variant": variant, "arrange": arrange, "aligned": aligned, "reso": float(c["reso"]).hex(), "map_o": hexes(c["map_o"]),
                   "map_t": hexes(c["map_t"]), "ori_pre": hexes(c["ori_pre"]), "pos": hexes(c["pos"]), "goal_xy": hexes(c["goal"]), "ifa": c["ifa"],
                   "raw_shape": list(c["raw"].shape), "raw_hex": c["raw"].astype(np.int8).tobytes().hex(),
                   "prior_shape": None if c["prior"] is None else list(c["prior"].shape),
                   "prior_bits": None if c["prior"] is None else bits(c["prior"])}
            rec.update(out)
            cases.append(rec)
            made += 1
    print(count)
    assert count["raises"] >= 10 and count["trunc_off"] >= 10 and count["free_over_occupied"] >= 10, count
    p = os.path.join(HERE, "worldprep.json")
    with open(p, "w") as f:
        json.dump(cases, f, separators=(",", ":"))
    print("wrote", p, len(cases), "cases", os.path.getsize(p), "bytes")
    assert os.path.getsize(p) <= 200 * 1024


if __name__ == "__main__":
    main()
