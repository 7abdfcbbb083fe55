#!/usr/bin/env python3
"""Golden vectors for the ccst node's crop in front of the world-frame calls, produced by
EXECUTING the reference's own lines, read from /root/reference at generation time, dedented and exec'ed on prepared inputs:
    the crop                 scripts/global_planner_ccst.py:36-63   (remove_zero_rowscols; comment-only lines dropped
                                                                     before dedenting: line 62 sits at column 0)
    whether the node plans   scripts/global_planner_ccst.py:351     (the condition of that line, evaluated as it stands)
    merge, world -> cell and the preparation                        (the blocks make_golden_worldprep.py reads, through its
                                                                     run_ref, on the window and the moved map_o / map_t)
Only inputs and outputs are stored (tests/golden/cropprep.json): the message as int8 hex, grids bit-packed, every float
as float.hex().

    python tests/golden/make_golden_cropprep.py
"""
import json
import os
import re
import sys
import textwrap
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_worldprep as W  # noqa: E402

NAME = "global_planner_ccst.py"
CLASSES = ("planned", "planned_prior", "none", "win_zero", "narrow", "lo_negative", "vehicle_decides")
PER_CLASS = 15
I32_MAX = 2147483647


def ref_lines(lo, hi):
    with open(os.path.join(W.REF, NAME), encoding="utf-8", errors="replace") as f:
        return f.readlines()[lo - 1:hi]


def crop_function():
    """remove_zero_rowscols as the reference defines it."""
    src = "".join(l for l in ref_lines(36, 63) if not l.lstrip().startswith("#"))
    ns = {"np": np}
    exec(compile(textwrap.dedent(src), "%s:36-63" % NAME, "exec"), ns)
    return ns["remove_zero_rowscols"]


def plans_condition():
    """The condition of ccst:351, without its `if`, its colon and the comment behind it."""
    line = ref_lines(351, 351)[0]
    m = re.match(r"\s*if (.*\)):\s*(#.*)?$", line)
    assert m, line
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (`is not 0`)
        return compile(m.group(1), "%s:351" % NAME, "eval")


def run_ref(crop, cond, c):
    """-> the record's outputs."""
    planner = W._O()
    planner.map_o = list(c["map_o"])  # (map_callback, ccst:26-28)
    planner.map_reso = c["reso"]
    planner.map_c1, planner.map_r1 = c["raw"].shape
    planner.if_map_pub = 1
    planner.pos = object()
    px, py = c["pos"]
    _stdout, sys.stdout = sys.stdout, open(os.devnull, "w")
    try:
        mapu = crop(planner, c["raw"], px, py)
    finally:
        sys.stdout.close()
        sys.stdout = _stdout
    nzx, nzy = c["raw"].nonzero()
    none = len(nzx) == 0
    assert none == isinstance(mapu, int)
    bbox = [I32_MAX, I32_MAX, -1, -1] if none else [int(nzx.min()), int(nzy.min()), int(nzx.max()), int(nzy.max())]
    start0 = [int(v) for v in ((np.array([px, py]) - np.array(c["map_o"])) / c["reso"]).astype(int)]  # ccst:47, for the record
    out = {"bbox": bbox, "start0": start0}
    plans = bool(eval(cond, {"mapu": mapu, "planner": planner, "global_goal": np.array([c["goal"][0], c["goal"][1], 1.5]), "ifa": c["ifa"]}))
    if none:
        out.update(outcome="not_planned", lo=None, win=None, crop_o=None, crop_t=None)
        assert not plans
        return out
    win = [int(planner.map_c), int(planner.map_r)]
    lo = [bbox[2] - win[0], bbox[3] - win[1]]
    out.update(lo=lo, win=win, crop_o=W.hexes(planner.map_o), crop_t=W.hexes(planner.map_t))
    if not plans:
        out["outcome"] = "not_planned"
        return out
    if min(lo) < 0:  # the slice counted from the end: what the reference does from here on is not the crop
        out["outcome"] = "refused"
        return out
    assert mapu.shape == tuple(win)
    out.update(outcome="planned", window_shape=list(mapu.shape), window_bits=W.bits(mapu != 0))
    w = W.run_ref(1, dict(c, raw=np.array(mapu), map_o=list(planner.map_o), map_t=list(planner.map_t)))
    if w["raises"] or w["prep"] is None:
        return None
    if c["prior"] is not None:
        o1 = [min(planner.map_o[k], c["ori_pre"][k]) for k in range(2)]
        at = [int((planner.map_o[k] - o1[k]) / c["reso"]) for k in range(2)] + [int((c["ori_pre"][k] - o1[k]) / c["reso"]) for k in range(2)]
        cw = w["canvas_shape"]
        if any(at[k] + win[k] > cw[k] or at[2 + k] + c["prior"].shape[k] > cw[k] for k in range(2)):
            return None  # the reference went on with a clipped rectangle: the library deviates there
    out.update(w)
    return out


def make_case(rng, want):
    reso = float(rng.choice(W.RESOS))
    aligned = rng.random() < 0.6
    W0, H0 = int(rng.integers(1, 21)), int(rng.integers(1, 21))
    ifa = int(rng.integers(0, 3))
    if want == "narrow":
        ifa = int(rng.integers(1, 3))
        W0 = int(rng.integers(1, 2 * ifa + 1))
    elif want not in ("none", "win_zero"):
        W0, H0 = max(W0, 2 * ifa + 2), max(H0, 3)
    raw = np.zeros((W0, H0), dtype=np.int64)
    if want != "none":
        x0, y0 = int(rng.integers(0, W0)), int(rng.integers(0, H0))
        x1, y1 = int(rng.integers(x0, W0)) + 1, int(rng.integers(y0, H0)) + 1
        if want == "win_zero" and rng.random() < 0.7:
            if rng.random() < 0.5:
                x1 = x0 + 1
            else:
                y1 = y0 + 1
        raw[x0:x1, y0:y1] = rng.choice(np.array([0, 0, 0, 1, 1, 50, 3], dtype=np.int64), size=(x1 - x0, y1 - y0))
        if want in ("narrow", "win_zero", "lo_negative", "vehicle_decides", "planned", "planned_prior") and not raw.any():
            raw[x0, y0] = 1
    ko = [int(rng.integers(-120, 40)), int(rng.integers(-120, 40))]
    off = [0.0, 0.0] if aligned else [float(rng.choice([0.03, 0.07, 0.013])), float(rng.choice([0.02, 0.041, 0.009]))]
    map_o = [W.dec(ko[0], reso, off[0]), W.dec(ko[1], reso, off[1])]
    # the vehicle: mostly inside the message, every cell equally likely; where a class asks for it, left of / below the
    # origin, or inside and in front of the first non-zero cell on an axis
    cell = [float(rng.integers(0, W0)) + float(rng.random()), float(rng.integers(0, H0)) + float(rng.random())]
    nz = raw.nonzero()
    if want == "lo_negative":
        cell[int(rng.integers(0, 2))] = -float(rng.integers(1, 5)) - float(rng.random())
    elif want == "vehicle_decides" and len(nz[0]):
        k = int(rng.integers(0, 2))
        first = int(nz[k].min())
        if first == 0:
            return None
        cell[k] = float(rng.integers(0, first)) + 0.5
    pos = [float(round(map_o[k] + cell[k] * reso, 4)) for k in range(2)]
    goal = [float(round(map_o[0] + float(rng.uniform(-3, W0 + 3)) * reso, 4)), float(round(map_o[1] + float(rng.uniform(-3, H0 + 3)) * reso, 4))]
    prior = None
    ori_pre = [-15.0, -15.0]
    if want == "planned_prior" or (want != "planned" and rng.random() < 0.5):
        l1, l2 = int(rng.integers(1, 25)), int(rng.integers(1, 25))
        kp = [ko[0] + int(rng.integers(-8, 12)), ko[1] + int(rng.integers(-8, 12))]
        off_p = [0.0, 0.0] if aligned else [float(rng.choice([0.0, 0.01, 0.06])), float(rng.choice([0.0, 0.033, 0.017]))]
        ori_pre = [W.dec(kp[0], reso, off_p[0]), W.dec(kp[1], reso, off_p[1])]
        prior = (rng.random((l1, l2)) < 0.35).astype(np.uint8)
    return {"reso": reso, "aligned": bool(aligned), "map_o": map_o, "ori_pre": ori_pre, "pos": pos, "goal": goal, "ifa": ifa, "raw": raw, "prior": prior}


def classify(c, out):
    if out["outcome"] == "refused":
        return "lo_negative"
    if out["outcome"] == "not_planned":
        if out["bbox"][2] < 0:
            return "none"
        return "win_zero" if out["win"][0] * out["win"][1] <= 0 else "narrow"
    if any(out["start0"][k] < out["bbox"][k] for k in range(2)):
        return "vehicle_decides"
    return "planned" if c["prior"] is None else "planned_prior"


def main():
    rng = np.random.default_rng(20240790)
    crop, cond = crop_function(), plans_condition()
    cases, count = [], {k: 0 for k in CLASSES}
    while min(count.values()) < PER_CLASS:
        want = min(CLASSES, key=lambda k: count[k])
        c = make_case(rng, want)
        if c is None:
            continue
        out = run_ref(crop, cond, c)
        if out is None:
            continue
        cls = classify(c, out)
        if count[cls] >= PER_CLASS + 3:
            continue
        count[cls] += 1
        rec = {"cls": cls, "aligned": c["aligned"], "reso": float(c["reso"]).hex(), "map_o": W.hexes(c["map_o"]), "ori_pre": W.hexes(c["ori_pre"]),
               "pos": W.hexes(c["pos"]), "goal_xy": W.hexes(c["goal"]), "ifa": c["ifa"], "raw_shape": list(c["raw"].shape),
               "raw_hex": c["raw"].astype(np.int8).tobytes().hex(), "prior_shape": None if c["prior"] is None else list(c["prior"].shape),
               "prior_bits": None if c["prior"] is None else W.bits(c["prior"])}
        if cls == "lo_negative":  # only the inputs and the flag
            out = {"outcome": "refused"}
        out.pop("raises", None)
        rec.update(out)
        cases.append(rec)
    print(count)
    assert all(v >= PER_CLASS for v in count.values()), count
    p = os.path.join(HERE, "cropprep.json")
    with open(p, "w") as f:
        json.dump(cases, f, separators=(",", ":"))
    print("wrote", p, len(cases), "cases", os.path.getsize(p), "bytes")
    assert os.path.getsize(p) <= 200 * 1024


if __name__ == "__main__":
    main()
