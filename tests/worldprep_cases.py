"""tests/golden/worldprep.json decoded once for the CPU and the GPU suite of the world-frame calls."""
import functools

import numpy as np

from conftest import load_golden


def unpack(bits_hex, shape):
    W, H = shape
    return np.unpackbits(np.frombuffer(bytes.fromhex(bits_hex), dtype=np.uint8))[:W * H].reshape(W, H)


def floats(hexes):
    return [float.fromhex(h) for h in hexes]


@functools.lru_cache(maxsize=1)
def cases():
    out = []
    for r in load_golden("worldprep.json"):
        c = dict(r)
        c["reso"] = float.fromhex(r["reso"])
        for k in ("map_o", "map_t", "ori_pre", "pos", "goal_xy"):
            c[k] = floats(r[k])
        c["raw"] = np.frombuffer(bytes.fromhex(r["raw_hex"]), dtype=np.int8).reshape(r["raw_shape"]).astype(np.int64)
        c["prior"] = None if r["prior_shape"] is None else unpack(r["prior_bits"], r["prior_shape"])
        if not r["raises"]:
            c["canvas"] = unpack(r["canvas_bits"], r["canvas_shape"])
            c["canvas_o"] = floats(r["canvas_o"])
            if r["prep"] is not None:
                c["prep"] = dict(r["prep"], grid=unpack(r["prep"]["grid_bits"], r["prep"]["grid_shape"]), origin=floats(r["prep"]["origin"]))
        out.append(c)
    return out


def merge_args(c):
    """merge_host's arguments for a case (map_t as the fixture recorded it)."""
    return dict(raw=c["raw"], map_o=c["map_o"], map_reso=c["reso"], pos_xy=c["pos"], goal_xy=c["goal_xy"], prior=c["prior"], ori_pre=c["ori_pre"],
                map_t=c["map_t"])


def placements(c):
    """The four placement quotients of a case with a prior (detected x, y, prior x, y), before truncation."""
    o1 = [min(c["map_o"][k], c["ori_pre"][k]) for k in range(2)]
    return [(c["map_o"][k] - o1[k]) / c["reso"] for k in range(2)] + [(c["ori_pre"][k] - o1[k]) / c["reso"] for k in range(2)]
