"""tests/golden/cropprep.json decoded once for the CPU and the GPU suite of the cropped world-frame calls."""
import functools

import numpy as np

from conftest import load_golden
from worldprep_cases import floats, unpack

OUTCOME = {"planned": 0, "not_planned": 1, "refused": -1}  # FXJPS_OK, FXJPS_JOB_NOT_PLANNED, FXJPS_E_ARG


@functools.lru_cache(maxsize=1)
def cases():
    out = []
    for r in load_golden("cropprep.json"):
        c = dict(r)
        c["reso"] = float.fromhex(r["reso"])
        for k in ("map_o", "ori_pre", "pos", "goal_xy"):
            c[k] = floats(r[k])
        c["raw"] = np.frombuffer(bytes.fromhex(r["raw_hex"]), dtype=np.int8).reshape(r["raw_shape"]).astype(np.int64)
        c["prior"] = None if r["prior_shape"] is None else unpack(r["prior_bits"], r["prior_shape"])
        c["status"] = OUTCOME[r["outcome"]]
        if r.get("crop_o") is not None:
            c["crop_o"], c["crop_t"] = floats(r["crop_o"]), floats(r["crop_t"])
        if r["outcome"] == "planned":
            c["window"] = unpack(r["window_bits"], r["window_shape"])
            c["canvas"] = unpack(r["canvas_bits"], r["canvas_shape"])
            c["canvas_o"] = floats(r["canvas_o"])
            c["prep"] = dict(r["prep"], grid=unpack(r["prep"]["grid_bits"], r["prep"]["grid_shape"]), origin=floats(r["prep"]["origin"]))
        out.append(c)
    return out


def message(c):
    """The case's matrix as the data[] of a nav_msgs/OccupancyGrid: (data, width, height), 1 sent as 100."""
    m = c["raw"]
    return np.where(m == 1, 100, m).astype(np.int8).T.reshape(-1).copy(), int(m.shape[0]), int(m.shape[1])


def bits(v):
    return np.array(v, dtype=np.float64).tobytes()


def check_record(rec, c, where):
    """A crop record (a dict as crop_host returns it) against the case: every field the reference computed."""
    if "bbox" not in c:  # (a refused case: only the inputs and the flag are stored)
        return
    assert list(rec["bbox"]) == c["bbox"] and list(rec["start0"]) == c["start0"], where
    if c["lo"] is not None:
        assert list(rec["lo"]) == c["lo"] and list(rec["win"]) == c["win"], where
        assert bits(rec["map_o"]) == bits(c["crop_o"]) and bits(rec["map_t"]) == bits(c["crop_t"]), where
