"""GPU suite (-m gpu): every derived map of the device -- neighbour bytes, straight and diagonal scan words, cell infos, jump
distances, component forest -- against the host reference of oracle/derived_maps.py, which packs the C oracle's own
jump() / forced / dblock answers and components into the documented layouts.  The device-against-device comparisons of
test_map_updates_gpu.py share every per-item map function between their two sides; these do not.

Shapes where map kernels go wrong: lines that cross a 64-bit word, H not a multiple of 64 (label runs across rows), the
first diagonal step of a checkerboard, the 13-bit distance field at 8190 cells a side, the read-set tile shift at every
size.  Build paths: the fused and the separate build, the waiting and the queued fxjps_set_grid, device grids, prepared
grids, images, slots.  After cell updates in every jump-distance mode, deferred, by replan_frame, with repeated cells.
Tests whose names end in `_and_plans` also run the search; the others only build and read maps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import derived_maps as dm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_maps(dev, occ, tag, comp="exact", ever_free=None):
    ref = dm.reference_maps(occ)
    msg = dm.first_difference(dev, ref)
    assert msg is None, (tag, occ.shape, msg)
    if comp is not None:
        msg = dm.component_problem(dev["comp"], occ, exact=comp == "exact", ever_free=ever_free)
        assert msg is None, (tag, occ.shape, "comp", msg)


def checkerboard(W, H, phase=0):
    return ((np.add.outer(np.arange(W), np.arange(H)) + phase) % 2).astype(np.uint8)


def maze():
    """The structured maze of test_gpu_parity.test_structured_maps_vs_oracle."""
    occ = np.zeros((193, 193), dtype=np.uint8)
    occ[::16, :] = 1
    occ[:, ::16] = 1
    rng = np.random.default_rng(3)
    for k in range(1, 12):
        for j in range(12):
            occ[16 * k, 16 * j + int(rng.integers(1, 16))] = 0
            occ[16 * j + int(rng.integers(1, 16)), 16 * k] = 0
    occ[100:110, 100:110] = 1
    occ[103:106, 103:106] = 0
    return occ


def png_maps():
    """The reference's 35 maps and the 256 x 256 canvas of config 1."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "maps_png.npz"))
    with open(os.path.join(ROOT, "tests", "golden", "maps_png.json")) as f:
        recs = json.load(f)
    out = []
    for nm in z.files:
        W, H = [r for r in recs if r["map"] == nm and "canvas" not in r][0]["shape"]
        out.append(np.unpackbits(z[nm])[:W * H].reshape(W, H).astype(np.uint8))
        if nm == "-16.20-11.40_out.png":
            canvas = np.zeros((256, 256), np.uint8)
            canvas[:147, :112] = out[-1]
            out.append(canvas)
    return out


def small_shapes():
    """Grids the fused build and the queued set_grid take (at most 2^18 cells)."""
    rng = np.random.default_rng(41)
    out = []
    sides = (61, 62, 63, 64, 126, 127, 128)  # W + 2 / H + 2 around a multiple of 64
    for i, W in enumerate(sides):
        for j, H in enumerate(sides):
            out.append((rng.random((W, H)) < (0.2, 0.45, 0.05)[(i + j) % 3]).astype(np.uint8))
    for W, H, d in ((500, 3, 0.1), (300, 37, 0.35), (1000, 1, 0.05), (1, 1, 0.0), (1, 1, 1.0), (1, 2, 0.0), (2, 1, 0.0),
                    (1, 2, 0.5), (2, 1, 0.5), (300, 300, 0.0), (70, 90, 1.0)):
        out.append((rng.random((W, H)) < d).astype(np.uint8))
    out += [checkerboard(100, 62), checkerboard(65, 66, 1), checkerboard(127, 3), maze()]
    return out


def large_shapes():
    from fuxi_planner_amd import synth
    rng = np.random.default_rng(43)
    out = [np.zeros((1, 8190), np.uint8), np.zeros((8190, 1), np.uint8), (rng.random((8190, 3)) < 0.01).astype(np.uint8),
           synth.synth_grid(1024, 1024, 2, 0.20), (rng.random((700, 333)) < 0.3).astype(np.uint8),
           (rng.random((130, 2100)) < 0.15).astype(np.uint8)]
    return out


@pytest.mark.parametrize("build", ["queued", "wait", "separate"])
def test_set_grid_maps_equal_host_reference(build, monkeypatch):
    """fxjps_set_grid on small grids: the queued call (returns with the build queued) and the waiting one
    (FXJPS_SETGRID_WAIT=1) of the fused four-launch build, and the eight separate kernels (FXJPS_FUSED_BUILD=0)."""
    import fuxi_planner_amd as fx
    if build == "wait":
        monkeypatch.setenv("FXJPS_SETGRID_WAIT", "1")
    if build == "separate":
        monkeypatch.setenv("FXJPS_FUSED_BUILD", "0")
    grids = small_shapes() + (png_maps() if build != "separate" else png_maps()[::4])
    with fx.Planner([0]) as p:
        for i, g in enumerate(grids):
            p.set_grid_occ(g)
            check_maps(p.debug_maps(), g, (build, i))


def test_large_grids_equal_host_reference():
    """The largest side (1 x 8190 and 8190 x 1 empty: a ray 8190 cells long in the 13-bit field; 8190 x 3), config 2,
    700 x 333, 130 x 2100 and a config-3 grid (4096^2 at 20 %, tsh = 6)."""
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import synth
    with fx.Planner([0]) as p:
        for g in large_shapes() + [synth.synth_grid(4096, 4096, 2, 0.20)]:
            p.set_grid_occ(g)
            check_maps(p.debug_maps(), g, ("large", g.shape))


def test_prepared_and_image_grids_equal_host_reference():
    """prepare_grid / prepare_occupancy_msg (against the prepared grid get_grid returns) and set_grid_image."""
    import fuxi_planner_amd as fx
    rng = np.random.default_rng(47)
    with fx.Planner([0]) as p:
        for it in range(8):
            W0, H0 = int(rng.integers(20, 200)), int(rng.integers(20, 200))
            raw = (rng.random((W0, H0)) < 0.06).astype(np.uint8)
            start, goal = (int(rng.integers(0, W0)), int(rng.integers(0, H0))), (int(rng.integers(0, W0)), int(rng.integers(0, H0)))
            if it % 2 == 0:
                p.prepare_grid(raw, start, goal, 1 + it % 3, it % 4 // 2)
            else:
                data = np.where(raw.T > 0, 100, np.where(rng.random((H0, W0)) < 0.1, -1, 0)).astype(np.int8).reshape(-1)
                p.prepare_occupancy_msg(data, W0, H0, start, goal, 1 + it % 3, it % 4 // 2)
            g = p.get_grid()
            check_maps(p.debug_maps(), g, ("prepared", it))
        for rows, cols in ((70, 130), (1, 64), (127, 1), (300, 257)):
            gray = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
            p.set_grid_image(gray)
            g = (gray[::-1].T <= 200).astype(np.uint8)
            assert np.array_equal(p.get_grid(), g)
            check_maps(p.debug_maps(), g, ("image", rows, cols))


_DEVICE = r'''
import sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import numpy as np
import torch
import fuxi_planner_amd as fx
from test_derived_maps_gpu import check_maps
rng = np.random.default_rng(53)
with fx.Planner([0]) as p:
    for W, H, d in ((300, 260, 0.2), (63, 127, 0.4), (1, 700, 0.1), (600, 600, 0.25)):
        occ = (rng.random((W, H)) < d).astype(np.uint8)
        buf = torch.from_numpy(occ.reshape(-1).copy()).to("cuda:0")
        torch.cuda.synchronize()
        p.set_grid_device(buf.data_ptr(), W, H)
        check_maps(p.debug_maps(), occ, ("device", W, H))
        del buf
print("DEVICE-MAPS-OK")
'''


def test_device_grid_maps_equal_host_reference(tmp_path):
    """fxjps_set_grid_device (a torch buffer; own process: torch's HIP runtime must initialise first)."""
    pytest.importorskip("torch")
    script = tmp_path / "device_maps.py"
    script.write_text(_DEVICE % {"root": ROOT, "tests": os.path.join(ROOT, "tests")})
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "DEVICE-MAPS-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_slot_maps_equal_host_reference():
    """Grid slots of different shapes on one handle, set in turn and one replaced by another shape."""
    import fuxi_planner_amd as fx
    rng = np.random.default_rng(59)
    grids = {0: (rng.random((127, 64)) < 0.3).astype(np.uint8), 3: checkerboard(66, 130), 17: maze(),
             255: (rng.random((500, 3)) < 0.1).astype(np.uint8), 9: (rng.random((1024, 700)) < 0.2).astype(np.uint8)}
    with fx.Planner([0]) as p:
        p.set_grid_occ(np.zeros((5, 5), np.uint8))
        for s, g in grids.items():
            p.set_grid_slot(s, g)
        grids[3] = (rng.random((61, 200)) < 0.25).astype(np.uint8)
        p.set_grid_slot(3, grids[3])
        for s, g in grids.items():
            check_maps(p.debug_slot_maps(s), g, ("slot", s))
        check_maps(p.debug_maps(), np.zeros((5, 5), np.uint8), "resident beside the slots")


def random_update(rng, cur, kind):
    W, H = cur.shape
    if kind == 0:  # a window, all its cells sent
        w = int(rng.integers(1, min(48, W, H) + 1))
        x0, y0 = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - w + 1))
        xs, ys = np.meshgrid(np.arange(x0, x0 + w), np.arange(y0, y0 + w), indexing="ij")
        xy = np.stack([xs.ravel(), ys.ravel()], 1)
        return xy, (rng.random(len(xy)) < 0.3).astype(np.uint8)
    if kind == 1:  # one cell flipped
        xy = np.array([[int(rng.integers(0, W)), int(rng.integers(0, H))]])
        return xy, (1 - cur[xy[:, 0], xy[:, 1]]).astype(np.uint8)
    if kind == 2:  # scattered cells, each named several times: the last entry wins
        cells = np.stack([rng.integers(0, W, 12), rng.integers(0, H, 12)], 1)
        xy = cells[rng.integers(0, 12, 80)]
        return xy, rng.integers(0, 2, 80).astype(np.uint8)
    # a line across the map, set or cleared
    if rng.random() < 0.5:
        x = int(rng.integers(0, W))
        xy = np.stack([np.full(H, x), np.arange(H)], 1)
    else:
        y = int(rng.integers(0, H))
        xy = np.stack([np.arange(W), np.full(W, y)], 1)
    return xy, np.full(len(xy), int(rng.integers(0, 2)), np.uint8)


def update_grids(large):
    rng = np.random.default_rng(61)
    out = [(rng.random((127, 64)) < 0.2).astype(np.uint8), (rng.random((62, 128)) < 0.4).astype(np.uint8),
           (rng.random((300, 37)) < 0.35).astype(np.uint8), (rng.random((500, 3)) < 0.1).astype(np.uint8),
           (rng.random((1000, 1)) < 0.05).astype(np.uint8), (rng.random((2, 1)) < 0.5).astype(np.uint8),
           checkerboard(100, 62), maze(), np.zeros((300, 300), np.uint8), png_maps()[-1],
           (rng.random((130, 2100)) < 0.15).astype(np.uint8), (rng.random((3, 2000)) < 0.02).astype(np.uint8),
           np.zeros((1, 8190), np.uint8)]
    if large:
        from fuxi_planner_amd import synth
        out += [synth.synth_grid(1024, 1024, 2, 0.20), (rng.random((700, 333)) < 0.3).astype(np.uint8)]
    return out


@pytest.mark.parametrize("jd_mode", ["walk", "walk_max_3", "walk_max_3_no_list", "stream"])
def test_updated_maps_equal_host_reference(jd_mode, monkeypatch):
    """After cell updates (windows, single cells, lists that repeat cells, lines; some deferred): nb8, bm, ci, dbm and jd
    exactly those of the updated grid, the forest sound (every host component under one root, every free cell with
    one, no root on a cell never free since the last full labelling).  jd modes as in
    test_partial_rebuild_equals_fresh_upload."""
    import fuxi_planner_amd as fx
    if jd_mode.startswith("walk_max_3"):
        monkeypatch.setenv("FXJPS_JD_WALK_MAX", "3")
        monkeypatch.setenv("FXJPS_JD_STREAM_DIV", "1")
        if jd_mode.endswith("no_list"):
            monkeypatch.setenv("FXJPS_JD_OVF_CAP", "0")
    elif jd_mode == "stream":
        monkeypatch.setenv("FXJPS_JD_WALK", "0")
    rng = np.random.default_rng(67)
    with fx.Planner([0]) as p:
        for gi, cur in enumerate(update_grids(large=jd_mode == "walk")):
            p.set_grid_occ(cur)
            ever_free = cur == 0
            for step in range(8):
                xy, val = random_update(rng, cur, step % 4)
                cur[xy[:, 0], xy[:, 1]] = val
                ever_free |= cur == 0
                rebuild = step % 3 != 1
                p.update_cells(xy.astype(np.int32), val, rebuild=rebuild)
                if rebuild:
                    check_maps(p.debug_maps(), cur, (jd_mode, gi, step), comp="sound", ever_free=ever_free)


def test_replan_frame_updates_and_plans(oracle):
    """replan_frame carrying updates: the maps of the updated grid, and the plans the oracle makes on it."""
    import fuxi_planner_amd as fx
    from fuxi_planner_amd import synth
    rng = np.random.default_rng(71)
    cur = (rng.random((200, 127)) < 0.25).astype(np.uint8)
    s, g = synth.synth_queries(cur, 5, 200)
    with fx.Planner([0]) as p:
        p.set_grid_occ(cur)
        p.set_queries(s, g, 2)
        ever_free = cur == 0
        for step in range(6):
            xy, val = random_update(rng, cur, step % 4)
            cur[xy[:, 0], xy[:, 1]] = val
            ever_free |= cur == 0
            off, cells, cost, st = p.replan_frame(xy.astype(np.int32), val)
            check_maps(p.debug_maps(), cur, ("replan", step), comp="sound", ever_free=ever_free)
            oc, ol, ocost, _ = oracle.plan_batch(cur, s, g, 2, literal=False, max_len=max(int(st.max()), 1) + 8, nthreads=8)
            assert np.array_equal(st, ol) and cost.tobytes() == ocost.tobytes(), step
            for q in range(len(s)):
                assert np.array_equal(cells[off[q]:off[q + 1]], oc[q, :max(int(ol[q]), 0)]), (step, q)


def test_components_after_updates_and_relabelling():
    """Small updates are united into the forest (sound); the 65th small update in a row -- 64 are taken incrementally --
    and any update of more than 8192 cells relabel the map within the same update_cells call, exact again.  A large
    DEFERRED update is relabelled by the next call that rebuilds the maps: the read of the maps itself is one."""
    import fuxi_planner_amd as fx
    rng = np.random.default_rng(73)
    with fx.Planner([0]) as p:
        cur = (rng.random((300, 37)) < 0.45).astype(np.uint8)  # many small components, H not a multiple of 64
        p.set_grid_occ(cur)
        check_maps(p.debug_maps(), cur, "fresh")
        ever_free = cur == 0
        for step in range(65):
            xy = np.array([[int(rng.integers(0, 300)), int(rng.integers(0, 37))]])
            val = (1 - cur[xy[:, 0], xy[:, 1]]).astype(np.uint8)
            cur[xy[:, 0], xy[:, 1]] = val
            ever_free |= cur == 0
            p.update_cells(xy.astype(np.int32), val)
            dev = p.debug_maps()
            msg = dm.component_problem(dev["comp"], cur, exact=step == 64, ever_free=ever_free)
            assert msg is None, (step, msg)
        check_maps(p.debug_maps(), cur, "after the 65th small update")
        idx = rng.choice(300 * 37, 9000, replace=False)  # more than 8192 cells
        xy = np.stack([idx // 37, idx % 37], 1).astype(np.int32)
        val = (rng.random(9000) < 0.45).astype(np.uint8)
        cur[xy[:, 0], xy[:, 1]] = val
        p.update_cells(xy, val)
        check_maps(p.debug_maps(), cur, "after a large update")
        idx = rng.choice(300 * 37, 9000, replace=False)
        xy = np.stack([idx // 37, idx % 37], 1).astype(np.int32)
        val = (rng.random(9000) < 0.45).astype(np.uint8)
        cur[xy[:, 0], xy[:, 1]] = val
        p.update_cells(xy, val, rebuild=False)
        assert np.array_equal(p.get_grid(), cur)
        check_maps(p.debug_maps(), cur, "after a large deferred update")


def test_door_between_components_and_plans(oracle):
    """A wall with one door: closed at the start (two components), opened by a one-cell update (the forest must unite
    them, or a reachable goal is answered "no path"), closed, reopened.  Forest checked each time, queries across the
    door planned against the oracle."""
    import fuxi_planner_amd as fx
    from test_gpu_parity import gpu_vs_oracle
    W, H = 130, 70
    cur = np.zeros((W, H), np.uint8)
    cur[65, :] = 1
    door = (65, 33)
    rng = np.random.default_rng(79)
    left = np.stack([rng.integers(0, 65, 40), rng.integers(0, H, 40)], 1).astype(np.int32)
    right = np.stack([rng.integers(66, W, 40), rng.integers(0, H, 40)], 1).astype(np.int32)
    s, g = np.concatenate([left, right]), np.concatenate([right, left])
    with fx.Planner([0]) as p:
        p.set_grid_occ(cur)
        check_maps(p.debug_maps(), cur, "closed")
        ever_free = cur == 0
        _, _, _, st = gpu_vs_oracle(p, oracle, cur, s, g, 2)
        assert (st == 0).all()
        for step, v in enumerate((0, 1, 0)):
            p.update_cells(np.array([door], np.int32), np.array([v], np.uint8))
            cur[door] = v
            ever_free |= cur == 0
            dev = p.debug_maps()
            check_maps(dev, cur, ("door", step, v), comp="sound", ever_free=ever_free)
            if v == 0:
                r = dm.roots(dev["comp"]).reshape(W, H)
                assert r[0, 0] == r[W - 1, H - 1] >= 0, step
            _, _, _, st = gpu_vs_oracle(p, oracle, cur, s, g, 2)
            assert ((st > 0) if v == 0 else (st == 0)).all(), step
