"""bench.py with and without --full: a plain run sets up, warms up, times its steps and prints its line; the CPU baselines,
config.also and every other measurement or check around the timed steps are behind --full."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
PLAIN_BUDGET_S = 30.0  # a plain run outside its steps: start to exit less (steps + warmup) * ms_per_step


def _bench(*args):
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), wall


def test_full_is_an_option_of_the_benchmark():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.gpu
def test_plain_run_is_lean_and_full_carries_what_moved(tmp_path):
    """Plain: the headline keys, the dumped arrays, no CPU baseline, no config.also, at most 30 s outside the steps.
    --full (here with a small CPU sample and without config.also, which is minutes of other workloads): the same keys plus
    the CPU baselines, whose legs check the last step against the oracle."""
    steps, warmup = 3, 1
    plain, wall = _bench("--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path / "dump"))
    outside = wall - (steps + warmup) * plain["ms_per_step"] * 1e-3
    print("plain run: %.1f s from start to exit, %.1f s of them outside its %d steps of %.1f ms" % (wall, outside, steps + warmup, plain["ms_per_step"]))
    assert all(k in plain for k in HEADLINE) and plain["steps"] == steps and plain["warmup"] == warmup
    assert plain["metric"] == "start->goal plans/sec on 1024x1024 grid" and plain["unit"] == "plans/s" and plain["dtype"] == "f64"
    assert plain["higher_is_better"] is True and plain["value"] > 0
    assert "cpu_baseline" not in plain and "cpu_baseline_python" not in plain and "also" not in plain["config"]
    assert sorted(os.listdir(str(tmp_path / "dump"))) == ["cells.npy", "cost.npy", "offsets.npy", "query_ids.npy", "status.npy"]
    assert outside <= PLAIN_BUDGET_S

    full, _ = _bench("--gpus", "1", "--steps", "1", "--warmup", "1", "--full", "--no-also", "--cpu-sample", "500", "--py-sample", "4")
    assert all(k in full for k in HEADLINE) and [full[k] for k in HEADLINE[:5] if k != "value"] == [plain[k] for k in HEADLINE[:5] if k != "value"]
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline_python"]["value"] > 0 and "also" not in full["config"]
