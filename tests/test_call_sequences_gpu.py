"""GPU suite (-m gpu): random call sequences on ONE handle against the stateless host model of tests/call_sequences.py.

Every other GPU test builds the state it needs, makes its calls in a scripted order and stops.  Here 120 drawn steps (and
a closing round that brings every op kind to three) run on one handle: the resident grid's setters, prepare and refresh
calls, cell updates now and deferred, read-backs, plan_batch / plan_one / plan, set_queries with replan_frame and
replan_frame_raw, every slot call with its world-frame forms, plan_batch_slots and replan_slots with slots rewritten
between them, the waypoint and tick-output calls on the resident paths, and calls that must be refused and touch nothing.
After every step the outputs are byte for byte the C oracle's / the host references' on the model's current bytes, the
flags (kept, the refresh mode and changed cells, out_reused) are those include/fxjps.h states, and the derived maps are
those of oracle/derived_maps.py.  The op list of a seed is the one tests/test_call_sequences_host.py ran on the host twin
and checked for coverage.

Profiles: `single` -- Planner([0]), the generation rule; `tiles` -- the same with set_slot_reuse among the ops;
`two_contexts` -- Planner([0, 0]): replan_slots is a plain batch, every flag 0, context 1's copies are read as well;
`shim` -- the ops run on default_planner() with jps1.method and jps1.method_many among them, the printed costs compared
as test_gpu_parity.py compares them; `world` -- Planner([0]) and `world_two_contexts` -- Planner([0, 0]): the shared
prior maps (set_prior_map / set_prior_image / clear_prior_map, absorb_prior, absorb_prior_grow, absorb_prior_slide with keep
windows and limits of 48 .. 96 cells, get_prior_map, prior_origin), the cropped prepares and check_paths_slots among the
world-frame prepares, replans, read-backs and waypoint calls they interact with.  There every set prior is read back
after each call that writes or is refused on one, the outputs and records of the folds are worldprep's host references'
field by field, and context 1's copy of a prior shows through the slots prepared from it, whose bytes and derived maps
are read on context 1 after every slot write.  No sequence of these two profiles has failed on the library so far.

A failure names seed, step and the ops up to it as Python literals; `replay(ops)` below runs such a list.

Per-test times on an MI355X (pytest's call durations; a sequence is 120 drawn steps plus the forced and the closing
ops): single 0.42 - 0.70 s, tiles 0.41 - 0.53 s, two_contexts 0.73 - 0.92 s, shim 0.45 - 0.56 s, the scripted replay
0.03 s; the file's 17 tests 9.6 s.  With the world profiles: world 0.29 - 0.35 s, world_two_contexts 0.45 - 0.56 s (the
earlier ones in the same run: single 0.41 - 0.68 s, tiles 0.39 - 0.50 s, two_contexts 0.74 - 0.96 s, shim 0.42 - 0.54 s); the
file's 25 tests 12.8 s.

The order test_st_rule_on_resident_paths_after_a_smaller_grid replays: fxjps_waypoint_st_batch on resident paths has to size
its table of angles from the grid the batch ran on, not from the one resident now -- else, on a handle whose table is
still small, the angles of cells beyond the resident grid are read clamped and the waypoints are well-formed and wrong.
Half of the sequences begin on a small grid, so that no early call leaves a large table behind.
"""
import numpy as np
import pytest

import call_sequences as cs
from call_sequences import SEEDS, STEPS

pytestmark = pytest.mark.gpu


def replay(ops, oracle, devices=(0,)):
    """Run an op list on a new handle."""
    import fuxi_planner_amd as fx
    dev = list(devices)
    with fx.Planner(dev) as p:
        return cs.run(p, ops, oracle, fresh=lambda: fx.Planner(dev), contexts=len(dev), seed="replay")


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("profile", ["single", "tiles", "two_contexts"])
def test_sequence_on_one_handle(oracle, profile, seed):
    import fuxi_planner_amd as fx
    dev = [0, 0] if profile == "two_contexts" else [0]
    with fx.Planner(dev) as p:
        cs.run(p, cs.generate(seed, STEPS, profile), oracle, fresh=lambda: fx.Planner(dev), contexts=len(dev), seed=(profile, seed))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("profile", ["world", "world_two_contexts"])
def test_world_sequence_on_one_handle(oracle, profile, seed):
    """The shared prior maps as the most mutable state of a handle: absorbed into, grown, slid, uploaded again and
    released between the world-frame and cropped prepares that read them, the replans that must not notice and the
    path checks on slots rewritten since their batch."""
    import fuxi_planner_amd as fx
    dev = [0, 0] if profile == "world_two_contexts" else [0]
    with fx.Planner(dev) as p:
        cs.run(p, cs.generate(seed, STEPS, profile), oracle, fresh=lambda: fx.Planner(dev), contexts=len(dev), seed=(profile, seed))


@pytest.mark.parametrize("seed", SEEDS)
def test_sequence_through_the_shim(oracle, seed):
    """The process-wide planner of the jps1 shim: other tests have used it, so the slots the sequences name are emptied
    first; the first ops of every sequence set the grid, the queries and the slots they rely on."""
    import fuxi_planner_amd as fx
    p = fx.default_planner()
    for s in tuple(range(cs.NSLOTS)) + cs.EMPTY_SLOTS:
        p.clear_grid_slot(s)
    p.set_slot_reuse("generation")
    cs.run(p, cs.generate(seed, STEPS, "shim"), oracle, fresh=lambda: fx.Planner([0]), seed=("shim", seed))


def test_st_rule_on_resident_paths_after_a_smaller_grid(oracle):
    """A scripted order: paths planned on a 100 x 120 grid, a 4 x 5 grid made resident, the st rule on the resident paths.
    The rule's table of angles has to cover the grid the PATHS lie on, not the one that is resident now (on a new
    handle no earlier call has left a larger table behind)."""
    s = [[1, 1], [98, 3], [50, 60], [3, 117], [97, 118], [10, 80], [60, 5], [33, 33]]
    g = [[97, 117], [2, 115], [5, 5], [95, 4], [4, 2], [90, 30], [20, 110], [70, 99]]
    ops = [{"op": "set_grid_occ", "g": {"W": 100, "H": 120, "seed": 5, "p": 0.2, "set": []}},
           {"op": "plan_batch", "s": s, "g": g, "hchoice": 2, "mpl": None},
           {"op": "set_grid_occ", "g": {"W": 4, "H": 5, "seed": 6, "p": 0.0, "set": []}},
           {"op": "select_st_batch", "nq": 8, "seed": 11, "end_occu": False, "prev": False},
           {"op": "select_st_batch", "nq": 8, "seed": 12, "end_occu": True, "prev": True}]
    replay(ops, oracle)
