"""GPU suite (-m gpu): the search kernel's parity and work identity (test_search_work_gpu) on builds other than the default one.

Every other GPU test runs one build of k_search.  The relax phase of `search_one` orders its vectorised commit with a
slot-collision detector (WaveLds::hz): a ray beaten in two hashed LDS cells is HELD, and a held ray is examined exactly --
a false hold is let go, a pair of rays for one cell is relaxed in the same pass, anything else cuts the committed prefix.
At the default detector sizes (512 / 1024 cells) a second-long test takes these branches a handful of times.  The stress
builds of fuxi-planner_amd/Makefile shrink the detector to 128 cells, 64 per hash, where most iterations with more than a
few relaxing rays hold some; the results must not change, because every hold is resolved exactly:

  libfxjps_hz7.so        -DFXJPS_HZ_LOG2=7 -DFXJPS_HZ_LOG2_DIRECT=7      the shipping kernel, only the detector shrunk
  libfxjps_hz7_prof.so   the same with -DFXJPS_PROF                      ... and the counters that prove the branches ran
  libfxjps_kn32_hz7.so   -DFXJPS_KN=32 and the two detector flags        two-row batches on the small detector
  libfxjps_kn8.so        -DFXJPS_KN=8                                    the width behind the proxy of DESIGN.md section 4

Each library gets one child process (FXJPS_LIB, FXJPS_QSTAT=1) that runs a subset of test_search_work_gpu.SCENARIOS through
its run_scenario: the same assertions, bit for bit against the oracle and per query in pops.  The subset keeps every
instantiation and pool and leaves out the inputs that cost seconds (512x512, 130x2100, the banded far tier, which does not
touch the detector).

The counted run reads, after each scenario, the device counters of the FXJPS_PROF build (Planner.debug_counters):
  [39] iterations with a hold      [35] held rays            [36] held rays that really share a bucket
  [37] pairs relaxed in the pass   [38] iterations cut at an unresolved ray        [31] nodes behind a shared bucket
Summed over each layout group [39], [35] - [36] (the false holds), [36], [37] and [38] must all be > 0: conditions on the
inputs, which say that the branch ran, not how often.  The same scenarios on libfxjps_prof.so give the figures at the
default detector sizes; no stress sum may be below its default sum.

Measured on an MI355X (sums over each group's scenarios; 128 cells / default detector of 1024 or 512 cells):

  group        [39] iterations       [35] held rays        false holds [35]-[36]   [36] real   [37] pairs   [38] cuts   [31] nodes
  slotless     1 346 504 / 978 821   2 942 578 / 1 795 688   1 162 454 / 15 564    1 780 124   1 324 666     136 149    1 104 723
  carrying       558 159 / 479 947   1 309 354 / 1 033 324     299 221 / 23 191    1 010 133     509 498     147 122      972 657
  large pool     306 513 / 285 619     821 131 / 700 633       128 637 /  8 139      692 494     269 170     137 414      760 600

[36], [37], [38] and [31] are the same number on both detectors, as they must be: a real share is held at every size, and a
false hold is let go before it can cut anything, so both builds run the same iterations.  What the small detector adds is
false holds, 13 to 75 times as many.  (So the real shares, the pairs and the cuts are NOT rare at the default size: two nodes
that see one jump point are an everyday event.  The false holds are: under 1 % of the held rays on the slotless layout.)
A child takes about 2 s, a test about 3 s, the counted test with its two children about 5 s.

Two defects of the diagnostic build showed on the first run and are fixed with this test: [36] and [37] were always 0 (their
__ballot sat in DBG_COUNT's argument, evaluated by lane 0 alone), and [39] also collected the clock of r_refill's first mark.
"""
import os
import re
import subprocess
import sys
import time

import pytest

import test_search_work_gpu as work

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "fuxi-planner_amd")

# the layout groups: which open-list layout (and so which detector) the scenario's searches run on
GROUPS = {
    "slotless": ("small 96x80", "small 96x80, slot of 3 cells", "sparse 300x200", "rooms 193x193", "edge batch 96x80", "head launch 256x256", "slots"),
    "carrying": ("tracked small 96x80", "tracked sparse 300x200", "hashed small 96x80", "hashed sparse 300x200", "hashed slots",
                 "hashed tracked small 96x80"),
    "large pool": ("retry sparse 300x200, far tier of 64", "retry sparse 300x200, table of 256"),
}
SELECT = tuple(n for names in GROUPS.values() for n in names)
COUNTERS = (39, 35, 36, 37, 38, 31)
# what must be > 0 per group on the 128-cell detector, and >= the default build's: name -> f(counters by index)
CONDITIONS = {
    "iterations with a hold [39]": lambda c: c[39],
    "false holds [35] - [36]": lambda c: c[35] - c[36],
    "rays really sharing a bucket [36]": lambda c: c[36],
    "pairs relaxed in the pass [37]": lambda c: c[37],
    "iterations cut at an unresolved ray [38]": lambda c: c[38],
}


def selected_names():
    return ["%s h=%d" % (sc[0], h) for sc in work.SCENARIOS if sc[0] in SELECT for h in sc[4]]


# ------------------------------------------------------------------ the child processes
def child_main():
    work.child_main(select=SELECT)


def child_counted():
    """child_main with the counters of the diagnostic build behind every scenario's line.  run_scenario opens its own planner
    and closes it behind the one batch: the counters are read as it closes."""
    import types
    import fuxi_planner_amd as fx
    run = work.run_scenario

    def run_counted(_, oracle, sc, h):
        taken = []

        class Counted(fx.Planner):
            def close(self):
                if getattr(self, "_h", None):
                    taken.append(self.debug_counters())
                super().close()

        line, bad = run(types.SimpleNamespace(Planner=Counted), oracle, sc, h)
        if len(taken) != 1:
            bad.append("the counters were read %d times" % len(taken))
        else:
            line += " | counters " + " ".join("[%d] %d" % (k, int(taken[0][k])) for k in COUNTERS)
        return line, bad

    work.run_scenario = run_counted
    work.child_main(select=SELECT)


# ------------------------------------------------------------------ the parent
def library(name):
    """The path of a stress build; built here if build() has not (a failure of the test, never a skip, if that cannot work)."""
    path = os.path.join(PKG, name)
    if not os.path.exists(path):
        r = subprocess.run(["make", "-C", PKG, name], capture_output=True, text=True)
        assert r.returncode == 0 and os.path.exists(path), (name, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    return path


def run_child(lib, entry="child_main"):
    """One child process on the library `lib`: -> its output, every selected scenario reported ok."""
    env = dict(os.environ, FXJPS_LIB=library(lib), FXJPS_QSTAT="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    t0 = time.time()
    r = subprocess.run([sys.executable, "-c", "import test_search_stress_builds_gpu as t; t.%s()" % entry], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    print("%s: %.1f s" % (lib, time.time() - t0))
    print(r.stdout)
    assert r.returncode == 0, (lib, r.returncode, r.stdout[-6000:], r.stderr[-4000:])
    for name in selected_names():
        assert "work ok  " + name + ":" in r.stdout, (lib, name, r.stdout[-6000:])
    return r.stdout


def group_sums(out):
    """{group: {counter: sum over the group's scenario lines}} of a counted child's output."""
    sums = {}
    for group, names in GROUPS.items():
        c = dict.fromkeys(COUNTERS, 0)
        for sc in work.SCENARIOS:
            if sc[0] not in names:
                continue
            for h in sc[4]:
                lines = [ln for ln in out.splitlines() if ln.startswith("work ok  %s h=%d:" % (sc[0], h))]
                assert len(lines) == 1 and " | counters " in lines[0], (sc[0], h, lines)
                got = {int(k): int(v) for k, v in re.findall(r"\[(\d+)\] (\d+)", lines[0].split(" | counters ")[1])}
                assert sorted(got) == sorted(COUNTERS), (sc[0], h, got)
                for k in COUNTERS:
                    c[k] += got[k]
        sums[group] = c
    return sums


def test_detector_of_128_cells():
    """The shipping kernel with a detector of 128 cells on both layouts: the oracle's bytes and the reference's work."""
    run_child("libfxjps_hz7.so")


def test_detector_of_128_cells_counted():
    """The same on the diagnostic build, and the proof that the rare branches ran: per layout group the holds, the false
    holds, the real shares, the pairs and the cuts are all there, and none of them rarer than on the default detector."""
    stress = group_sums(run_child("libfxjps_hz7_prof.so", "child_counted"))
    default = group_sums(run_child("libfxjps_prof.so", "child_counted"))
    for group in GROUPS:
        for k in COUNTERS:
            print("%-10s [%d] 128 cells %8d   default %8d" % (group, k, stress[group][k], default[group][k]))
    bad = []
    for group in GROUPS:
        for what, f in CONDITIONS.items():
            s, d = f(stress[group]), f(default[group])
            if not s > 0:
                bad.append("%s: %s is %d on the 128-cell detector" % (group, what, s))
            if not s >= d:
                bad.append("%s: %s is %d on the 128-cell detector, %d on the default one" % (group, what, s, d))
    assert not bad, bad


def test_batches_of_32_nodes():
    """Two-row batches (row_dup_cross, the lanes of the second row in the detector) on the 128-cell detector."""
    run_child("libfxjps_kn32_hz7.so")


def test_batches_of_8_nodes():
    """The batch width behind the proxy measurement of DESIGN.md section 4."""
    run_child("libfxjps_kn8.so")
