"""CPU suite: the grid-slot instantiations of the search kernel (k_search<HC, false, DIRECT, true>: every query reads the
descriptor of its own grid) exist for gfx950, keep to the register budget of the others (<= 128 VGPRs, so that four
wavefronts per SIMD still fit) and use no private segment.  Device pass only, no GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "fuxi-planner_amd", "csrc", "fxjps.hip")
HIPCC = "/opt/rocm/bin/hipcc"


def _resource_usage():
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fvisibility=hidden",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null", SRC],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-1500:]
    rows, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            rows[cur] = {}
            continue
        m = re.search(r":\s+([A-Za-z][^:]*?): (\S+) \[-Rpass", line)
        if m and cur:
            rows[cur][m.group(1).strip()] = m.group(2)
    return rows


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_grid_slot_search_instantiations_fit_the_budget():
    rows = _resource_usage()
    found = {}
    for name, v in rows.items():
        m = re.search(r"k_searchILi(\d)ELb(\d)ELb(\d)ELb(\d)E", name)
        if m and m.group(4) == "1":
            found[(int(m.group(1)), m.group(2) == "1", m.group(3) == "1")] = v
    assert set(found) == {(1, False, False), (1, False, True), (2, False, False), (2, False, True)}, sorted(found)
    for k, v in found.items():
        assert int(v["ScratchSize [bytes/lane]"]) == 0, (k, v)
        assert int(v["VGPRs Spill"]) == 0, (k, v)
        assert int(v["VGPRs"]) <= 128, (k, v)
        assert int(v["Occupancy [waves/SIMD]"]) >= 4, (k, v)
