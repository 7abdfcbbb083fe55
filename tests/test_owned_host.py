"""CPU suite: the move-only owners behind every buffer, stream and event of a handle (fuxi-planner_amd/csrc/fxjps_owned.h,
DESIGN.md section 8b) as a stand-alone host program under AddressSanitizer + UBSan: tests/owned_check.cpp puts malloc / free
and counting stand-ins in place of the runtime's calls and checks that moves, self-assignment, std::swap, growth, a refused
allocation and a resized vector of holders free every allocation exactly once."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owners_free_everything_exactly_once(tmp_path):
    exe = str(tmp_path / "owned_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(ROOT, "tests", "owned_check.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("owned ok"), r.stdout
