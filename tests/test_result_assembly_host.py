"""CPU suite: the host assembly of a streamed batch's results (fuxi-planner_amd/csrc/fxjps_results.h)
as a stand-alone host program under AddressSanitizer + UBSan.  tests/result_assembly_check.cpp hands it lengths with zeros
and negative status codes between the paths, arena pieces in an order unrelated to query order, a length-1 path,
max_len-long paths, a split over 1, 3 and 8 threads that must give identical output, and overflow marks (base < 0) that
must be reported and not read."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_result_assembly_under_sanitizers(tmp_path):
    exe = str(tmp_path / "result_assembly_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "result_assembly_check.cpp")],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("result assembly ok"), r.stdout
