"""host/worklist_selftest.cpp: the work lists of the persistent filter launch (csrc/apss_worklist.hpp) against the grid they
replace -- every round of every working cell covered exactly once, no item of a symmetric join across a query tile, cut
pieces last -- as a stand-alone program built with -fsanitize=address,undefined and run on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "all-pairs-similarity_amd", "host")


def test_work_lists_cover_the_grid(tmp_path):
    exe = str(tmp_path / "worklist_selftest")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-o", exe, os.path.join(HOST, "worklist_selftest.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "worklist selftest ok" in run.stdout and "c3 symmetric" in run.stdout
