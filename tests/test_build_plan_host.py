"""host/build_plan_selftest.cpp: the index build's plan (csrc/apss_build_plan.hpp) against a table of literal decisions taken
from the code the plan replaced -- a row on each side of every threshold, every hook, the measured shapes -- and its trace
lines, as a stand-alone program built with -fsanitize=address,undefined and run on the CPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "all-pairs-similarity_amd", "host")


def test_build_plan_matches_the_table(tmp_path):
    exe = str(tmp_path / "build_plan_selftest")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-o", exe, os.path.join(HOST, "build_plan_selftest.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    assert "warning" not in build.stderr, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "build plan selftest ok: 75 rows, 5 traces" in run.stdout
