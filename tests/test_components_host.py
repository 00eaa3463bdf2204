"""host/components_selftest.cpp: the union-find core of the components stage (csrc/apss_components_core.hpp) -- the very find /
link / shorten the kernels run, through the host atomics policy -- against a textbook union-find, as a stand-alone program on the
CPU: once under -fsanitize=address,undefined (sequential edge lists: random, a path forward, reversed and shuffled, a star,
duplicates), once under -fsanitize=thread with 8 threads hooking disjoint slices of one shuffled edge list.  In every run the
roots must be the smallest member of every component."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "all-pairs-similarity_amd", "host")


def build_and_run(tmp_path, name, sanitize, *args):
    exe = str(tmp_path / name)
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *sanitize, "-o", exe, os.path.join(HOST, "components_selftest.cpp"),
                            "-lpthread"], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "WARNING: ThreadSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    return run.stdout


def test_core_against_a_textbook_union_find(tmp_path):
    out = build_and_run(tmp_path, "components_selftest", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert "components selftest ok (sequential)" in out


@pytest.mark.parametrize("mode", ["address", "thread"])
def test_core_with_eight_threads(tmp_path, mode):
    sanitize = ["-fsanitize=thread"] if mode == "thread" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    out = build_and_run(tmp_path, "components_selftest_" + mode, sanitize, "threads")
    assert "components selftest ok (8 threads)" in out
