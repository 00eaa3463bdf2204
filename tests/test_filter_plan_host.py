"""host/filter_plan_selftest.cpp: the filter plan (csrc/apss_filter_plan.hpp: kernel instantiation, window, staging waves, rows
per round, accumulator scales, coarse tile rows) against tables of literal decisions taken from the code the header replaced --
a row on each side of every threshold, every hook, the quoted shapes, the diag lines -- and a swept grid of facts whose unlisted
plans and whose every decision are pinned and which, with the table, reaches every listed variant; as a stand-alone program
built with -fsanitize=address,undefined and run on the CPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "all-pairs-similarity_amd", "host")
CSRC = os.path.join(ROOT, "all-pairs-similarity_amd", "csrc")


def test_filter_plan_matches_the_table_and_the_sweep(tmp_path):
    exe = str(tmp_path / "filter_plan_selftest")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-o", exe, os.path.join(HOST, "filter_plan_selftest.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    assert "warning" not in build.stderr, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert ("filter plan selftest ok: 112 plan rows, 9 diag rows, 47 scale rows, 24 tile rows, 20 merge rows, 309408 grid points, "
            "76 variants reached") in run.stdout
    assert len(re.findall(r"^not listed: ", run.stdout, re.M)) == 7


def test_the_header_is_plain_cpp_and_the_selftest_is_in_the_makefile():
    text = open(os.path.join(CSRC, "apss_filter_plan.hpp")).read()
    assert not re.search(r"#include\s*<hip/", text) and not re.search(r"\bhip[A-Z]\w*\(", text) and "__global__" not in text
    mk = open(os.path.join(HOST, "Makefile")).read()
    assert re.search(r"^filter_plan_selftest:", mk, re.M) and not re.search(r"^all:.*\bfilter_plan_selftest\b", mk, re.M)
    assert re.search(r"^clean:\n\trm -f .*\bfilter_plan_selftest\b", mk, re.M)
    # the rule's arithmetic is in the header alone: the threshold formula is written once, nowhere in the handle's translation unit
    src = open(os.path.join(CSRC, "apss_hip.hip")).read()
    assert text.count("1.0 / 2048") == 1 and "1.0 / 2048" not in src
