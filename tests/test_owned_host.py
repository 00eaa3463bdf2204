"""host/owned_selftest.cpp: the owning types every device array, event, pinned block and stream of the library lives in
(csrc/apss_owned.hpp), over a counting fake of the back-end, as a stand-alone program on the CPU under
-fsanitize=address,undefined: the capacities of the handle's, the group's and the stages' growth policies against literal
tables, `keep`, the order of allocate / copy / wait / free, the ledger after every step, a failure injected at every back-end call
(nothing leaked: the fake's live count and LeakSanitizer), moves, the other owners, a stage's struct assigned from an empty one.
The header must compile without a HIP include path: the build line names none."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "all-pairs-similarity_amd")
HOST = os.path.join(PKG, "host")
CSRC = os.path.join(PKG, "csrc")
HIP_OWNERSHIP_CALLS = ("hipMalloc", "hipFree", "hipHostMalloc", "hipHostFree", "hipEventCreate", "hipEventDestroy", "hipStreamCreate",
                       "hipStreamDestroy")


def test_owning_types_over_a_counting_back_end(tmp_path):
    exe = str(tmp_path / "owned_selftest")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            "-o", exe, os.path.join(HOST, "owned_selftest.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    assert "warning" not in build.stderr, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "runtime error" not in run.stderr and "LeakSanitizer" not in run.stderr, run.stderr[-3000:]
    assert "owned selftest ok" in run.stdout


def test_the_core_header_knows_no_hip():
    text = open(os.path.join(CSRC, "apss_owned.hpp")).read()
    assert not re.search(r"#include\s*<hip/", text) and not re.search(r"\bhip[A-Z]\w*\(", text)
    mk = open(os.path.join(HOST, "Makefile")).read()
    assert re.search(r"^owned_selftest:", mk, re.M) and not re.search(r"^all:.*\bowned_selftest\b", mk, re.M)
    assert re.search(r"^clean:\n\trm -f .*\bowned_selftest\b", mk, re.M)


def test_only_the_hip_back_end_reserves_and_frees():
    """device memory, pinned memory, events and streams are made and destroyed in ONE file of csrc/ (HipBackend, apss_stage.hpp):
    everything else holds them in owners, and no destroy function carries a list"""
    found = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".hpp")):
            text = open(os.path.join(CSRC, f)).read()
            n = sum(len(re.findall(r"\b%s" % name, text)) for name in HIP_OWNERSHIP_CALLS)
            if n:
                found[f] = n
    assert list(found) == ["apss_stage.hpp"], found
    for f in ("apss_hip.hip", "apss_group.hip", "apss_stage.hpp", "apss_topk.hpp", "apss_top_pairs.hpp", "apss_components.hpp"):
        assert "release(" not in open(os.path.join(CSRC, f)).read(), f
    src = open(os.path.join(CSRC, "apss_hip.hip")).read()
    destroy = src[src.index("void apss_destroy("):src.index("const char *apss_last_error(")]
    assert len(destroy.strip().splitlines()) <= 7 and "delete h;" in destroy, destroy
    grp = open(os.path.join(CSRC, "apss_group.hip")).read()
    destroy = grp[grp.index("void apss_group_destroy("):grp.index("const char *apss_group_last_error(")]
    assert "DevBuf" not in destroy and ".reset()" not in destroy and destroy.count(" = {};") == 5, destroy
