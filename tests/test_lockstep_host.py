"""host/lockstep_selftest.cpp: the lock-step rule of the group's member threads (csrc/apss_lockstep.hpp) -- a member publishes its
failure before the next barrier, every thread acts on the flag as that barrier returned it -- as a stand-alone program on the CPU
with real threads, once under -fsanitize=address,undefined and once under -fsanitize=thread: a failure injected at every
(thread, step) of a 6-step script on 1, 2, 3 and 8 threads, two failures in one step, the steps that are skipped once the call
has failed, one barrier over 12,000 generations while the flag changes behind the threads' backs, two groups of threads on one
flag, run_members' join, and the exchange's offsets and key width against literal tables.  Beside it, text checks: the header
knows no HIP, and apss_group.hip waits at a barrier and raises the flag nowhere but through that header."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "all-pairs-similarity_amd")
HOST = os.path.join(PKG, "host")
CSRC = os.path.join(PKG, "csrc")
SANITIZE = {"address": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "thread": ["-fsanitize=thread"]}


@pytest.mark.parametrize("mode", ["address", "thread"])
def test_the_rule_with_real_threads(tmp_path, mode):
    exe = str(tmp_path / ("lockstep_selftest_" + mode))
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *SANITIZE[mode], "-o", exe, os.path.join(HOST, "lockstep_selftest.cpp"),
                            "-lpthread"], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    assert "warning" not in build.stderr, build.stderr[-3000:]
    run = subprocess.run(["timeout", "-k", "10", "240", exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    for report in ("WARNING: ThreadSanitizer", "runtime error", "AddressSanitizer", "LeakSanitizer"):
        assert report not in run.stderr, run.stderr[-3000:]
    assert run.stdout.strip().splitlines()[-1] == "lockstep selftest ok"


def test_the_header_knows_no_hip():
    text = open(os.path.join(CSRC, "apss_lockstep.hpp")).read()
    assert not re.search(r"#include\s*[<\"]hip", text) and not re.search(r"\bhip[A-Z]\w*\(", text)
    assert not re.search(r'#include\s*"', text)  # (nothing of the project either: it stands alone)
    selftest = open(os.path.join(HOST, "lockstep_selftest.cpp")).read()
    assert re.findall(r'#include\s*"([^"]+)"', selftest) == ["../csrc/apss_lockstep.hpp"]
    mk = open(os.path.join(HOST, "Makefile")).read()
    assert re.search(r"^lockstep_selftest:", mk, re.M) and not re.search(r"^all:.*\blockstep_selftest\b", mk, re.M)
    assert re.search(r"^clean:\n\trm -f .*\blockstep_selftest\b", mk, re.M)


def function_body(src, signature):
    """the text of the function that starts at `signature`, up to the closing brace in column 0"""
    at = src.index(signature)
    return src[at:src.index("\n}\n", at)]


def test_the_group_waits_and_fails_through_the_header_only():
    grp = open(os.path.join(CSRC, "apss_group.hip")).read()
    code = re.sub(r"//[^\n]*", "", grp)
    assert '#include "apss_lockstep.hpp"' in grp
    assert ".wait(" not in code and "failed.store" not in code and "fail_here" not in grp
    assert "class Barrier" not in grp and "std::thread" not in code and "condition_variable" not in code
    assert len(re.findall(r"\bLockstep ls\(", code)) == 2  # member_main and relayout_main
    # the sequencing functions only sequence: no collective, no launch (those are the stages')
    for signature in ("bool member_phase(", "void relayout_main("):
        body = re.sub(r"//[^\n]*", "", function_body(grp, signature))
        assert not re.search(r"\bRccl\b|load_rccl\(|\br->|\bnccl[A-Za-z]+\(", body), signature
        assert "hipLaunchKernelGGL" not in body, signature
        assert len(body.splitlines()) <= 40, (signature, len(body.splitlines()))
    phase = function_body(grp, "bool member_phase(")
    assert len(re.findall(r"\bls\.step\(", phase)) == 6  # B1, B2 without an exchange, B2, B3, B3b, B4
    assert len(re.findall(r"\bls\.step\(", function_body(grp, "void relayout_main("))) == 3  # R1, R2, R3
    # two transports, four free functions, chosen in one place
    for name in ("gather_rccl", "gather_copies", "reduce_rccl", "reduce_copies"):
        assert len(re.findall(r"^int32_t %s\(Phase &P\) \{$" % name, grp, re.M)) == 1, name
    assert len(re.findall(r"= gather_rccl\b", code)) == 1 and len(re.findall(r"= gather_copies\b", code)) == 1
    # the range's final list: one function, reached with and without an exchange
    assert len(re.findall(r"^int32_t range_final_list\(Phase &P\) \{$", grp, re.M)) == 1
    assert len(re.findall(r"\brange_final_list\(P\)", code)) == 2
    assert len(re.findall(r"\bk_threshold_compact\b", code)) == 2  # the kernel and its one launch
    # one thread start and one failure report for the call and the re-layout
    assert len(re.findall(r"\brun_members\(g, ", code)) == 2 and len(re.findall(r"apss::run_members\(", code)) == 1
    assert '"a member failed"' in grp and '"a member failed during the re-layout"' in grp
