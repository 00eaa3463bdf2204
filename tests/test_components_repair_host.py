"""host/components_repair_selftest.cpp: the per-slot decisions of the components' repair (csrc/apss_components_repair_core.hpp) --
the very touch / detach / renumber the kernels take -- against a textbook recomputation (a union-find of the live-live edges, a
renumbering by rank), as a stand-alone program on the CPU under -fsanitize=address,undefined: random forests, a path, a star,
dead roots and dead leaves among rows marked earlier."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "all-pairs-similarity_amd", "host")


def test_decisions_against_a_textbook_recomputation(tmp_path):
    exe = str(tmp_path / "components_repair_selftest")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                            os.path.join(HOST, "components_repair_selftest.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-3000:]
    assert "components repair selftest ok" in run.stdout
