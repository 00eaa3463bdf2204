"""The one-pass ingest kernel of plain batches (k_ingest_plain, apss_kernels.hpp) without a GPU: the library builds for gfx950
with it, and the kernel keeps everything in registers -- no scratch, full occupancy (it is a memory-bound copy: what it needs is
waves in flight).  hipcc cross-compiles for gfx950 without a GPU; only the ingest kernels are compiled here (the whole library
takes minutes: test_kernel_resources.py does that)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "all-pairs-similarity_amd", "csrc")


def test_library_builds_with_the_kernel():
    from apss import _lib
    so = _lib.build()
    assert os.path.exists(so)
    with open(so, "rb") as f:
        blob = f.read()
    # the kernel's mangled name: its host-side launch stub and its entry in the gfx950 code object
    assert blob.count(b"_ZN4apss14k_ingest_plainENS_15IngestPlainArgsE") >= 2
    assert b"no_fused_ingest" in blob  # the escape hatch's token


def test_kernel_has_no_scratch(tmp_path):
    src = tmp_path / "k.hip"
    src.write_text('#include "apss_kernels.hpp"\nvoid *keep_ingest_plain = (void *)apss::k_ingest_plain;\n')
    out = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-I", CSRC,
                          "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "k.s"), str(src)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    cur, res = None, {}
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
        for key in ("VGPRs", "ScratchSize \\[bytes/lane\\]", "Occupancy \\[waves/SIMD\\]"):
            m = re.search(r"\s%s: (\d+)" % key, line)
            if m and cur:
                res[cur][key.split(" ")[0]] = int(m.group(1))
    mine = [r for name, r in res.items() if "k_ingest_plain" in name]
    assert len(mine) == 1, sorted(res)
    r = mine[0]
    assert r["ScratchSize"] == 0 and r["VGPRs"] <= 64 and r["Occupancy"] >= 8, r
