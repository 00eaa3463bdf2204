"""The one-pass ingest kernel of plain batches (k_ingest_plain, apss_kernels.hpp) without a GPU: the library builds for gfx950
with it, and the kernel keeps everything in registers -- no scratch, full occupancy (it is a memory-bound copy: what it needs is
waves in flight).  hipcc cross-compiles for gfx950 without a GPU; only the ingest kernels are compiled here (the whole library
takes minutes: test_kernel_resources.py does that)."""
import os

import resource_report


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
    res = resource_report.compile_report(str(src), "-I", resource_report.CSRC)
    mine = list(resource_report.instantiations("k_ingest_plain", res).values())
    assert len(mine) == 1, sorted(res)
    r = mine[0]
    assert r["ScratchSize"] == 0 and r["VGPRs"] <= 64 and r["Occupancy"] >= 8, r
