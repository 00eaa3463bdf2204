"""The per-query top-k kernels (csrc/apss_topk.hpp) keep the registers, LDS and occupancy DESIGN.md 5e states for them, with
no scratch.  Same compile step as tests/test_kernel_resources.py (hipcc cross-compiles for gfx950 without a GPU)."""
import os

import resource_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel -> (VGPRs at most, LDS bytes per workgroup at most, waves per SIMD at least): DESIGN.md 5e
STATED = {
    "k_topk_count": (32, 16 * 1024, 8),         # 2048-slot hash table: keys + counts
    "k_topk_scan": (32, 16 * 1024 + 64, 8),     # two 1024 x u64 scan arrays
    "k_topk_scatter": (32, 24 * 1024, 6),       # keys + counts + bases: six 256-thread workgroups per CU
    "k_topk_select": (64, 18 * 1024, 8),        # 1024 x 128-bit keys + histogram
}


def test_topk_kernels_meet_their_stated_resources():
    res = resource_report.report()
    found = set()
    for name, r in res.items():
        if "k_topk_" not in name:
            continue
        assert r["ScratchSize"] == 0, (name, r)
        for kernel, (vgprs, lds, occ) in STATED.items():
            if kernel in name:
                assert r["VGPRs"] <= vgprs and r["LDS"] <= lds and r["Occupancy"] >= occ, (name, r)
                found.add(kernel)
    assert found == set(STATED), found
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for kernel in STATED:
        assert kernel in design, kernel
