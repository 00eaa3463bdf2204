"""The window kernels (csrc/apss_window.hpp) keep the registers, LDS and occupancy DESIGN.md 5e states for them, with no scratch.
Same compile step as tests/test_topk_resources.py (hipcc cross-compiles for gfx950 without a GPU)."""
import os

import resource_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel -> (VGPRs at most, LDS bytes per workgroup at most, waves per SIMD at least): DESIGN.md 5e, "Windows"
STATED = {
    "k_win_df": (32, 16 * 1024, 8),    # the 2048-slot hash table of k_topk_count: keys + counts
    "k_win_bound": (32, 0, 8),         # one wave per row, a 64-bit sum reduced by shuffles
    "k_win_append": (32, 0, 8),        # three streams copied
}


def test_window_kernels_meet_their_stated_resources():
    res = resource_report.report()
    found = set()
    for name, r in res.items():
        if "k_win_" not in name:
            continue
        print(name, r)
        assert r["ScratchSize"] == 0, (name, r)
        for kernel, (vgprs, lds, occ) in STATED.items():
            if kernel in name:
                assert r["VGPRs"] <= vgprs and r["LDS"] <= lds and r["Occupancy"] >= occ, (name, r)
                found.add(kernel)
    assert found == set(STATED), found
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for kernel in STATED:
        assert kernel in design, kernel
