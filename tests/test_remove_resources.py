"""The removal kernels (csrc/apss_remove.hpp) keep the registers, LDS and occupancy DESIGN.md 5f states for them, with no scratch.
Same compile step as tests/test_topk_window_resources.py (hipcc cross-compiles for gfx950 without a GPU)."""
import os
import re

import resource_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel -> (VGPRs at most, LDS bytes per workgroup at most, waves per SIMD at least): DESIGN.md 5f, the plan's column
STATED = {
    "k_rm_mark": (32, 16, 8),     # two ids, a binary search's bounds in 64 bits; one word of LDS per wave
    "k_rm_drop": (48, 0, 8),      # four pairs (12 values), four 64-bit ballots, the places
    "k_rm_rows": (16, 0, 8),      # a flag and a difference per row
    "k_rm_gather": (24, 0, 8),    # one wave per row, two streams copied
}


def test_removal_kernels_meet_their_stated_resources():
    res = resource_report.report()
    found = set()
    for name, r in res.items():
        if "k_rm_" not in name:
            continue
        print(name, r)
        assert r["ScratchSize"] == 0, (name, r)
        for kernel, (vgprs, lds, occ) in STATED.items():
            if kernel in name:
                assert r["VGPRs"] <= vgprs and r["LDS"] <= lds and r["Occupancy"] >= occ, (name, r)
                found.add(kernel)
    assert found == set(STATED), found
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 5f"):]
    for kernel, (vgprs, lds, occ) in STATED.items():
        row = re.search(r"^\| `%s` \| (\d+) \| (\d+) \| (\d+) \|" % kernel, section, re.M)
        assert row and (int(row.group(1)), int(row.group(2)), int(row.group(3))) == (vgprs, lds, occ), kernel
