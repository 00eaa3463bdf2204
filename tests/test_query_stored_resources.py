"""The kernels of the stored-row query (csrc/apss_query_stored.hpp) keep the registers, LDS and occupancy DESIGN.md 5g states for
them, with no scratch.  Same compile step as tests/test_remove_resources.py (hipcc cross-compiles for gfx950 without a GPU)."""
import os
import re

import resource_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kernel -> (VGPRs at most, LDS bytes per workgroup at most, waves per SIMD at least): DESIGN.md 5g, the plan's column
STATED = {
    "k_qs_select": (32, 0, 8),    # two ids, two binary searches' bounds in 64 bits, two flags and two counts
    "k_qs_ids": (16, 32, 8),      # two counters; one word of LDS per wave and counter
    "k_qs_slots": (8, 0, 8),      # a flag and a rank per slot
    "k_qs_gather": (24, 16, 8),   # one wave per selected row, two streams copied; the four summary words in LDS
}


def test_stored_query_kernels_meet_their_stated_resources():
    res = resource_report.report()
    found = set()
    for name, r in res.items():
        if "k_qs_" not in name:
            continue
        print(name, r)
        assert r["ScratchSize"] == 0, (name, r)
        assert r["Occupancy"] >= 8, (name, r)
        for kernel, (vgprs, lds, occ) in STATED.items():
            if kernel in name:
                assert r["VGPRs"] <= vgprs and r["LDS"] <= lds and r["Occupancy"] >= occ, (name, r)
                found.add(kernel)
    assert found == set(STATED), found
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 5g"):]
    for kernel, (vgprs, lds, occ) in STATED.items():
        row = re.search(r"^\| `%s` \| (\d+) \| (\d+) \| (\d+) \|" % kernel, section, re.M)
        assert row and (int(row.group(1)), int(row.group(2)), int(row.group(3))) == (vgprs, lds, occ), kernel
