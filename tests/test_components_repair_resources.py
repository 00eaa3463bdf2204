"""The kernels of the components' repair (csrc/apss_components_repair.hpp) keep the registers, LDS and occupancy DESIGN.md 5j
states for them, with no scratch.  Same compile step as tests/test_components_resources.py (hipcc cross-compiles for gfx950 without
a GPU); the rows are read from the document."""
import os
import re

import resource_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_cr_touch", "k_cr_detach", "k_cr_remap")


def stated_rows():
    """kernel -> (VGPRs at most, LDS bytes per workgroup at most, waves per SIMD at least), from DESIGN.md 5j's table"""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 5j"):]
    section = section[:section.index("\n## ")] if "\n## " in section else section
    rows = {}
    for kernel, vgprs, lds, occ in re.findall(r"^\| `(k_cr_\w+)` \| (\d+) \| (\d+) \| (\d+) \|", section, re.M):
        rows[kernel] = (int(vgprs), int(lds), int(occ))
    return rows


def test_repair_kernels_meet_their_stated_resources():
    stated = stated_rows()
    assert set(stated) == set(KERNELS), stated
    res = resource_report.report()
    found = set()
    for name, r in res.items():
        m = re.search(r"\d+(k_cr_[a-z_]+?)E", name)  # the mangled name holds the kernel's own, length first
        if not m:
            continue
        kernel = m.group(1)
        print(kernel, r)
        assert r["ScratchSize"] == 0, (name, r)
        assert r["Occupancy"] >= 8, (name, r)
        vgprs, lds, occ = stated[kernel]
        assert occ >= 8, kernel
        assert r["VGPRs"] <= vgprs and r["LDS"] <= lds and r["Occupancy"] >= occ, (name, r, stated[kernel])
        found.add(kernel)
    assert found == set(KERNELS), found
