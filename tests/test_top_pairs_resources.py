"""The kernels of the global top-K (csrc/apss_top_pairs.hpp) keep the registers, LDS and occupancy DESIGN.md 5h states for them,
with no scratch.  Same compile step as tests/test_query_stored_resources.py (hipcc cross-compiles for gfx950 without a GPU); the
rows are read from the document."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "all-pairs-similarity_amd", "csrc")
KERNELS = ("k_tp_hist", "k_tp_pick", "k_tp_collect", "k_tp_tie_hist", "k_tp_tie_collect", "k_tp_keys", "k_tp_write")


def stated_rows():
    """kernel -> (VGPRs at most, LDS bytes per workgroup at most, waves per SIMD at least), from DESIGN.md 5h's table"""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("### 5h"):]
    section = section[:section.index("\n## ")] if "\n## " in section else section
    rows = {}
    for kernel, vgprs, lds, occ in re.findall(r"^\| `(k_tp_\w+)` \| (\d+) \| (\d+) \| (\d+) \|", section, re.M):
        rows[kernel] = (int(vgprs), int(lds), int(occ))
    return rows


def test_top_pairs_kernels_meet_their_stated_resources(tmp_path):
    stated = stated_rows()
    assert set(stated) == set(KERNELS), stated
    out = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "k.s"),
                          os.path.join(CSRC, "apss_hip.hip")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    cur, res = None, {}
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
        for key in ("VGPRs", "ScratchSize \\[bytes/lane\\]", "Occupancy \\[waves/SIMD\\]", "LDS Size \\[bytes/block\\]"):
            m = re.search(r"\s%s: (\d+)" % key, line)
            if m and cur:
                res[cur][key.split(" ")[0]] = int(m.group(1))
    found = set()
    for name, r in res.items():
        m = re.search(r"\d+(k_tp_[a-z_]+?)E", name)  # the mangled name holds the kernel's own, length first
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
