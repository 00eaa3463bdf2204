"""k_probe_planes (csrc/apss_even.hpp: the plain 512-thread thin-round filter with two planes of 8-bit sums) is held to the
bounds of the k_probe_even family (test_kernel_resources.py, test_persist_resources.py): no scratch, at most 128 VGPRs, 4 waves
per SIMD, and its static LDS twice in the CU's 160 KB -- for every window a plain 512-thread handle takes (2 .. 6 steps).  hipcc
cross-compiles for gfx950 without a GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "all-pairs-similarity_amd", "csrc")


def test_two_plane_kernels_keep_two_workgroups_per_cu(tmp_path):
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
    planes = {k: v for k, v in res.items() if "k_probe_planes" in k}
    assert set(planes) == {"_ZN4apss14k_probe_planesILi%dEEEvNS_9ProbeArgsE" % u for u in (2, 3, 4, 5, 6)}, sorted(planes)
    for name, r in sorted(planes.items()):
        print(name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs"] <= 128 and r["Occupancy"] == 4, (name, r)
        assert 2 * r["LDS"] <= 160 * 1024, (name, r)
