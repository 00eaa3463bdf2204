"""k_probe_planes (csrc/apss_even.hpp: the plain 512-thread thin-round filter with two planes of 8-bit sums) is held to the
bounds of the k_probe_even family (test_kernel_resources.py, test_persist_resources.py): no scratch, at most 128 VGPRs, 4 waves
per SIMD, and its static LDS twice in the CU's 160 KB -- for every window a plain 512-thread handle takes (2 .. 6 steps).  hipcc
cross-compiles for gfx950 without a GPU."""
import resource_report


def test_two_plane_kernels_keep_two_workgroups_per_cu():
    planes = resource_report.instantiations("k_probe_planes")
    assert set(planes) == {"_ZN4apss14k_probe_planesILi%dEEEvNS_9ProbeArgsE" % u for u in (2, 3, 4, 5, 6)}, sorted(planes)
    for name, r in sorted(planes.items()):
        print(name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs"] <= 128 and r["Occupancy"] == 4, (name, r)
        assert 2 * r["LDS"] <= 160 * 1024, (name, r)
