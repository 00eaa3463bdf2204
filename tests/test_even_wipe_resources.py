"""k_probe_planes<5> and <6> (csrc/apss_even.hpp, WIPE: planes 32,768 bytes apart, the idle one zeroed whole by
ds_write_addtid_b32 stores from inline assembly) keep the bounds of the k_probe_even family: no scratch, at most 128 VGPRs,
4 waves per SIMD -- the wipe holds a zero in one vector register and its addresses in scalar ones, in a kernel that is at its
scalar limit as it is.  hipcc cross-compiles for gfx950 without a GPU."""
import resource_report


def test_the_wiping_kernels_keep_their_registers_and_occupancy():
    planes = resource_report.instantiations("k_probe_planes")
    for u in (5, 6):
        name = "_ZN4apss14k_probe_planesILi%dEEEvNS_9ProbeArgsE" % u
        assert name in planes, sorted(planes)
        r = planes[name]
        print(name, r)
        assert r["ScratchSize"] == 0 and r["VGPRs"] <= 128 and r["Occupancy"] == 4, (name, r)
