"""The persistent loop around k_probe_even's body (csrc/apss_even.hpp, probe_even_body) must not cost the kernels their
registers: every k_probe_even / k_probe_even_merged instantiation keeps the occupancy the grid launch's build had -- 4 waves
per SIMD for all 40 of them, read from the resource remarks of the commit before the loop -- uses no scratch, stays within 128
VGPRs, and its static LDS still fits the CU's 160 KB twice (512 threads) or once (1024).  hipcc cross-compiles for gfx950
without a GPU."""
import resource_report

# (threads, window steps, shard rule, 8-bit accumulators) of k_probe_even -- signed weights have no instantiation -- and
# (window steps, 8-bit accumulators) of k_probe_even_merged; waves per SIMD of each in the build before the persistent loop
# (512 threads, 7 steps without the shard rule went with APSS_DEBUG=even_wide, the only way to it: csrc/apss_filter_plan.hpp)
EVEN = ([(512, u, sh, a8) for u in (2, 3, 4, 5, 6, 7) for sh, a8 in ((0, 0), (1, 0), (1, 1)) if (u, sh) != (7, 0)] +
        [(512, u, 0, 1) for u in (2, 3, 4)] + [(1024, u, 0, a8) for u in (3, 5, 6, 7) for a8 in (0, 1)])
MERGED = [(u, a8) for u in (2, 3, 4, 5, 6, 7) for a8 in (0, 1)]
OCCUPANCY_BEFORE = {}
for b, u, sh, a8 in EVEN:
    OCCUPANCY_BEFORE["_ZN4apss12k_probe_evenILi%dELi%dELi%dELb%dELb0ELb%dEEEvNS_9ProbeArgsE" % (b, u, 128 if b == 512 else 256, sh, a8)] = 4
for u, a8 in MERGED:
    OCCUPANCY_BEFORE["_ZN4apss19k_probe_even_mergedILi%dELb%dEEEvNS_9ProbeArgsE" % (u, a8)] = 4


def test_persistent_loop_keeps_registers_and_occupancy():
    assert len(OCCUPANCY_BEFORE) == 40
    res = resource_report.report()
    even = {k: v for k, v in res.items() if "k_probe_even" in k}
    assert set(even) == set(OCCUPANCY_BEFORE), set(even) ^ set(OCCUPANCY_BEFORE)
    for name, r in sorted(even.items()):
        print(name, r)
        assert r["ScratchSize"] == 0, (name, r)
        assert r["Occupancy"] == OCCUPANCY_BEFORE[name], (name, r)
        assert r["VGPRs"] <= 128, (name, r)
        per_cu = 1 if "k_probe_evenILi1024" in name else 2
        assert per_cu * r["LDS"] <= 160 * 1024, (name, r)
