"""The cut instantiations of k_probe (csrc/apss_kernels.hpp, apss_set_top_k_tile_cut) keep to the budget DESIGN.md 5e states for
them -- no scratch, at most 128 VGPRs, four waves per SIMD -- and the instantiations without the cut still compile to the
registers they had before the cut existed.  Same compile step as tests/test_topk_resources.py."""
import os
import re

import resource_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# k_probe<2, BLOCK, FX> without the cut: VGPRs of the commit before the cut was added ("Cut inside the probe")
BEFORE = {(512, True): 113, (1024, True): 113, (512, False): 110, (1024, False): 109}


def test_cut_instantiations_meet_their_stated_resources():
    res = resource_report.report()
    cut, plain = {}, {}
    for name, r in res.items():
        m = re.fullmatch(r"_ZN4apss7k_probeILi2ELi(\d+)ELb([01])ELb([01])EEEvNS_9ProbeArgsE", name)
        if m:
            (cut if m.group(3) == "1" else plain)[(int(m.group(1)), m.group(2) == "1")] = r
    assert set(cut) == set(plain) == set(BEFORE), (sorted(cut), sorted(plain))
    for inst, r in cut.items():
        print("k_probe<2, %d, %s, true>: %s" % (inst[0], inst[1], r))
        assert r["ScratchSize"] == 0 and r["VGPRs"] <= 128 and r["Occupancy"] >= 4, (inst, r)
    for inst, r in plain.items():
        assert r["ScratchSize"] == 0 and r["VGPRs"] == BEFORE[inst], (inst, r)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "| `k_probe<2, 512 \\| 1024, FX, true>` |" in design  # the row of the kernel table
