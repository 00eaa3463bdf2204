"""The compiler's resource report of the device code, shared by the resource tests: hipcc cross-compiles for gfx950 without a GPU
and says, per kernel instantiation, what registers, scratch, LDS and occupancy it ended up with.  The whole translation unit is
compiled once per process."""
import functools
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "all-pairs-similarity_amd", "csrc")
FIELDS = {"TotalSGPRs": "SGPRs", "VGPRs": "VGPRs", "AGPRs": "AGPRs", "ScratchSize [bytes/lane]": "ScratchSize",
          "Occupancy [waves/SIMD]": "Occupancy", "LDS Size [bytes/block]": "LDS"}


def compile_report(source, *flags):
    """{mangled name: {SGPRs, VGPRs, AGPRs, ScratchSize, Occupancy, LDS}} of every kernel `source` compiles to"""
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", *flags,
                              "-Rpass-analysis=kernel-resource-usage", "-o", os.path.join(tmp, "k.s"), source],
                             capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    cur, res = None, {}
    for line in out.stderr.splitlines():
        m = re.search(r"remark:\s+([^:]+): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = res.setdefault(m.group(2), {})
        elif m.group(1) in FIELDS and cur is not None:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    return res


@functools.lru_cache(maxsize=None)
def report():
    """the report of csrc/apss_hip.hip, every kernel of the handle (about two minutes, once)"""
    return compile_report(os.path.join(CSRC, "apss_hip.hip"))


def instantiations(kernel, res=None):
    """{mangled name: figures} of the instantiations of the kernel whose own name is `kernel` (the mangled name holds it with
    its length in front: k_probe_even does not find k_probe_even_merged)"""
    res = report() if res is None else res
    return {name: r for name, r in res.items() if re.search(r"(?<!\d)%d%s(?![a-z_0-9])" % (len(kernel), kernel), name)}
