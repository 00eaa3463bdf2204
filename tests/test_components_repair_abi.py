"""apss_set_components_repair / apss_components_repair_get at the drop-in boundary, without a GPU: declared, listed, exported,
mirrored field for field with the size stated, the constants mirrored, NULL and a bad struct_size refused, and every binding and
document carries the feature."""
import ctypes
import os
import re
import subprocess

import pytest

from apss import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "all-pairs-similarity_amd")
NEW = ("apss_set_components_repair", "apss_components_repair_get")
C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}


@pytest.fixture(scope="module")
def so():
    return _lib.build()


def test_symbols_declared_listed_and_exported(so):
    hdr = open(os.path.join(ROOT, "include", "apss.h")).read()
    L = ctypes.CDLL(so)
    for sym in NEW:
        assert sym in _lib.SYMBOLS
        assert getattr(L, sym) is not None
    assert re.search(r"^int32_t apss_set_components_repair\(apss_handle \*h, int64_t max_rows\);", hdr, re.M)
    assert re.search(r"^int32_t apss_components_repair_get\(apss_handle \*h, apss_components_repair_info \*out\);", hdr, re.M)
    for name, value in (("RAN", 0), ("OFF", 1), ("NO_COMPONENTS", 2), ("BUDGET", 3), ("NOTHING", 4)):
        assert re.search(r"^#define APSS_CCR_%s %d\b" % (name, value), hdr, re.M), name
        assert getattr(_lib, "CCR_" + name) == value
    # the section stands behind apss_components_fetch and in front of the group's banner, and says what changes with the repair on
    assert hdr.index("int32_t apss_components_fetch(") < hdr.index("across a removal and a compaction: the repair") < hdr.index("apss_group: the sharded index")
    comment = hdr[hdr.index("across a removal and a compaction: the repair"):hdr.index("#define APSS_CCR_RAN")]
    for text in ("with the setting off every call\n * launches, reads and allocates exactly what it does without this section", "0 is off",
                 "the most live rows one apss_remove[_dev]", "survives apss_clear", "no effect while apss_set_components is off",
                 "What changes with the repair on", "every marked slot flags its root", "one wait", "The last call's results stay fetchable",
                 "as the batch apss_query_stored of them would be", "behind k_rm_drop into the forest", "complete and resets stay as they were",
                 "APSS_E_STATE, as after an insert", "declined = APSS_CCR_BUDGET, budget_resets + 1", "never costs more than the caller allowed",
                 "The marks stay: the removal\n *      happened", "a marked row is always a singleton once apss_remove returns",
                 "a fresh apss_self_join over the live rows", "never wrong about an edge", "renumber the forest", "remaps + 1",
                 "max_rows < 0 or > 2^31 - 1", "APSS_E_UNSUPPORTED (\"term shard\")", "apss_group has no such call"):
        assert text in comment, text


def test_struct_is_mirrored_field_for_field(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "apss.h")).read()
    body = re.search(r"typedef struct apss_components_repair_info \{(.*?)\} apss_components_repair_info; +/\* (\d+) bytes \*/", hdr, re.S)
    stated = int(body.group(2))
    body = re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S)
    fields = []
    for t, names in re.findall(r"\b(int64_t|int32_t|double)\s+([a-z_0-9, ]+);", body):
        fields += [(n.strip(), C_TYPES[t]) for n in names.split(",")]
    assert fields == list(_lib.ComponentsRepairInfo._fields_)
    assert [n for n, _ in fields] == ["struct_size", "declined", "max_rows", "rows_marked", "components_touched", "rows_rejoined",
                                      "pairs_rejoined", "repairs", "budget_resets", "remaps", "detach_ms", "rejoin_ms", "remap_ms",
                                      "launches", "reserved0"]
    # its size, and the neighbours', compiled from the header: nothing else grew
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "apss.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(apss_components_repair_info), sizeof(apss_components_info), sizeof(apss_removal_info), sizeof(apss_stats), "
                   "sizeof(apss_config), offsetof(apss_components_repair_info, launches)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split()
    assert out == ["104", "112", str(ctypes.sizeof(_lib.RemovalInfo)), "288", "64", "96"], out
    assert stated == 104 and ctypes.sizeof(_lib.ComponentsRepairInfo) == 104 and _lib.ComponentsRepairInfo.launches.offset == 96


def test_null_and_bad_struct_size_are_refused(so):
    L = _lib.lib()
    info = _lib.ComponentsRepairInfo()
    info.struct_size = ctypes.sizeof(info)
    assert L.apss_set_components_repair(None, 100) == _lib.E_INVALID
    assert L.apss_set_components_repair(None, 0) == _lib.E_INVALID
    assert L.apss_components_repair_get(None, ctypes.byref(info)) == _lib.E_INVALID
    # (a bad struct_size and a bad max_rows need a handle, and a handle needs a device: tests/test_gpu_components_repair.py covers
    # them; here the checks stand in the source, in front of everything that changes the handle)
    src = open(os.path.join(PKG, "csrc", "apss_hip.hip")).read()
    get = src[src.index("int32_t apss_components_repair_get("):]
    get = get[:get.index("\n}\n")]
    assert get.index("apss_components_repair_info.struct_size must be set") < get.index("std::memcpy(out")
    put = src[src.index("int32_t apss_set_components_repair("):]
    put = put[:put.index("\n}\n")]
    assert put.index("max_rows < 0 || max_rows > 0x7fffffffLL") < put.index("h->ccr_max = max_rows")
    assert put.index("term shard") < put.index("h->ccr_max = max_rows")


def test_every_binding_carries_the_feature():
    engine = open(os.path.join(PKG, "apss", "engine.py")).read()
    for text in ("components_repair=0", "def set_components_repair(self, max_rows)", "def components_repair_info(self)",
                 "apss_set_components_repair", "apss_components_repair_get"):
        assert text in engine, text
    hpp = open(os.path.join(PKG, "host", "cpslab_host.hpp")).read()
    cpp = open(os.path.join(PKG, "host", "cpslab_host.cpp")).read()
    assert re.search(r"\blong componentsRepairRows = 0;", hpp) and "cpslab.allpair.gpu.componentsRepairRows" in hpp
    assert "apss_set_components_repair(h_, conf.componentsRepairRows)" in cpp and "cpslab.allpair.gpu.componentsRepairRows ignored" in cpp
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert re.search(r"^components_repair_selftest:", mk, re.M) and not re.search(r"^all:.*components_repair_selftest\b", mk, re.M)
    assert re.search(r"^clean:\n\trm -f .*\bcomponents_repair_selftest\b", mk, re.M)
    jni = open(os.path.join(PKG, "jvm", "apss_jni.c")).read()
    assert "apss_set_components_repair((apss_handle *)t, " in jni
    scala = open(os.path.join(PKG, "jvm", "NativeApss.scala")).read()
    assert re.search(r"def setComponentsRepair\(h: Long, maxRows: Long\): Int", scala)
    actor = open(os.path.join(PKG, "jvm", "GpuIndexingWorkerActor.scala")).read()
    assert "cpslab.allpair.gpu.componentsRepairRows" in actor and "NativeApss.setComponentsRepair(handle, componentsRepairRows)" in actor
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    hdrs = re.search(r"^HDRS\s*=(.*)$", mk, re.M).group(1).split()
    assert "apss_components_repair.hpp" in hdrs and "apss_components_repair_core.hpp" in hdrs
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "apss_set_components_repair" in text, doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 5j" in design and design.index("### 5i") < design.index("### 5j")
    for text in ("k_cr_touch", "k_cr_detach", "k_cr_remap", "Invariant", "Completeness", "Twins"):
        assert text in design[design.index("### 5j"):], text
    nine = design[design.index("## 9"):]
    for text in ("across a removal", "term shard", "budget"):
        assert text in nine, text
