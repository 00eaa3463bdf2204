"""apss_set_components / apss_components_get / _dev / _fetch at the drop-in boundary, without a GPU: declared, listed, exported,
mirrored field for field, NULL and a bad struct_size refused, no pinned struct grown, and every binding and document carries the
feature."""
import ctypes
import os
import re
import subprocess

import pytest

from apss import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "all-pairs-similarity_amd")
NEW = ("apss_set_components", "apss_components_get", "apss_components_dev", "apss_components_fetch")
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
    assert re.search(r"^int32_t apss_set_components\(apss_handle \*h, int32_t on\);", hdr, re.M)
    assert re.search(r"^int32_t apss_components_get\(apss_handle \*h, apss_components_info \*out\);", hdr, re.M)
    assert re.search(r"^int32_t apss_components_dev\(apss_handle \*h, const int32_t \*\*d_label, int64_t \*rows\);", hdr, re.M)
    assert re.search(r"^int32_t apss_components_fetch\(apss_handle \*h, int64_t offset, int64_t count, int32_t \*out_label, "
                     r"int64_t \*out_rep_ext\);", hdr, re.M)
    for name, value in (("RAN", 0), ("OFF", 1), ("OUTSIDE", 2), ("TILE_CUT", 3)):
        assert re.search(r"^#define APSS_CC_%s %d\b" % (name, value), hdr, re.M), name
        assert getattr(_lib, "CC_" + name) == value
    # the section stands behind the global top-K's, and the state rules stand in the header
    assert hdr.index("int32_t apss_top_pairs_get(") < hdr.index("near-duplicate groups: the connected components") < hdr.index("apss_group: the sharded index")
    comment = hdr[hdr.index("near-duplicate groups: the connected components"):hdr.index("#define APSS_CC_RAN")]
    for text in ("launches nothing new, reads nothing new and allocates nothing", "label[slot] is the smallest slot of the slot's component",
                 "A row marked removed has label -1", "Either output pointer may be NULL",
                 "valid until the next insert, query-type call, remove,", "Every stored slot becomes a singleton",
                 "complete = 1 only on an empty store", "survives apss_clear, which empties the structure and sets complete = 1",
                 "frees the stage's buffers", "then answer APSS_E_STATE", "on = 0, declined = APSS_CC_OFF",
                 "behind k_rm_drop and before the per-query cut", "whatever apss_set_top_k and apss_set_top_pairs keep",
                 "every window's list is absorbed before that window's cut", "untouched, element by element",
                 "slot_first + row when the batch is stored rows", "The selected slots for apss_query_stored[_dev]",
                 "declined with APSS_CC_OUTSIDE and changes nothing", "not admitted have no slot",
                 "apss_self_join resets to singletons, absorbs, and leaves complete = 1",
                 "sets new slots to singletons, absorbs, and keeps complete as it was", "Its pairs are true edges",
                 "set new slots to singletons and set complete = 0", "A call declined with APSS_CC_TILE_CUT", "sets complete = 0 if it stored rows",
                 "resets to singletons with complete = 0 on a non-empty store if it is an apss_self_join",
                 "that marks at least one row, and every compaction that discards rows (auto-compaction included)",
                 "complete = 0 unless the store is empty, resets + 1", "never wrong about an edge", "a range outside [0, rows]",
                 "APSS_E_UNSUPPORTED (\"term shard\")", "leaves the structure reset", "apss_group has no such call",
                 "gains no synchronisation", "ONE synchronisation", "A second read without a change launches nothing",
                 "at most 12 B per stored slot", "apss_stats.hbm_bytes"):
        assert text in comment, text


def test_struct_is_mirrored_field_for_field(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "apss.h")).read()
    body = re.search(r"typedef struct apss_components_info \{(.*?)\} apss_components_info;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for t, names in re.findall(r"\b(int64_t|int32_t|double)\s+([a-z_0-9, ]+);", body):
        fields += [(n.strip(), C_TYPES[t]) for n in names.split(",")]
    assert fields == list(_lib.ComponentsInfo._fields_)
    assert [n for n, _ in fields] == ["struct_size", "on", "complete", "declined", "rows", "rows_live", "components", "singletons",
                                      "largest", "pairs_absorbed", "unions_total", "resets", "hook_ms", "label_ms", "hook_launches",
                                      "label_launches", "reserved"]
    # its size, and the pinned structs', compiled from the header: nothing else grew
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "apss.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(apss_components_info), sizeof(apss_config), sizeof(apss_stats), sizeof(apss_group_stats), "
                   "sizeof(apss_top_pairs_info), offsetof(apss_components_info, label_launches)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split()
    assert out == ["112", "64", "288", "424", "72", "100"], out
    assert ctypes.sizeof(_lib.ComponentsInfo) == 112 and _lib.ComponentsInfo.label_launches.offset == 100
    assert (ctypes.sizeof(_lib.Config), ctypes.sizeof(_lib.Stats), ctypes.sizeof(_lib.GroupStats)) == (64, 288, 424)


def test_null_and_bad_struct_size_are_refused(so):
    L = _lib.lib()
    info = _lib.ComponentsInfo()
    info.struct_size = ctypes.sizeof(info)
    rows, p = ctypes.c_int64(0), ctypes.c_void_p()
    assert L.apss_set_components(None, 1) == _lib.E_INVALID
    assert L.apss_set_components(None, 0) == _lib.E_INVALID
    assert L.apss_components_get(None, ctypes.byref(info)) == _lib.E_INVALID
    assert L.apss_components_dev(None, ctypes.byref(p), ctypes.byref(rows)) == _lib.E_INVALID
    assert L.apss_components_fetch(None, 0, 0, None, None) == _lib.E_INVALID
    # (a bad struct_size needs a handle, and a handle needs a device: tests/test_gpu_components.py covers the rest; here the check
    # stands in the source, in front of everything that touches the device)
    src = open(os.path.join(PKG, "csrc", "apss_hip.hip")).read()
    get = src[src.index("int32_t apss_components_get("):src.index("int32_t apss_components_dev(")]
    assert get.index("apss_components_info.struct_size must be set") < get.index("enter(h)")


def test_every_binding_carries_the_feature():
    engine = open(os.path.join(PKG, "apss", "engine.py")).read()
    for text in ("components=False", "def set_components(self, on)", "def components(self", "def components_dev(self)",
                 "def components_info(self)", "apss_set_components", "apss_components_get", "apss_components_dev", "apss_components_fetch"):
        assert text in engine, text
    hpp = open(os.path.join(PKG, "host", "cpslab_host.hpp")).read()
    cpp = open(os.path.join(PKG, "host", "cpslab_host.cpp")).read()
    assert re.search(r"\bbool components = false;", hpp) and "cpslab.allpair.gpu.components" in hpp
    assert re.search(r"std::unordered_map<std::string, std::string> groups\(\);", hpp)
    assert "apss_set_components(h_, 1)" in cpp and "cpslab.allpair.gpu.components ignored" in cpp and "apss_components_fetch(h_" in cpp
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert re.search(r"^host_components_selftest:", mk, re.M) and re.search(r"^all:.*\bhost_components_selftest\b", mk, re.M)
    assert re.search(r"^clean:\n\trm -f .*\bhost_components_selftest\b", mk, re.M)
    assert re.search(r"^components_selftest:", mk, re.M) and not re.search(r"^all:.*(?<!host_)components_selftest\b", mk, re.M)
    assert "groups()" in open(os.path.join(PKG, "host", "host_components_selftest.cpp")).read()
    jni = open(os.path.join(PKG, "jvm", "apss_jni.c")).read()
    assert "apss_set_components((apss_handle *)t, " in jni and "apss_components_fetch((apss_handle *)t, " in jni
    scala = open(os.path.join(PKG, "jvm", "NativeApss.scala")).read()
    assert re.search(r"def setComponents\(h: Long, on: Boolean\): Int", scala)
    assert re.search(r"def components\(h: Long\): \(Array\[Int\], Array\[Long\]\)", scala)
    actor = open(os.path.join(PKG, "jvm", "GpuIndexingWorkerActor.scala")).read()
    assert "cpslab.allpair.gpu.components" in actor and "NativeApss.setComponents(handle, true)" in actor
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    hdrs = re.search(r"^HDRS\s*=(.*)$", mk, re.M).group(1).split()
    assert "apss_components.hpp" in hdrs and "apss_components_core.hpp" in hdrs
    # no new site that makes an event: the stage's four come out of begin_timed / end_timed_read (apss_stage.hpp)
    made = {f: open(os.path.join(PKG, "csrc", f)).read().count("hipEventCreate") for f in os.listdir(os.path.join(PKG, "csrc"))
            if f.endswith((".hip", ".hpp"))}
    # (every event is an owner that makes itself where it is first recorded: the timed and the untimed call of the HIP back-end,
    # the only file that may make or destroy one -- tests/test_owned_host.py holds the frees to the same file; there were seven sites)
    assert {f: n for f, n in made.items() if n} == {"apss_stage.hpp": 2}
    assert sum(made.values()) <= 7
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "apss_set_components" in text, doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 5i" in design and "k_cc_hook" in design and "cc_grid" in design
    nine = design[design.index("## 9"):]
    for text in ("apss_set_components", "grid", "across a removal", "term shard"):
        assert text in nine, text
    assert os.path.exists(os.path.join(ROOT, "profiles", "components.md")) and os.path.exists(os.path.join(ROOT, "profiles", "components.py"))
