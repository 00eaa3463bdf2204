"""apss_query_stored / apss_query_stored_dev / apss_stored_query_get at the drop-in boundary, without a GPU: declared, listed,
exported, mirrored field for field, NULL refused, no pinned struct grown, and every binding and document carries the call."""
import ctypes
import os
import re
import subprocess

import pytest

from apss import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "all-pairs-similarity_amd")
NEW = ("apss_query_stored", "apss_query_stored_dev", "apss_stored_query_get")
C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}


@pytest.fixture(scope="module")
def so():
    return _lib.build()


def test_symbols_declared_listed_and_exported(so):
    hdr = open(os.path.join(ROOT, "include", "apss.h")).read()
    L = ctypes.CDLL(so)
    for sym in NEW:
        assert re.search(r"^int32_t %s\(apss_handle \*h[,)]" % sym, hdr, re.M), sym
        assert sym in _lib.SYMBOLS
        assert getattr(L, sym) is not None
    assert re.search(r"^int32_t apss_query_stored\(apss_handle \*h, int64_t n, const int64_t \*ext_ids, int64_t \*n_rows, int64_t \*n_results\);", hdr, re.M)
    assert re.search(r"^int32_t apss_query_stored_dev\(apss_handle \*h, int64_t n, const int64_t \*d_ext_ids, int64_t \*n_rows, int64_t \*n_results\);", hdr, re.M)
    assert re.search(r"^int32_t apss_stored_query_get\(apss_handle \*h, apss_stored_query_info \*out\);", hdr, re.M)
    # the semantics stand in the header: the batch, the answer, the results, the edge cases, the errors, groups
    comment = hdr[hdr.index("query stored vectors by external id"):hdr.index("typedef struct apss_stored_query_info")]
    for text in ("in stored (slot) order", "marked removed is not selected", "selects both", "selects nothing more",
                 "not applied again", "Self-exclusion is by external id", "k_rm_drop", "APSS_SYM_NOT_WHOLE", "It builds nothing",
                 "auto-compaction does not run", "invalidates the last results on entry", "d_query_ext", "apss_result_count answers 0",
                 "n > 2^31 - 1", "term shard", "apss_group has no such call"):
        assert text in comment, text


def test_struct_is_mirrored_field_for_field(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "apss.h")).read()
    body = re.search(r"typedef struct apss_stored_query_info \{(.*?)\} apss_stored_query_info;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for t, names in re.findall(r"\b(int64_t|int32_t|double)\s+([a-z_0-9, ]+);", body):
        fields += [(n.strip(), C_TYPES[t]) for n in names.split(",")]
    assert fields == list(_lib.StoredQueryInfo._fields_)
    assert [n for n, _ in fields] == ["struct_size", "launches", "ids_given", "ids_distinct", "ids_missing", "rows_selected",
                                      "nnz_selected", "select_ms", "gather_ms"]
    # its size, and the pinned structs', compiled from the header
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "apss.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(apss_stored_query_info), sizeof(apss_config), sizeof(apss_stats), sizeof(apss_group_stats), sizeof(apss_topk_info), "
                   "sizeof(apss_topk_window_info), sizeof(apss_topk_tile_cut_info), sizeof(apss_removal_info)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split()
    assert out == ["64", "64", "288", "424", "56", "80", "32", "88"], out
    assert ctypes.sizeof(_lib.StoredQueryInfo) == 64
    assert (ctypes.sizeof(_lib.Config), ctypes.sizeof(_lib.Stats), ctypes.sizeof(_lib.GroupStats), ctypes.sizeof(_lib.TopkInfo),
            ctypes.sizeof(_lib.TopkWindowInfo), ctypes.sizeof(_lib.TopkTileCutInfo), ctypes.sizeof(_lib.RemovalInfo)) == (64, 288, 424, 56, 80, 32, 88)


def test_null_is_refused(so):
    L = _lib.lib()
    info = _lib.StoredQueryInfo()
    info.struct_size = ctypes.sizeof(info)
    rows, n = ctypes.c_int64(0), ctypes.c_int64(0)
    ids = (ctypes.c_int64 * 1)(3)
    assert L.apss_query_stored(None, 1, ctypes.cast(ids, ctypes.c_void_p), ctypes.byref(rows), ctypes.byref(n)) == _lib.E_INVALID
    assert L.apss_query_stored_dev(None, 0, None, None, None) == _lib.E_INVALID
    assert L.apss_stored_query_get(None, ctypes.byref(info)) == _lib.E_INVALID


def test_every_binding_carries_the_call():
    engine = open(os.path.join(PKG, "apss", "engine.py")).read()
    for text in ("def query_stored(self, ids, fetch=True)", "def stored_query_info(self)", "apss_query_stored_dev", "apss_stored_query_get"):
        assert text in engine, text
    hpp = open(os.path.join(PKG, "host", "cpslab_host.hpp")).read()
    cpp = open(os.path.join(PKG, "host", "cpslab_host.cpp")).read()
    assert "SimilarityOutput similarTo(const std::vector<std::string> &ids);" in hpp
    assert "apss_query_stored(h_, " in cpp and "term-sharded" in cpp[cpp.index("GpuIndexingWorker::similarTo"):cpp.index("apss_query_stored(h_, ")]
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert re.search(r"^host_query_stored_selftest:", mk, re.M) and re.search(r"^all:.*\bhost_query_stored_selftest\b", mk, re.M)
    assert "similarTo" in open(os.path.join(PKG, "host", "host_query_stored_selftest.cpp")).read()
    jni = open(os.path.join(PKG, "jvm", "apss_jni.c")).read()
    assert "if (mode == 6) return apss_query_stored((apss_handle *)t, n, id, NULL, n_res);" in jni
    scala = open(os.path.join(PKG, "jvm", "NativeApss.scala")).read()
    assert re.search(r"def queryStored\(h: Long, ids: Array\[Long\]\): Long", scala) and "submit(h, 6, " in scala
    actor = open(os.path.join(PKG, "jvm", "GpuIndexingWorkerActor.scala")).read()
    assert re.search(r"def similarTo\(names: Iterable\[String\]\)", actor) and "NativeApss.queryStored(handle, " in actor
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "apss_query_stored" in text, doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 5g" in design and "k_qs_gather" in design
    nine = design[design.index("## 9"):]
    assert "apss_query_stored" in nine and "group" in nine.lower()
