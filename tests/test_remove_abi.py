"""apss_remove / apss_remove_dev / apss_compact / apss_set_auto_compact / apss_removal_get at the drop-in boundary, without a GPU:
declared, listed, exported, mirrored field for field, NULL refused, no pinned struct grown, and every binding carries them."""
import ctypes
import os
import re
import subprocess

import pytest

from apss import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "all-pairs-similarity_amd")
NEW = ("apss_remove", "apss_remove_dev", "apss_compact", "apss_set_auto_compact", "apss_removal_get")
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
    assert re.search(r"^int32_t apss_remove\(apss_handle \*h, int64_t n, const int64_t \*ext_ids, int64_t \*n_rows_removed\);", hdr, re.M)
    assert re.search(r"^int32_t apss_remove_dev\(apss_handle \*h, int64_t n, const int64_t \*d_ext_ids, int64_t \*n_rows_removed\);", hdr, re.M)
    assert re.search(r"^int32_t apss_set_auto_compact\(apss_handle \*h, double fraction\);", hdr, re.M)


def test_struct_is_mirrored_field_for_field(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "apss.h")).read()
    body = re.search(r"typedef struct apss_removal_info \{(.*?)\} apss_removal_info;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for t, names in re.findall(r"\b(int64_t|int32_t|double)\s+([a-z_0-9, ]+);", body):
        fields += [(n.strip(), C_TYPES[t]) for n in names.split(",")]
    assert fields == list(_lib.RemovalInfo._fields_)
    assert [n for n, _ in fields] == ["struct_size", "compactions", "rows_removed", "rows_live", "removed_total", "pairs_dropped",
                                      "compacted_rows", "auto_compact", "mark_ms", "drop_ms", "compact_ms", "drop_launches", "reserved0"]
    # its size, and the pinned structs', compiled from the header
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "apss.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", '
                   "sizeof(apss_removal_info), sizeof(apss_config), sizeof(apss_stats), sizeof(apss_group_stats), sizeof(apss_topk_info), "
                   "sizeof(apss_topk_window_info), sizeof(apss_topk_tile_cut_info), APSS_TILE_CUT_REMOVED); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split()
    assert out == [str(ctypes.sizeof(_lib.RemovalInfo)), "64", "288", "424", "56", "80", "32", "4"], out
    assert ctypes.sizeof(_lib.RemovalInfo) == 88
    assert _lib.TILE_CUT_REMOVED == 4
    assert (ctypes.sizeof(_lib.Config), ctypes.sizeof(_lib.Stats), ctypes.sizeof(_lib.GroupStats), ctypes.sizeof(_lib.TopkInfo),
            ctypes.sizeof(_lib.TopkWindowInfo), ctypes.sizeof(_lib.TopkTileCutInfo)) == (64, 288, 424, 56, 80, 32)


def test_null_is_refused(so):
    L = _lib.lib()
    info = _lib.RemovalInfo()
    info.struct_size = ctypes.sizeof(info)
    n = ctypes.c_int64(0)
    ids = (ctypes.c_int64 * 1)(3)
    assert L.apss_remove(None, 1, ctypes.cast(ids, ctypes.c_void_p), ctypes.byref(n)) == _lib.E_INVALID
    assert L.apss_remove_dev(None, 0, None, None) == _lib.E_INVALID
    assert L.apss_compact(None) == _lib.E_INVALID
    assert L.apss_set_auto_compact(None, 0.5) == _lib.E_INVALID
    assert L.apss_removal_get(None, ctypes.byref(info)) == _lib.E_INVALID


def test_every_binding_carries_removal():
    engine = open(os.path.join(PKG, "apss", "engine.py")).read()
    for text in ("auto_compact=0.0", "def remove(self, ids)", "def compact(self)", "def removal_info(self)",
                 "def set_auto_compact(self, fraction)", "apss_remove_dev"):
        assert text in engine, text
    hpp = open(os.path.join(PKG, "host", "cpslab_host.hpp")).read()
    cpp = open(os.path.join(PKG, "host", "cpslab_host.cpp")).read()
    assert re.search(r"double autoCompact = 0\.0;", hpp) and "cpslab.allpair.gpu.autoCompact" in hpp
    assert "int64_t remove(const std::vector<std::string> &ids);" in hpp and "bool compact();" in hpp
    assert "apss_set_auto_compact(h_, conf.autoCompact)" in cpp and "apss_remove(h_, " in cpp and "apss_compact(h_)" in cpp
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert re.search(r"^host_remove_selftest:", mk, re.M) and re.search(r"^all:.*\bhost_remove_selftest\b", mk, re.M)
    assert "autoCompact" in open(os.path.join(PKG, "host", "host_remove_selftest.cpp")).read()
    jni = open(os.path.join(PKG, "jvm", "apss_jni.c")).read()
    assert "apss_remove((apss_handle *)t, n, id, n_res)" in jni and "apss_compact((apss_handle *)t)" in jni
    assert "apss_set_auto_compact((apss_handle *)t, " in jni
    scala = open(os.path.join(PKG, "jvm", "NativeApss.scala")).read()
    assert re.search(r"def remove\(h: Long, ids: Array\[Long\]\): Long", scala) and re.search(r"def compact\(h: Long\): Int", scala)
    assert re.search(r"def setAutoCompact\(h: Long, fraction: Double\): Int", scala)
    actor = open(os.path.join(PKG, "jvm", "GpuIndexingWorkerActor.scala")).read()
    assert '"cpslab.allpair.gpu.autoCompact"' in actor and "NativeApss.setAutoCompact(handle, autoCompact)" in actor
    assert "NativeApss.remove(handle, " in actor
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "apss_remove" in text and "apss_compact" in text, doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "5f" in design and "APSS_TILE_CUT_REMOVED" in design
