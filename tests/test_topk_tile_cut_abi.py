"""apss_set_top_k_tile_cut / apss_topk_tile_cut_get at the drop-in boundary, without a GPU: declared, exported, mirrored field
for field, NULL refused, no pinned struct grown, and every binding carries the setting."""
import ctypes
import os
import re
import subprocess

import pytest

from apss import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "all-pairs-similarity_amd")
NEW = ("apss_set_top_k_tile_cut", "apss_topk_tile_cut_get")
C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}


@pytest.fixture(scope="module")
def so():
    return _lib.build()


def test_symbols_declared_listed_and_exported(so):
    hdr = open(os.path.join(ROOT, "include", "apss.h")).read()
    L = ctypes.CDLL(so)
    for sym in NEW:
        assert re.search(r"^int32_t %s\(apss_handle \*h, " % sym, hdr, re.M), sym
        assert sym in _lib.SYMBOLS
        assert getattr(L, sym) is not None


def test_struct_is_mirrored_field_for_field():
    hdr = open(os.path.join(ROOT, "include", "apss.h")).read()
    body = re.search(r"typedef struct apss_topk_tile_cut_info \{(.*?)\} apss_topk_tile_cut_info;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int64_t|int32_t)\s+([a-z_0-9]+)\s*;", body)
    assert [(n, C_TYPES[t]) for t, n in fields] == list(_lib.TopkTileCutInfo._fields_)
    assert [n for _, n in fields] == ["struct_size", "applied", "declined", "prefix_bits", "pairs_emitted", "rounds_cut"]
    assert ctypes.sizeof(_lib.TopkTileCutInfo) == 32
    for name, val in re.findall(r"#define\s+APSS_(TILE_CUT_[A-Z_]+)\s+(\d+)", hdr):
        assert getattr(_lib, name) == int(val), name
    assert (_lib.TILE_CUT_RAN, _lib.TILE_CUT_OFF, _lib.TILE_CUT_NO_K, _lib.TILE_CUT_PATH) == (0, 1, 2, 3)


def test_null_is_refused(so):
    L = _lib.lib()
    info = _lib.TopkTileCutInfo()
    info.struct_size = ctypes.sizeof(info)
    assert L.apss_set_top_k_tile_cut(None, 1) == _lib.E_INVALID
    assert L.apss_set_top_k_tile_cut(None, 0) == _lib.E_INVALID
    assert L.apss_topk_tile_cut_get(None, ctypes.byref(info)) == _lib.E_INVALID


def test_no_pinned_struct_grew(tmp_path):
    assert ctypes.sizeof(_lib.Config) == 64
    assert ctypes.sizeof(_lib.Stats) == 288
    assert ctypes.sizeof(_lib.GroupStats) == 424
    assert ctypes.sizeof(_lib.TopkInfo) == 56
    assert ctypes.sizeof(_lib.TopkWindowInfo) == 80
    # ... and the header agrees with the mirrors
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "apss.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(apss_config), '
                   "sizeof(apss_stats), sizeof(apss_group_stats), sizeof(apss_topk_info), sizeof(apss_topk_window_info), "
                   "sizeof(apss_topk_tile_cut_info)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["64", "288", "424", "56", "80", "32"]


def test_every_binding_carries_the_setting():
    engine = open(os.path.join(PKG, "apss", "engine.py")).read()
    assert "top_k_tile_cut=False" in engine and "def topk_tile_cut_info(self)" in engine and "def set_top_k_tile_cut(self, on)" in engine
    hpp = open(os.path.join(PKG, "host", "cpslab_host.hpp")).read()
    cpp = open(os.path.join(PKG, "host", "cpslab_host.cpp")).read()
    assert re.search(r"bool topKTileCut = false;", hpp) and "cpslab.allpair.gpu.topKTileCut" in hpp
    assert "apss_set_top_k_tile_cut(h_, 1)" in cpp
    assert "topKTileCut" in open(os.path.join(PKG, "host", "host_topk_selftest.cpp")).read()
    jni = open(os.path.join(PKG, "jvm", "apss_jni.c")).read()
    assert "apss_set_top_k_tile_cut(h, topKTileCut)" in jni
    scala = open(os.path.join(PKG, "jvm", "NativeApss.scala")).read()
    assert re.search(r"@native def create\([^)]*topKTileCut: Int,\s+headTerms: Int, topKWindowPairs: Long, topK: Int\)", scala, re.S)
    actor = open(os.path.join(PKG, "jvm", "GpuIndexingWorkerActor.scala")).read()
    assert '"cpslab.allpair.gpu.topKTileCut"' in actor and "devices(0), topKTileCut, headTerms, topKWindowPairs, topK)" in actor
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert "apss_set_top_k_tile_cut" in open(os.path.join(ROOT, doc)).read(), doc
