"""apss_set_top_pairs / apss_top_pairs_get at the drop-in boundary, without a GPU: declared, listed, exported, mirrored field for
field, NULL refused, no pinned struct grown, and every binding and document carries the feature."""
import ctypes
import os
import re
import subprocess

import pytest

from apss import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "all-pairs-similarity_amd")
NEW = ("apss_set_top_pairs", "apss_top_pairs_get")
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
    assert re.search(r"^int32_t apss_set_top_pairs\(apss_handle \*h, int64_t k_pairs\);", hdr, re.M)
    assert re.search(r"^int32_t apss_top_pairs_get\(apss_handle \*h, apss_top_pairs_info \*out\);", hdr, re.M)
    assert re.search(r"^#define APSS_TOP_PAIRS_MAX \(1 << 20\)", hdr, re.M) and _lib.TOP_PAIRS_MAX == 1 << 20
    # the semantics stand in the header: the setting, the order's five items, the answer, where the cut runs, the errors, groups
    comment = hdr[hdr.index("global top-K: a call's K best pairs"):hdr.index("#define APSS_TOP_PAIRS_MAX")]
    for text in ("launches nothing new, reads nothing new and allocates nothing", "leaves the last call's results alone and survives",
                 "1. fp32 score descending", "-0.0f counts as +0.0f and is reported as +0.0f", "2. Query external id ascending (signed int64)",
                 "3. Candidate external id ascending", "4. Query row within the batch ascending", "5. Candidate slot ascending",
                 "first min(K, n) pairs", "apss_results_copy_dev", "apss_stats.result_pairs",
                 "With n <= K nothing is dropped, but the list is still put into rank order", "Score bits are unchanged",
                 "after k_rm_drop: a row marked removed never takes a place among the K",
                 "after the per-query cut if k > 0", "replaces \"grouped by query\"",
                 "apss_set_top_k_window) once, after the windows' lists are concatenated", "pairs_in is what they handed over",
                 "both directions of a pair are two pairs", "k_pairs < 0 or > APSS_TOP_PAIRS_MAX", "term shard", "partial scores",
                 "APSS_E_STATE", "apss_group has no such call"):
        assert text in comment, text


def test_struct_is_mirrored_field_for_field(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "apss.h")).read()
    body = re.search(r"typedef struct apss_top_pairs_info \{(.*?)\} apss_top_pairs_info;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for t, names in re.findall(r"\b(int64_t|int32_t|double)\s+([a-z_0-9, ]+);", body):
        fields += [(n.strip(), C_TYPES[t]) for n in names.split(",")]
    assert fields == list(_lib.TopPairsInfo._fields_)
    assert [n for n, _ in fields] == ["struct_size", "launches", "k_pairs", "pairs_in", "kept", "above", "tied", "tied_kept",
                                      "kth_score", "select_ms"]
    # its size, and the pinned structs', compiled from the header
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "apss.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   "sizeof(apss_top_pairs_info), sizeof(apss_config), sizeof(apss_stats), sizeof(apss_group_stats), sizeof(apss_topk_info), "
                   "sizeof(apss_topk_window_info), sizeof(apss_topk_tile_cut_info), sizeof(apss_removal_info), "
                   "sizeof(apss_stored_query_info)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = subprocess.check_output([str(exe)], text=True).split()
    assert out == ["72", "64", "288", "424", "56", "80", "32", "88", "64"], out
    assert ctypes.sizeof(_lib.TopPairsInfo) == 72
    assert (ctypes.sizeof(_lib.Config), ctypes.sizeof(_lib.Stats), ctypes.sizeof(_lib.GroupStats), ctypes.sizeof(_lib.TopkInfo),
            ctypes.sizeof(_lib.TopkWindowInfo), ctypes.sizeof(_lib.TopkTileCutInfo), ctypes.sizeof(_lib.RemovalInfo),
            ctypes.sizeof(_lib.StoredQueryInfo)) == (64, 288, 424, 56, 80, 32, 88, 64)


def test_null_is_refused(so):
    L = _lib.lib()
    info = _lib.TopPairsInfo()
    info.struct_size = ctypes.sizeof(info)
    assert L.apss_set_top_pairs(None, 5) == _lib.E_INVALID
    assert L.apss_set_top_pairs(None, 0) == _lib.E_INVALID
    assert L.apss_top_pairs_get(None, ctypes.byref(info)) == _lib.E_INVALID


def test_every_binding_carries_the_feature():
    engine = open(os.path.join(PKG, "apss", "engine.py")).read()
    for text in ("top_pairs=0", "def set_top_pairs(self, K)", "def top_pairs_info(self)", "apss_set_top_pairs", "apss_top_pairs_get"):
        assert text in engine, text
    hpp = open(os.path.join(PKG, "host", "cpslab_host.hpp")).read()
    cpp = open(os.path.join(PKG, "host", "cpslab_host.cpp")).read()
    assert re.search(r"\blong topPairs = 0;", hpp) and "cpslab.allpair.gpu.topPairs" in hpp
    assert "apss_set_top_pairs(h_, conf.topPairs)" in cpp and "cpslab.allpair.gpu.topPairs ignored" in cpp
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert re.search(r"^host_top_pairs_selftest:", mk, re.M) and re.search(r"^all:.*\bhost_top_pairs_selftest\b", mk, re.M)
    assert "topPairs" in open(os.path.join(PKG, "host", "host_top_pairs_selftest.cpp")).read()
    jni = open(os.path.join(PKG, "jvm", "apss_jni.c")).read()
    assert "apss_set_top_pairs((apss_handle *)t, " in jni
    scala = open(os.path.join(PKG, "jvm", "NativeApss.scala")).read()
    assert re.search(r"def setTopPairs\(h: Long, pairs: Long\): Int", scala)
    assert re.search(r"def create\(dim: Int, theta: Double, indexThreshold: Double, flags: Int, device: Int, topKTileCut: Int,\s+"
                     r"headTerms: Int, topKWindowPairs: Long, topK: Int\): Long", scala)  # (its signature is as it was)
    actor = open(os.path.join(PKG, "jvm", "GpuIndexingWorkerActor.scala")).read()
    assert "cpslab.allpair.gpu.topPairs" in actor and "NativeApss.setTopPairs(handle, topPairs)" in actor
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    # the object's and the assembly's dependency lists: both name the one header list, and the header is in it
    assert "apss_top_pairs.hpp" in re.search(r"^HDRS\s*=(.*)$", mk, re.M).group(1).split()
    assert all("$(HDRS)" in re.search(r"^%s:(.*)$" % rule, mk, re.M).group(1).split() for rule in (r"apss_hip\.o", "asm"))
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "apss_set_top_pairs" in text, doc
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 5h" in design and "k_tp_hist" in design and "tp_grid" in design
    nine = design[design.index("## 9"):]
    assert "a GLOBAL top-k" not in nine
    for text in ("apss_set_top_pairs", "group", "2^20", "inside the"):
        assert text in nine, text
    assert os.path.exists(os.path.join(ROOT, "profiles", "top_pairs.md"))
