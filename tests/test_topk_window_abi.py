"""CPU-side checks of the windowed top-k boundary: the three entry points are declared, listed and exported,
apss_topk_window_info is mirrored field for field, NULL objects are refused without touching a device, the pinned structs did
not grow, and the Python face, the host mirror and the JVM binding carry the new setting."""
import ctypes
import os
import re

import pytest

from apss import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "all-pairs-similarity_amd")
WINDOW_SYMBOLS = ["apss_set_top_k_window", "apss_topk_window_get", "apss_topk_window_cuts"]


@pytest.fixture(scope="module")
def so():
    return _lib.build()


def _header():
    return open(os.path.join(ROOT, "include", "apss.h")).read()


def test_window_symbols_are_declared_listed_and_exported(so):
    hdr = _header()
    L = ctypes.CDLL(so)
    for sym in WINDOW_SYMBOLS:
        assert re.search(r"\bint32_t %s\s*\(" % sym, hdr), sym
        assert not re.search(r"\d", sym)
        assert sym in _lib.SYMBOLS, sym
        assert getattr(L, sym) is not None


def test_window_info_matches_the_header():
    hdr = _header()
    body = re.search(r"typedef struct apss_topk_window_info \{(.*?)\} apss_topk_window_info;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int64_t|int32_t|double)\s+([a-z_0-9]+)\s*;", body)
    ctype = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "double": ctypes.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.TopkWindowInfo._fields_)
    assert [(t, n) for t, n in fields] == [
        ("int32_t", "struct_size"), ("int32_t", "windows"), ("int64_t", "max_pairs"), ("int64_t", "bound_total"),
        ("int64_t", "bound_window_max"), ("int64_t", "pairs_window_max"), ("int64_t", "rows_window_min"),
        ("int64_t", "rows_window_max"), ("int64_t", "single_row_over"), ("int32_t", "overflow_reruns"),
        ("int32_t", "plan_launches"), ("double", "plan_ms")]
    assert ctypes.sizeof(_lib.TopkWindowInfo) == 80


def test_null_objects_are_refused(so):
    L = _lib.lib()
    wi = _lib.TopkWindowInfo()
    wi.struct_size = ctypes.sizeof(_lib.TopkWindowInfo)
    n = ctypes.c_int64(0)
    assert L.apss_set_top_k_window(None, 1000) == _lib.E_INVALID
    assert L.apss_topk_window_get(None, ctypes.byref(wi)) == _lib.E_INVALID
    assert L.apss_topk_window_cuts(None, 0, None, ctypes.byref(n)) == _lib.E_INVALID


def test_pinned_structs_did_not_grow():
    assert ctypes.sizeof(_lib.Config) == 64
    assert ctypes.sizeof(_lib.Stats) == 288
    assert ctypes.sizeof(_lib.GroupStats) == 424
    assert ctypes.sizeof(_lib.TopkInfo) == 56
    body = re.search(r"typedef struct apss_topk_info \{(.*?)\} apss_topk_info;", _header(), re.S).group(1)
    assert "reserved0" in body


def test_python_face_takes_top_k_window():
    import inspect
    from apss.engine import ApssIndex
    assert inspect.signature(ApssIndex.__init__).parameters["top_k_window"].default == 0
    for name in ("set_top_k_window", "topk_window_info", "topk_window_cuts"):
        assert callable(getattr(ApssIndex, name)), name


def test_host_mirror_config_has_the_key():
    hpp = open(os.path.join(PKG, "host", "cpslab_host.hpp")).read()
    conf = re.search(r"struct Config \{(.*?)\n\};", hpp, re.S).group(1)
    assert re.search(r"\blong topKWindowPairs = 0;", conf)
    assert "cpslab.allpair.gpu.topKWindowPairs" in conf
    cpp = open(os.path.join(PKG, "host", "cpslab_host.cpp")).read()
    assert "apss_set_top_k_window(h_, conf.topKWindowPairs)" in cpp
    assert cpp.index("apss_set_top_k_window(h_, conf.topKWindowPairs)") < cpp.index("apss_set_top_k(h_, conf.topK)")
    assert "apss_set_top_k_window(g_" not in cpp  # groups are left alone
    selftest = open(os.path.join(PKG, "host", "host_topk_selftest.cpp")).read()
    assert "topKWindowPairs" in selftest


def _params(text):
    return [p.strip() for p in text.replace("\n", " ").split(",") if p.strip()]


def test_scala_and_shim_agree_on_the_new_argument():
    scala = open(os.path.join(PKG, "jvm", "NativeApss.scala")).read()
    shim = open(os.path.join(PKG, "jvm", "apss_jni.c")).read()
    sp = _params(re.search(r"@native def create\((.*?)\): Long", scala, re.S).group(1))
    cp = _params(re.search(r"Java_cpslab_gpu_NativeApss_create\((.*?)\)\s*\{", shim, re.S).group(1))
    assert sp[-2:] == ["topKWindowPairs: Long", "topK: Int"], sp
    assert cp[-2:] == ["jlong topKWindowPairs", "jint topK"], cp
    assert len(cp) == len(sp) + 2  # JNIEnv *, jclass
    body = shim.split("Java_cpslab_gpu_NativeApss_create(", 1)[1].split("\nJNIEXPORT", 1)[0]
    assert "apss_set_top_k_window(" in body and "topKWindowPairs)" in body
    assert "destroy" in body.split("apss_set_top_k_window", 1)[1]  # a refusal destroys the handle: a failed create
    # createGroup is left alone, and no native method was added for the setting
    gp = _params(re.search(r"@native def createGroup\((.*?)\): Long", scala, re.S).group(1))
    assert "topKWindowPairs: Long" not in gp
    assert len(re.findall(r"@native def \w*[Ww]indow", scala)) == 0
    actor = open(os.path.join(PKG, "jvm", "GpuIndexingWorkerActor.scala")).read()
    assert 'conf.getLong("cpslab.allpair.gpu.topKWindowPairs")' in actor
    assert "headTerms, topKWindowPairs, topK)" in actor
