"""CPU-side checks of the per-query top-k boundary: the four entry points are exported and listed, apss_topk_info is mirrored
field for field, NULL objects are refused without touching a device, the pinned structs did not grow, and the host mirror and
the JVM binding carry the new setting."""
import ctypes
import os
import re

import pytest

from apss import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "all-pairs-similarity_amd")
TOPK_SYMBOLS = ["apss_set_top_k", "apss_topk_get", "apss_group_set_top_k", "apss_group_topk_get"]


@pytest.fixture(scope="module")
def so():
    return _lib.build()


def _header():
    return open(os.path.join(ROOT, "include", "apss.h")).read()


def test_topk_symbols_are_declared_listed_and_exported(so):
    hdr = _header()
    L = ctypes.CDLL(so)
    for sym in TOPK_SYMBOLS:
        assert re.search(r"\bint32_t %s\s*\(" % sym, hdr), sym
        assert sym in _lib.SYMBOLS, sym
        assert getattr(L, sym) is not None


def test_topk_info_matches_the_header():
    hdr = _header()
    body = re.search(r"typedef struct apss_topk_info \{(.*?)\} apss_topk_info;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int64_t|int32_t|double)\s+([a-z_0-9]+)\s*;", body)
    ctype = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "double": ctypes.c_double}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.TopkInfo._fields_)
    assert [n for _, n in fields] == ["struct_size", "k", "pairs_over_theta", "kept", "queries_cut", "longest_segment",
                                      "select_ms", "select_launches", "reserved0"]
    assert ctypes.sizeof(_lib.TopkInfo) == 56
    assert int(re.search(r"#define\s+APSS_TOP_K_MAX\s+(\d+)", hdr).group(1)) == _lib.TOP_K_MAX == 1024


def test_null_objects_are_refused(so):
    L = _lib.lib()
    ti = _lib.TopkInfo()
    ti.struct_size = ctypes.sizeof(_lib.TopkInfo)
    assert L.apss_set_top_k(None, 1) == _lib.E_INVALID
    assert L.apss_topk_get(None, ctypes.byref(ti)) == _lib.E_INVALID
    assert L.apss_group_set_top_k(None, 1) == _lib.E_INVALID
    assert L.apss_group_topk_get(None, ctypes.byref(ti)) == _lib.E_INVALID


def test_pinned_structs_did_not_grow():
    assert ctypes.sizeof(_lib.Config) == 64
    assert ctypes.sizeof(_lib.Stats) == 288
    assert ctypes.sizeof(_lib.GroupStats) == 424


def test_python_face_takes_top_k():
    import inspect
    from apss.engine import ApssGroup, ApssIndex
    for cls in (ApssIndex, ApssGroup):
        assert inspect.signature(cls.__init__).parameters["top_k"].default == 0
        assert callable(cls.set_top_k) and callable(cls.topk_info)


def test_host_mirror_config_has_topk():
    hpp = open(os.path.join(PKG, "host", "cpslab_host.hpp")).read()
    conf = re.search(r"struct Config \{(.*?)\n\};", hpp, re.S).group(1)
    assert re.search(r"\bint topK = 0;", conf)
    assert "cpslab.allpair.gpu.topK" in conf
    cpp = open(os.path.join(PKG, "host", "cpslab_host.cpp")).read()
    assert "apss_set_top_k(h_, conf.topK)" in cpp and "apss_group_set_top_k(g_, conf.topK)" in cpp
    mk = open(os.path.join(PKG, "host", "Makefile")).read()
    assert re.search(r"^host_topk_selftest:", mk, re.M)


def _params(text):
    return [p.strip() for p in text.replace("\n", " ").split(",") if p.strip()]


def test_scala_and_shim_agree_on_the_new_argument():
    scala = open(os.path.join(PKG, "jvm", "NativeApss.scala")).read()
    shim = open(os.path.join(PKG, "jvm", "apss_jni.c")).read()
    for name, setter in (("create", "apss_set_top_k"), ("createGroup", "apss_group_set_top_k")):
        sp = _params(re.search(r"@native def %s\((.*?)\): Long" % name, scala, re.S).group(1))
        cp = _params(re.search(r"Java_cpslab_gpu_NativeApss_%s\((.*?)\)\s*\{" % name, shim, re.S).group(1))
        assert sp[-1] == "topK: Int", sp
        assert cp[-1] == "jint topK", cp
        assert len(cp) == len(sp) + 2  # JNIEnv *, jclass
        body = shim.split("Java_cpslab_gpu_NativeApss_%s(" % name, 1)[1].split("\nJNIEXPORT", 1)[0]
        assert "%s(" % setter in body and "topK)" in body
        assert "destroy" in body.split(setter, 1)[1]  # a refusal destroys the object: a failed create
    actor = open(os.path.join(PKG, "jvm", "GpuIndexingWorkerActor.scala")).read()
    assert 'conf.getInt("cpslab.allpair.gpu.topK")' in actor
