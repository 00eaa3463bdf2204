"""CPU-side checks of the grid interface of apss_group (include/apss.h: apss_group_create_grid, apss_group_grid,
apss_group_grid_get): declared, listed, exported; the ctypes mirror lists the header's fields in order; bad shapes are refused
before a device is touched; the JNI shim reaches the grid through the native entry points it already had."""
import ctypes
import os
import re
import subprocess

import pytest

from apss import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JVM = os.path.join(ROOT, "all-pairs-similarity_amd", "jvm")
NEW = ("apss_group_create_grid", "apss_group_grid_get")


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def test_grid_symbols_are_declared_listed_and_exported(L):
    hdr = open(os.path.join(ROOT, "include", "apss.h")).read()
    declared = set(re.findall(r"\b(apss_[a-z_]+)\s*\(", hdr))
    for sym in NEW:
        assert sym in declared and sym in _lib.SYMBOLS
        assert getattr(L, sym) is not None
    assert _lib.GROUP_NO_SYMMETRIC_RANGES == 8
    assert re.search(r"#define\s+APSS_GROUP_NO_SYMMETRIC_RANGES\s+8u", hdr)


def test_group_grid_fields_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "apss.h")).read()
    body = re.search(r"typedef struct apss_group_grid \{(.*?)\} apss_group_grid;", hdr, re.S).group(1)
    assert re.match(r"\s*int32_t struct_size;", body)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [m.group(1) for m in re.finditer(r"\b(?:int64_t|uint32_t|int32_t|double|float|char)\s+([a-z_0-9]+)\s*(?:\[[^\]]+\])?\s*;", body)]
    assert fields == [f for f, _ in _lib.GroupGrid._fields_], (fields, [f for f, _ in _lib.GroupGrid._fields_])
    assert fields == ["struct_size", "n_term_ranges", "n_row_ranges", "symmetric_ranges", "rows_in_range", "outside_rows_max",
                      "mirrored_pairs", "own_ms_max", "outside_ms_max"]
    assert _lib.GroupGrid.rows_in_range.size == 8 * _lib.GROUP_MAX_MEMBERS
    assert ctypes.sizeof(_lib.GroupGrid) == 16 + 8 * 64 + 32
    # the grid adds a struct of its own: the two older ones keep their sizes
    assert ctypes.sizeof(_lib.GroupStats) == 424


def test_create_grid_refuses_bad_shapes_before_touching_a_device(L):
    """APSS_E_INVALID for a missing argument or a shape outside 1 <= T, 1 <= D, T x D <= 64, APSS_E_UNSUPPORTED for a grid that
    adapts its layout: all decided on the arguments alone (the same answers with and without a GPU)"""
    cfg = _lib.Config()
    cfg.struct_size = ctypes.sizeof(_lib.Config)
    cfg.dim, cfg.theta = 100, 0.5
    devs = (ctypes.c_int32 * 128)()
    g = ctypes.c_void_p()
    for T, D in ((0, 1), (1, 0), (-1, 2), (2, -1), (65, 1), (1, 65), (13, 5), (8, 9), (1 << 30, 1 << 30)):
        assert L.apss_group_create_grid(ctypes.byref(cfg), T, D, devs, 0, ctypes.byref(g)) == _lib.E_INVALID, (T, D)
        assert not g.value and L.apss_group_last_error(None)
    assert L.apss_group_create_grid(None, 2, 2, devs, 0, ctypes.byref(g)) == _lib.E_INVALID
    assert L.apss_group_create_grid(ctypes.byref(cfg), 2, 2, None, 0, ctypes.byref(g)) == _lib.E_INVALID
    assert L.apss_group_create_grid(ctypes.byref(cfg), 2, 2, devs, 0, None) == _lib.E_INVALID
    assert L.apss_group_create_grid(ctypes.byref(cfg), 2, 2, devs, _lib.GROUP_ADAPT_LAYOUT, ctypes.byref(g)) == _lib.E_UNSUPPORTED
    assert b"row range" in L.apss_group_last_error(None)
    bad = _lib.Config()
    bad.struct_size = 8
    assert L.apss_group_create_grid(ctypes.byref(bad), 2, 2, devs, 0, ctypes.byref(g)) == _lib.E_INVALID
    gr = _lib.GroupGrid()
    gr.struct_size = ctypes.sizeof(_lib.GroupGrid)
    assert L.apss_group_grid_get(None, ctypes.byref(gr)) == _lib.E_INVALID


def test_python_group_checks_the_shape():
    from apss.engine import ApssGroup
    with pytest.raises(ValueError):
        ApssGroup(100, 0.5, [0, 0, 0], row_ranges=2)


def test_jni_shim_reaches_the_grid_and_still_type_checks():
    """createGroupGrid is a Scala method over the native createGroup (the set of native entry points does not grow): the shim
    reads the row ranges out of groupFlags and calls apss_group_create_grid"""
    out = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "stubs"),
                          "-I", os.path.join(ROOT, "include"), os.path.join(JVM, "apss_jni.c")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    c = open(os.path.join(JVM, "apss_jni.c")).read()
    scala = open(os.path.join(JVM, "NativeApss.scala")).read()
    actor = open(os.path.join(JVM, "GpuIndexingWorkerActor.scala")).read()
    assert "apss_group_create_grid(" in c and "(groupFlags >> 16) & 0xff" in c
    assert re.search(r"\bdef createGroupGrid\(", scala) and "(rowRanges << 16)" in scala
    assert "GROUP_NO_SYMMETRIC_RANGES = 8" in scala
    assert "cpslab.allpair.gpu.rowRanges" in actor and "createGroupGrid(" in actor
