"""CPU-side checks of the index view's boundary: apss_index_view_get is declared, listed and exported, apss_index_view is
mirrored field for field at the header's offsets, NULL objects are refused without touching a device, and the pinned structs did
not grow."""
import ctypes
import os
import re

import pytest

from apss import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def so():
    return _lib.build()


def _header():
    return open(os.path.join(ROOT, "include", "apss.h")).read()


def test_index_view_symbol_is_declared_listed_and_exported(so):
    assert re.search(r"\bint32_t apss_index_view_get\s*\(apss_handle \*h, int32_t rendering, apss_index_view \*out\);", _header())
    assert "apss_index_view_get" in _lib.SYMBOLS
    assert getattr(ctypes.CDLL(so), "apss_index_view_get") is not None


def test_index_view_matches_the_header():
    hdr = _header()
    body = re.search(r"typedef struct apss_index_view \{(.*?)\} apss_index_view;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(int64_t|int32_t|double|const void \*|const int64_t \*|const float \*)\s*([a-z_0-9]+)\s*;", body)
    ctype = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "double": ctypes.c_double, "const void *": ctypes.c_void_p,
             "const int64_t *": ctypes.c_void_p, "const float *": ctypes.c_void_p}
    assert len(fields) == body.count(";")  # no field of a type this test does not know
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.IndexView._fields_)
    assert [n for _, n in fields] == ["struct_size", "rendering", "tile_rows", "seg_align", "posting_bytes", "slot_form",
                                      "weights_scaled", "dim", "n_tiles", "built_rows", "post_used", "d_seg", "d_base", "d_post",
                                      "d_sub", "d_tile_min", "max_seg", "long_segs", "chunk_weight"]
    assert ctypes.sizeof(_lib.IndexView) == 120
    offsets = {n: getattr(_lib.IndexView, n).offset for n, _ in _lib.IndexView._fields_}
    assert offsets == {"struct_size": 0, "rendering": 4, "tile_rows": 8, "seg_align": 12, "posting_bytes": 16, "slot_form": 20,
                       "weights_scaled": 24, "dim": 28, "n_tiles": 32, "built_rows": 40, "post_used": 48, "d_seg": 56, "d_base": 64,
                       "d_post": 72, "d_sub": 80, "d_tile_min": 88, "max_seg": 96, "long_segs": 104, "chunk_weight": 112}
    for name in ("PLAIN", "TIMES2", "WIDE"):
        assert int(re.search(r"#define\s+APSS_SLOT_%s\s+(\d+)" % name, hdr).group(1)) == getattr(_lib, "SLOT_" + name)
    assert (_lib.SLOT_PLAIN, _lib.SLOT_TIMES2, _lib.SLOT_WIDE) == (0, 1, 2)


def test_the_library_lays_the_struct_out_as_the_header_says(so, tmp_path):
    """sizeof and offsetof as a C compiler sees the header, against the ctypes mirror"""
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc is not None, "no C compiler (the CPU oracle needs one too)"
    names = [n for n, _ in _lib.IndexView._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "apss.h"\nint main(void) {\n  printf("%zu", sizeof(apss_index_view));\n' +
                   "".join('  printf(" %%zu", offsetof(apss_index_view, %s));\n' % n for n in names) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out == [ctypes.sizeof(_lib.IndexView)] + [getattr(_lib.IndexView, n).offset for n in names]


def test_null_objects_are_refused(so):
    L = _lib.lib()
    v = _lib.IndexView()
    v.struct_size = ctypes.sizeof(_lib.IndexView)
    assert L.apss_index_view_get(None, 0, ctypes.byref(v)) == _lib.E_INVALID
    assert L.apss_index_view_get(None, 1, None) == _lib.E_INVALID


def test_the_accessor_launches_and_reserves_nothing():
    """the accessor's body: no kernel launch, no allocation, no copy, no synchronisation -- it copies out what the handle knows"""
    src = open(os.path.join(_lib.CSRC, "apss_hip.hip")).read()
    body = src.split("int32_t apss_index_view_get(", 1)[1].split("\nint32_t apss_query_dev(", 1)[0]
    for word in ("hipLaunchKernelGGL", "ensure(", "hipMalloc", "hipMemcpy", "hipMemset", "Synchronize", "build_tiles", "build_index", "enter("):
        assert word not in body, word


def test_pinned_structs_did_not_grow():
    assert ctypes.sizeof(_lib.Config) == 64
    assert ctypes.sizeof(_lib.Stats) == 288
    assert ctypes.sizeof(_lib.GroupStats) == 424
