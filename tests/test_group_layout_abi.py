"""CPU-side checks of the group's layout interface (include/apss.h: apss_group_layout, apss_group_relayout,
apss_group_layout_get): the ctypes mirror lists the header's fields in order and the entry points refuse a NULL group
without touching a device."""
import ctypes
import os
import re

import pytest

from apss import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


def test_group_layout_fields_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "apss.h")).read()
    body = re.search(r"typedef struct apss_group_layout \{(.*?)\} apss_group_layout;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [m.group(1) for m in re.finditer(r"\b(?:int64_t|uint32_t|int32_t|double|float|char)\s+([a-z_0-9]+)\s*(?:\[[^\]]+\])?\s*;", body)]
    assert fields == [f for f, _ in _lib.GroupLayout._fields_], (fields, [f for f, _ in _lib.GroupLayout._fields_])
    assert re.match(r"\s*int32_t struct_size;", body)
    assert _lib.GroupLayout.term_cuts.size == 4 * (_lib.GROUP_MAX_MEMBERS + 1)
    assert _lib.GroupLayout.dfsq.size == 8 * _lib.GROUP_MAX_MEMBERS
    assert _lib.GROUP_ADAPT_LAYOUT == 4


def test_layout_entry_points_refuse_a_null_group(L):
    cuts = (ctypes.c_int32 * 3)(0, 5, 10)
    assert L.apss_group_relayout(None, None) == _lib.E_INVALID
    assert L.apss_group_relayout(None, cuts) == _lib.E_INVALID
    lo = _lib.GroupLayout()
    lo.struct_size = ctypes.sizeof(_lib.GroupLayout)
    assert L.apss_group_layout_get(None, ctypes.byref(lo)) == _lib.E_INVALID
    assert L.apss_group_layout_get(None, None) == _lib.E_INVALID


def test_store_entry_points_refuse_a_null_handle(L):
    n = ctypes.c_int64(7)
    assert L.apss_get_store_dev(None, None, None, None, ctypes.byref(n), None) == _lib.E_INVALID
    assert L.apss_insert_stored_dev(None, 0, 0, None, None, None, None) == _lib.E_INVALID
