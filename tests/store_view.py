"""What ingest left in HBM, read back element by element, and the same rows restated in numpy float64.

read_store(ix)          the store of one handle (rowptr, indices, values, ext ids) copied to the host
reference_store(...)    ingest restated in plain float64, batch after batch, in the order k_ingest_count / k_ingest_write
                        implement: normalise by the WHOLE row's norm -> admission on the sum of the normalised, unpruned row
                        -> value prune with strict `>` -> term range.  A row emptied by prune or range stays (empty, with its
                        ext id); a row refused by admission vanishes and the later rows close up.
assert_store_equal(...) structure exact, values bit-equal or inside a per-row relative bound
row_rel_tol / band_cases  the derived bound of a normalised weight and the inputs whose decision it leaves open

The bound of a normalised weight (inputs exact in fp32, u = 2^-24 the unit roundoff, every error relative):
  * the row's sum of squares: each of 16 lanes adds its ceil(nnz / 16) squares, then 4 butterfly steps add the lanes: a chain
    of D = ceil(nnz / 16) + 4 additions of positive terms, each term a rounded (or fused: no worse) product -> <= (D + 1) u
  * the square root halves that: (D + 1) u / 2 = (D + 1) / 4 * 2^-23
  * sqrtf, the reciprocal and the product val * inv round once each, allowed 2^-23, 2^-23 and 2^-24 (device sqrtf and
    division are not promised to round correctly; one unit in the last place each covers them)
  sum: ((D + 1) / 4 + 2.5) * 2^-23 <= (D / 4 + 3) * 2^-23 =: rel_tol.  nnz <= 16: D = 5, 4.25 * 2^-23 = 5.1e-7;
  nnz = 700: D = 48, 15 * 2^-23 = 1.8e-6.
A decision on such a weight (prune: val * inv > thr, admission: sum of val * inv >= theta, the sum another chain of D fp32
additions) may go either way when the float64 value lies within rel_tol (a sum: rel_tol + D * 2^-24) of its threshold: the
tests fix their seeds so that band_cases() is empty, and then compare the structure exactly.  Without normalisation the
tests' values are dyadic and every fp32 operation on them is exact: no band."""
import collections
import ctypes as C
import math

import numpy as np

from apss import _lib

Store = collections.namedtuple("Store", "rowptr indices values ext_ids src_nnz")
# rowptr int64 [rows + 1] (absolute), indices int32, values float32 (device) or float64 (reference), ext_ids int64 [rows],
# src_nnz int64 [rows]: entries of the INPUT row a stored row came from (what its bound depends on; None for a device store)

HIP_MEMCPY_DEVICE_TO_HOST = 2
_hip = None


def _hip_runtime():
    """the ONE HIP runtime already mapped in this process (a second copy would know nothing of the library's allocations)"""
    global _hip
    if _hip is None:
        paths = _lib.hip_runtimes_loaded()
        assert len(paths) == 1, "expected exactly one HIP runtime in the process: %s" % (paths,)
        _hip = C.CDLL(paths[0])
        _hip.hipMemcpy.restype = C.c_int
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return _hip


def _to_host(dev_ptr, count, dtype):
    out = np.empty(count, dtype)
    if count:
        assert dev_ptr, "null device pointer for %d elements" % count
        rc = _hip_runtime().hipMemcpy(out.ctypes.data, dev_ptr, out.nbytes, HIP_MEMCPY_DEVICE_TO_HOST)
        assert rc == 0, "hipMemcpy failed: %d" % rc
    return out


def store_pointers(ix):
    """(rowptr, indices, values, ext ids) device pointers (ints, 0 = null) + rows + nnz of a handle's store"""
    L, h = ix._L, ix._h
    rp, idx, val, ext = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    rows, nnz = C.c_int64(-1), C.c_int64(-1)
    assert L.apss_get_store_dev(h, C.byref(rp), C.byref(idx), C.byref(val), C.byref(rows), C.byref(nnz)) == _lib.OK
    assert L.apss_ext_ids_dev(h, C.byref(ext), None) == _lib.OK
    return rp.value or 0, idx.value or 0, val.value or 0, ext.value or 0, rows.value, nnz.value


def read_store(ix):
    """every library call has synchronised before it returned: a plain blocking copy is enough"""
    rp, idx, val, ext, rows, nnz = store_pointers(ix)
    assert (rows, nnz) == ix.size()
    if rows == 0:
        return Store(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.int64), None)
    return Store(_to_host(rp, rows + 1, np.int64), _to_host(idx, nnz, np.int32), _to_host(val, nnz, np.float32),
                 _to_host(ext, rows, np.int64), None)


def row_rel_tol(src_nnz):
    """(D / 4 + 3) * 2^-23 with D = ceil(nnz / 16) + 4 (module docstring), per row"""
    d = -(-np.asarray(src_nnz, np.int64) // 16) + 4
    return (d / 4.0 + 3.0) * 2.0 ** -23


def _sum_rel_band(src_nnz):
    d = -(-np.asarray(src_nnz, np.int64) // 16) + 4
    return row_rel_tol(src_nnz) + d * 2.0 ** -24


def _normalised_rows(rowptr, values, flags):
    """float64 rows after the optional L2 normalisation (LG:34-37): values / sqrt(sum of squares) of the whole row"""
    rowptr = np.asarray(rowptr, np.int64)
    v = np.array(values, np.float64, copy=True)
    if flags & _lib.FLAG_NORMALIZE:
        for r in range(rowptr.size - 1):
            b, e = rowptr[r], rowptr[r + 1]
            if e > b:
                norm = math.sqrt(float(np.sum(v[b:e] * v[b:e])))
                assert norm > 0.0, "a row of explicit zeros is outside what the reference states (0 / 0)"
                v[b:e] = v[b:e] / norm
    return v


def reference_store(batches, dim, flags=0, theta=0.0, index_threshold=0.0, term_range=None):
    """batches: [(ids, rowptr, indices, values), ...] in insertion order.  The thresholds are the two numbers the device
    compares against: float32(theta) and float32(index_threshold)."""
    lo, hi = (0, dim) if term_range is None else term_range
    th, thr = float(np.float32(theta)), float(np.float32(index_threshold))
    o_rp, o_idx, o_val, o_ext, o_src = [0], [], [], [], []
    for ids, rowptr, indices, values in batches:
        rowptr, indices = np.asarray(rowptr, np.int64), np.asarray(indices, np.int32)
        v = _normalised_rows(rowptr, values, flags)
        for r in range(rowptr.size - 1):
            b, e = rowptr[r], rowptr[r + 1]
            rv, ri = v[b:e], indices[b:e]
            if (flags & _lib.FLAG_ADMISSION) and not float(np.sum(rv)) >= th:  # EPA:89, on the unpruned row
                continue
            keep = np.ones(e - b, bool)
            if flags & _lib.FLAG_VALUE_PRUNE:
                keep &= rv > thr  # WWA:192, strict
            keep &= (ri >= lo) & (ri < hi)
            o_idx.append(ri[keep])
            o_val.append(rv[keep])
            o_rp.append(o_rp[-1] + int(keep.sum()))
            o_ext.append(int(ids[r]))
            o_src.append(int(e - b))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)  # noqa: E731
    return Store(np.array(o_rp, np.int64), cat(o_idx, np.int32), cat(o_val, np.float64), np.array(o_ext, np.int64),
                 np.array(o_src, np.int64))


def band_cases(batches, flags, theta, index_threshold):
    """[(batch, row, entry or None), ...]: every entry (prune) and every row (admission; entry None) whose float64 value lies
    within the fp32 bound of its threshold, so that the device may decide either way.  Only normalised values carry an
    error: without APSS_FLAG_NORMALIZE there is no band (the tests' un-normalised values are exact in fp32)."""
    if not flags & _lib.FLAG_NORMALIZE:
        return []
    th, thr = float(np.float32(theta)), float(np.float32(index_threshold))
    out = []
    for bi, (_, rowptr, _, values) in enumerate(batches):
        rowptr = np.asarray(rowptr, np.int64)
        v = _normalised_rows(rowptr, values, flags)
        nnz = np.diff(rowptr)
        tol, stol = row_rel_tol(nnz), _sum_rel_band(nnz)
        for r in range(rowptr.size - 1):
            rv = v[rowptr[r]:rowptr[r + 1]]
            if flags & _lib.FLAG_ADMISSION:
                s = float(np.sum(rv))
                if abs(s - th) <= stol[r] * max(abs(s), abs(th)):
                    out.append((bi, r, None))
            if flags & _lib.FLAG_VALUE_PRUNE:
                for k in np.nonzero(np.abs(rv - thr) <= tol[r] * np.maximum(np.abs(rv), abs(thr)))[0]:
                    out.append((bi, r, int(k)))
    return out


# row lengths at the edges of k_ingest_count's 16-lane stride and of k_ingest_write's per-sweep compaction
RAGGED = (0, 1, 2, 15, 16, 17, 31, 32, 33, 100, 700)


def ragged_batch(rng, lengths, dim, scales=None, first_id=0, id_step=1, low=0.05, high=1.0):
    """(ids, rowptr, indices, values) with rows of the given lengths: distinct ascending indices in [0, dim), values drawn
    in [low, high) (times the row's scale), cast to fp32 and widened -- the narrowing on the device is then exact, and the
    host path (doubles) and the device path (floats) must leave the same bits"""
    lengths = np.asarray(lengths, np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(dim, int(n), replace=False)) for n in lengths] + [np.zeros(0, np.int64)]).astype(np.int32)
    values = rng.uniform(low, high, int(rowptr[-1]))
    if scales is not None:
        values = values * np.repeat(np.asarray(scales, np.float64), lengths)
    values = values.astype(np.float32).astype(np.float64)
    ids = first_id + id_step * np.arange(lengths.size, dtype=np.int64)
    return ids, rowptr, indices, values


def _row_of(rowptr, pos):
    """(row, entry within the row) of position pos of a CSR's entry arrays"""
    r = int(np.searchsorted(rowptr, pos, side="right")) - 1
    return r, int(pos - rowptr[r])


def assert_store_equal(got, want, rel_tol_per_row=None):
    """rowptr, indices and ext ids exactly equal; values bit-equal (rel_tol_per_row None: `want` must then be exact in fp32)
    or each within its row's relative bound of `want`.  The message names the first offending row and entry."""
    g_rows, w_rows = got.rowptr.size - 1, want.rowptr.size - 1
    m = min(g_rows, w_rows)
    g_len, w_len = np.diff(got.rowptr), np.diff(want.rowptr)
    # rows first: a missing or extra row shifts everything behind it
    bad = np.nonzero((got.ext_ids[:m] != want.ext_ids[:m]) | (g_len[:m] != w_len[:m]))[0]
    if g_rows != w_rows:
        r = int(bad[0]) if bad.size else m
        raise AssertionError("store has %d rows, reference %d; first difference at row %d (ext id %s with %s entries, reference "
                             "%s with %s)" % (g_rows, w_rows, r, got.ext_ids[r] if r < g_rows else "-", g_len[r] if r < g_rows else "-",
                                              want.ext_ids[r] if r < w_rows else "-", w_len[r] if r < w_rows else "-"))
    assert got.rowptr[0] == want.rowptr[0] == 0, "rowptr[0] is %d, reference %d" % (got.rowptr[0], want.rowptr[0])
    bad = np.nonzero(got.rowptr != want.rowptr)[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError("rowptr[%d] (end of row %d) is %d, reference %d" % (i, i - 1, got.rowptr[i], want.rowptr[i]))
    bad = np.nonzero(got.ext_ids != want.ext_ids)[0]
    if bad.size:
        r = int(bad[0])
        raise AssertionError("row %d: ext id %d, reference %d" % (r, got.ext_ids[r], want.ext_ids[r]))
    nnz = int(want.rowptr[-1])
    assert got.indices.size == want.indices.size == nnz and got.values.size == want.values.size == nnz, \
        "entry arrays hold %d / %d entries, rowptr says %d" % (got.indices.size, got.values.size, nnz)
    bad = np.nonzero(got.indices != want.indices)[0]
    if bad.size:
        r, k = _row_of(want.rowptr, int(bad[0]))
        raise AssertionError("row %d entry %d: index %d, reference %d" % (r, k, got.indices[bad[0]], want.indices[bad[0]]))
    if rel_tol_per_row is None:
        w32 = want.values.astype(np.float32)
        inexact = np.nonzero(w32.astype(np.float64) != want.values.astype(np.float64))[0]
        if inexact.size:
            r, k = _row_of(want.rowptr, int(inexact[0]))
            raise AssertionError("row %d entry %d: reference %r is not an fp32 number: a bit-exact comparison needs one" % (r, k, want.values[inexact[0]]))
        bad = np.nonzero(got.values.astype(np.float32).view(np.uint32) != w32.view(np.uint32))[0]
        if bad.size:
            r, k = _row_of(want.rowptr, int(bad[0]))
            raise AssertionError("row %d entry %d: value %r, reference %r (bit-exact comparison)" % (r, k, float(got.values[bad[0]]), float(want.values[bad[0]])))
        return 0.0
    tol = np.repeat(np.asarray(rel_tol_per_row, np.float64), w_len)
    w = want.values.astype(np.float64)
    err = np.abs(got.values.astype(np.float64) - w)
    bad = np.nonzero(~(err <= tol * np.abs(w)))[0]  # (~<=: a NaN offends)
    if bad.size:
        r, k = _row_of(want.rowptr, int(bad[0]))
        raise AssertionError("row %d entry %d: value %r, reference %r: relative error %.3g * 2^-23 > bound %.3g * 2^-23" %
                             (r, k, float(got.values[bad[0]]), float(w[bad[0]]), err[bad[0]] / abs(w[bad[0]]) * 2.0 ** 23, tol[bad[0]] * 2.0 ** 23))
    # largest |got - ref| / |ref| in units of 2^-23 (a reference of exactly 0 passed the bound only with an error of 0)
    return float(np.max(err / np.where(w != 0.0, np.abs(w), 1.0)) * 2.0 ** 23) if nnz else 0.0
