"""The store comparison of tests/store_view.py checked without a GPU: its numpy reference agrees with the oracle's
restatements of the reference's three ingest steps, and assert_store_equal rejects every kind of defect the GPU tests
(tests/test_gpu_ingest.py) rely on it to reject.  These self-checks are the proof that the comparison can fail: no broken
kernel is ever run for it (a count / write mismatch in ingest writes out of bounds)."""
import numpy as np
import pytest

from apss import _lib
from store_view import RAGGED, Store, assert_store_equal, band_cases, ragged_batch, reference_store, row_rel_tol

DIM = 2000
NPA = _lib.FLAG_NORMALIZE | _lib.FLAG_VALUE_PRUNE | _lib.FLAG_ADMISSION


def _batch(seed=5):
    rng = np.random.default_rng(seed)
    lengths = rng.permutation(np.repeat(RAGGED, 4))
    b = ragged_batch(rng, lengths, DIM, scales=10.0 ** rng.uniform(-3, 3, lengths.size), first_id=500, id_step=3)
    # every third row gets negative entries: the normalised sum of a non-negative row is >= 1 and would always be admitted
    ids, rp, idx, val = b
    for r in range(0, lengths.size, 3):
        val[rp[r]:rp[r + 1]:2] *= -1.0
    return ids, rp, idx, val


def test_reference_agrees_with_the_oracle_steps(oracle):
    """LoadGenerator.scala:34-37 (l2_normalize), WriteWorkerActor.scala:188-194 (value_prune), EntryProxyActor.scala:81-93
    (admission), each against the numpy reference on a ragged batch: values within 1e-15, decisions identical"""
    ids, rp, idx, val = _batch()
    theta, thr = 0.75, 0.125
    assert not band_cases([(ids, rp, idx, val)], NPA, theta, thr)
    # normalise alone: every row stays, every entry stays
    ref_n = reference_store([(ids, rp, idx, val)], DIM, _lib.FLAG_NORMALIZE)
    nv = oracle.l2_normalize(rp, val)
    assert np.array_equal(ref_n.rowptr, rp) and np.array_equal(ref_n.indices, idx) and np.array_equal(ref_n.ext_ids, ids)
    assert np.max(np.abs(ref_n.values - nv)) <= 1e-15
    assert np.array_equal(ref_n.src_nnz, np.diff(rp))
    # normalise + prune: the oracle prunes ITS normalised rows; same entries, same values
    ref_p = reference_store([(ids, rp, idx, val)], DIM, _lib.FLAG_NORMALIZE | _lib.FLAG_VALUE_PRUNE, index_threshold=thr)
    prp, pidx, pval = oracle.value_prune(rp, idx, nv, thr)
    assert 0 < pidx.size < idx.size and (np.diff(prp) == 0).sum() > (np.diff(rp) == 0).sum()  # some rows emptied: they stay
    assert np.array_equal(ref_p.rowptr, prp) and np.array_equal(ref_p.indices, pidx)
    assert np.max(np.abs(ref_p.values - pval)) <= 1e-15
    # all three: admission on the normalised UNPRUNED row, then the prune
    keep = oracle.admission(rp, nv, theta)
    assert 4 < keep.sum() < keep.size - 4
    ref_a = reference_store([(ids, rp, idx, val)], DIM, NPA, theta=theta, index_threshold=thr)
    assert np.array_equal(ref_a.ext_ids, ids[keep])
    assert np.array_equal(np.diff(ref_a.rowptr), np.diff(prp)[keep])
    sel = np.repeat(keep, np.diff(prp))
    assert np.array_equal(ref_a.indices, pidx[sel]) and np.max(np.abs(ref_a.values - pval[sel])) <= 1e-15
    # the pruned row is not normalised again
    norms = np.sqrt(np.add.reduceat(np.append(ref_a.values, 0.0) ** 2, ref_a.rowptr[:-1]))[np.diff(ref_a.rowptr) > 0]
    assert norms.min() < 0.9 and norms.max() <= 1.0 + 1e-15


def test_reference_batches_continue_and_term_range_slices():
    rng = np.random.default_rng(11)
    b1 = ragged_batch(rng, [3, 0, 5], 50, first_id=10)
    b2 = ragged_batch(rng, [4, 2], 50, first_id=90)
    ref = reference_store([b1, b2], 50)
    assert list(ref.rowptr) == [0, 3, 3, 8, 12, 14] and list(ref.ext_ids) == [10, 11, 12, 90, 91]
    assert np.array_equal(ref.values, np.concatenate([b1[3], b2[3]]))
    ids = np.array([7, 8])
    rp, idx, val = np.array([0, 4, 6]), np.array([9, 10, 19, 20, 3, 30], np.int32), np.array([1.0, 2.0, 2.0, 4.0, 1.0, 1.0])
    sh = reference_store([(ids, rp, idx, val)], 50, _lib.FLAG_NORMALIZE, term_range=(10, 20))
    assert list(sh.rowptr) == [0, 2, 2] and list(sh.indices) == [10, 19] and list(sh.ext_ids) == [7, 8]
    assert np.allclose(sh.values, [0.4, 0.4], rtol=1e-15) and list(sh.src_nnz) == [4, 2]  # the whole row's norm (5), not the slice's


def test_band_cases_finds_a_value_and_a_sum_at_their_thresholds():
    ids, rp, idx = np.array([1, 2]), np.array([0, 2, 4]), np.array([0, 1, 0, 1], np.int32)
    val = np.array([3.0, 4.0, 1.0, 1.0])  # normalised: (0.6, 0.8), sum 1.4; (0.7071, 0.7071)
    b = [(ids, rp, idx, val)]
    assert band_cases(b, _lib.FLAG_NORMALIZE | _lib.FLAG_VALUE_PRUNE, 0.0, 0.6) == [(0, 0, 0)]
    assert band_cases(b, _lib.FLAG_NORMALIZE | _lib.FLAG_ADMISSION, 1.4, 0.0) == [(0, 0, None)]
    assert band_cases(b, NPA, 1.3, 0.5) == []
    assert band_cases(b, _lib.FLAG_VALUE_PRUNE, 0.0, 3.0) == []  # un-normalised values are exact: no band


@pytest.fixture(scope="module")
def ref():
    ids, rp, idx, val = _batch()
    r = reference_store([(ids, rp, idx, val)], DIM, NPA, theta=0.75, index_threshold=0.125)
    assert r.ext_ids.size > 10 and (np.diff(r.rowptr) >= 3).sum() > 5
    return r


def _as_device(st, **repl):
    """a copy of a reference store as a device store would come back (fp32 values), with fields replaced"""
    d = dict(rowptr=st.rowptr.copy(), indices=st.indices.copy(), values=st.values.astype(np.float32), ext_ids=st.ext_ids.copy(), src_nnz=None)
    d.update(repl)
    return Store(**d)


def _long_row(st):
    return int(np.nonzero(np.diff(st.rowptr) >= 3)[0][2])


def test_the_rounded_reference_passes_and_exact_mode_wants_fp32_numbers(ref):
    tol = row_rel_tol(ref.src_nnz)
    worst = assert_store_equal(_as_device(ref), ref, tol)
    assert 0.0 < worst <= 0.5  # rounding to fp32: at most half a unit in the last place, 2^-24 relative
    with pytest.raises(AssertionError, match="not an fp32 number"):
        assert_store_equal(_as_device(ref), ref)
    ref32 = ref._replace(values=ref.values.astype(np.float32).astype(np.float64))
    assert assert_store_equal(_as_device(ref32), ref32) == 0.0


def test_rejects_a_value_off_by_twice_its_bound(ref):
    tol = row_rel_tol(ref.src_nnz)
    r = _long_row(ref)
    p = int(ref.rowptr[r]) + 1
    for sign in (1.0, -1.0):
        v = ref.values.copy()
        v[p] *= 1.0 + sign * 0.5 * tol[r]
        assert_store_equal(_as_device(ref, values=v.astype(np.float32)), ref, tol)  # inside the bound: accepted
        v[p] = ref.values[p] * (1.0 + sign * 2.0 * tol[r])
        with pytest.raises(AssertionError, match=r"row %d entry 1: value" % r):
            assert_store_equal(_as_device(ref, values=v.astype(np.float32)), ref, tol)
    # bit-exact mode: one unit in the last place is enough
    ref32 = ref._replace(values=ref.values.astype(np.float32).astype(np.float64))
    v = ref32.values.astype(np.float32)
    v[p] = np.nextafter(v[p], np.float32(2.0))
    with pytest.raises(AssertionError, match=r"row %d entry 1: value .* \(bit-exact" % r):
        assert_store_equal(_as_device(ref32, values=v), ref32)


def test_rejects_an_entry_at_exactly_the_threshold_that_is_kept():
    """prune is strict: a store that kept an entry EQUAL to the threshold (a `>=` in the kernel) is refused"""
    ids, rp, idx = np.array([4, 5]), np.array([0, 3, 5]), np.array([1, 5, 9, 2, 3], np.int32)
    val = np.array([0.5, 0.25, 0.75, 0.25, 1.0])
    want = reference_store([(ids, rp, idx, val)], 16, _lib.FLAG_VALUE_PRUNE, index_threshold=0.25)
    assert list(want.rowptr) == [0, 2, 3] and list(want.values) == [0.5, 0.75, 1.0]
    assert_store_equal(_as_device(want), want)
    lax = Store(np.array([0, 3, 4]), np.array([1, 5, 9, 3], np.int32), np.array([0.5, 0.25, 0.75, 1.0], np.float32), ids, None)
    with pytest.raises(AssertionError, match=r"rowptr\[1\] \(end of row 0\) is 3, reference 2"):
        assert_store_equal(lax, want)


def test_rejects_two_neighbouring_entries_swapped(ref):
    tol = row_rel_tol(ref.src_nnz)
    r = _long_row(ref)
    p = int(ref.rowptr[r])
    idx, val = ref.indices.copy(), ref.values.astype(np.float32)
    idx[[p, p + 1]] = idx[[p + 1, p]]
    val[[p, p + 1]] = val[[p + 1, p]]
    with pytest.raises(AssertionError, match=r"row %d entry 0: index" % r):
        assert_store_equal(_as_device(ref, indices=idx, values=val), ref, tol)
    # the values alone swapped (indices in order): caught by the values
    assert abs(ref.values[p] - ref.values[p + 1]) > 1e-3 * ref.values[p]
    with pytest.raises(AssertionError, match=r"row %d entry 0: value" % r):
        assert_store_equal(_as_device(ref, values=val), ref, tol)


def test_rejects_a_rowptr_entry_off_by_one(ref):
    tol = row_rel_tol(ref.src_nnz)
    r = _long_row(ref)
    for d in (1, -1):
        rp = ref.rowptr.copy()
        rp[r + 1] += d
        with pytest.raises(AssertionError, match=r"rowptr\[%d\] \(end of row %d\) is %d, reference %d" % (r + 1, r, rp[r + 1], ref.rowptr[r + 1])):
            assert_store_equal(_as_device(ref, rowptr=rp), ref, tol)
    rp = ref.rowptr.copy()
    rp[-1] += 1  # the total: the entry arrays no longer match it either
    with pytest.raises(AssertionError):
        assert_store_equal(_as_device(ref, rowptr=rp), ref, tol)


def test_rejects_two_ext_ids_exchanged(ref):
    tol = row_rel_tol(ref.src_nnz)
    ext = ref.ext_ids.copy()
    ext[[3, 4]] = ext[[4, 3]]
    with pytest.raises(AssertionError, match=r"row 3: ext id %d, reference %d" % (ref.ext_ids[4], ref.ext_ids[3])):
        assert_store_equal(_as_device(ref, ext_ids=ext), ref, tol)


def test_rejects_one_admitted_row_missing(ref):
    tol = row_rel_tol(ref.src_nnz)
    r = _long_row(ref)
    b, e = int(ref.rowptr[r]), int(ref.rowptr[r + 1])
    rp = np.concatenate([ref.rowptr[:r + 1], ref.rowptr[r + 2:] - (e - b)])
    got = Store(rp, np.delete(ref.indices, np.s_[b:e]), np.delete(ref.values, np.s_[b:e]).astype(np.float32), np.delete(ref.ext_ids, r), None)
    with pytest.raises(AssertionError, match=r"store has %d rows, reference %d; first difference at row %d " % (rp.size - 1, ref.rowptr.size - 1, r)):
        assert_store_equal(got, ref, tol)
    # an EMPTY row missing (emptied by the prune: it must stay) is a missing row too
    empty = np.nonzero(np.diff(ref.rowptr) == 0)[0]
    assert empty.size
    r = int(empty[0])
    got = Store(np.delete(ref.rowptr, r + 1), ref.indices, ref.values.astype(np.float32), np.delete(ref.ext_ids, r), None)
    with pytest.raises(AssertionError, match=r"first difference at row %d " % r):
        assert_store_equal(got, ref, tol)
