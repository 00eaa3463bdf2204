"""Ingest, element by element: what k_narrow_f64, k_ingest_count, scan_i64 (one kernel, or three above 16,384 rows),
k_ingest_write and the host side of ingest() / upload() / insert_dev_impl() leave in HBM, read back through
apss_get_store_dev + apss_ext_ids_dev and compared with the float64 restatement of tests/store_view.py.

Everything without normalisation is compared bit for bit (the inputs are fp32 numbers, so the host path's doubles narrow
exactly); a normalised weight must lie within the derived bound of store_view.row_rel_tol (its docstring has the
derivation), and every test with normalisation first asserts ON THE REFERENCE that no prune or admission decision lies
within that bound of its threshold -- the structure (rowptr, indices, ext ids) is then compared exactly, never within a band.
That the comparison itself can fail is shown without a GPU in tests/test_store_compare.py."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_same_pairs, to_map
from store_view import (RAGGED, Store, assert_store_equal, band_cases, ragged_batch, read_store, reference_store, row_rel_tol,
                        store_pointers)

pytestmark = pytest.mark.gpu
DIM = 2000


@pytest.fixture(scope="module")
def engine():
    from apss import _lib, engine
    _lib.lib()  # raises if the HIP library is missing: no fallback
    return engine


@pytest.fixture(scope="module")
def F():
    from apss import _lib
    return _lib


def _to_device(batch):
    import torch
    ids, rp, idx, val = batch
    d = torch.device("cuda:0")
    t = (torch.from_numpy(np.ascontiguousarray(ids, np.int64)).to(d), torch.from_numpy(np.ascontiguousarray(rp, np.int64)).to(d),
         torch.from_numpy(np.ascontiguousarray(idx, np.int32)).to(d), torch.from_numpy(np.ascontiguousarray(val, np.float32)).to(d))
    torch.cuda.synchronize()
    return t


def _store_after(engine, batches, path, dim=DIM, theta=0.5, **cfg):
    """the store after the batches went in through apss_insert (`host`: doubles, narrowed on the device) or apss_insert_dev"""
    with engine.ApssIndex(dim, theta, **cfg) as ix:
        for b in batches:
            if path == "host":
                ix.insert(*b)
            else:
                t = _to_device(b)
                ix.insert_dev(*t)
                del t
        return read_store(ix)


def _both_paths(engine, batches, **cfg):
    host = _store_after(engine, batches, "host", **cfg)
    dev = _store_after(engine, batches, "dev", **cfg)
    assert_store_equal(dev, host)  # same bits, whichever way the batch came
    return host


def _concat(batches):
    ids = np.concatenate([b[0] for b in batches])
    rp = np.concatenate([[0]] + [b[1][1:] + off for b, off in zip(batches, np.cumsum([0] + [int(b[1][-1]) for b in batches[:-1]]))])
    return ids, rp.astype(np.int64), np.concatenate([b[2] for b in batches]).astype(np.int32), np.concatenate([b[3] for b in batches])


def _rows(ids, rows, first_id=None):
    """a batch from explicit rows [(indices, values), ...]"""
    rp = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.int64)
    idx = np.concatenate([np.asarray(r[0], np.int64) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int32)
    val = np.concatenate([np.asarray(r[1], np.float64) for r in rows] + [np.zeros(0)])
    assert np.array_equal(val.astype(np.float32).astype(np.float64), val)
    return np.asarray(ids, np.int64), rp, idx, val


def _with_negatives(batch, rows):
    """every second entry of the given rows negated: the normalised sum of a non-negative row is >= 1, so only such rows (and
    empty ones) can be refused by an admission threshold <= 1; a prune threshold > 0 drops the negative entries"""
    ids, rp, idx, val = batch
    val = val.copy()
    for r in rows:
        val[rp[r]:rp[r + 1]:2] *= -1.0
    return ids, rp, idx, val


# ---- case 1: no flags, three batches, the store reallocates
def test_plain_batches_append_bit_for_bit(engine):
    rng = np.random.default_rng(101)
    lens = np.tile(RAGGED, 31)
    batches = [ragged_batch(rng, [17], DIM, first_id=7_000_000, id_step=5),
               ragged_batch(rng, rng.permutation(lens[:37]), DIM, first_id=8_000_000, id_step=5),
               ragged_batch(rng, rng.permutation(lens[:300]), DIM, first_id=9_000_000, id_step=5)]
    want = reference_store(batches, DIM)
    whole = _concat(batches)
    # the reference of this case is the input itself: absolute rowptr across the batches, ext ids in order
    assert np.array_equal(want.rowptr, whole[1]) and np.array_equal(want.indices, whole[2])
    assert np.array_equal(want.values, whole[3]) and np.array_equal(want.ext_ids, whole[0])
    for path in ("host", "dev"):
        got = _store_after(engine, batches, path, capacity_rows=0, capacity_nnz=0)
        assert_store_equal(got, want)


# ---- case 2: normalise
def test_normalised_weights_within_the_derived_bound(engine, F):
    rng = np.random.default_rng(202)
    lens = rng.permutation(np.repeat(RAGGED, 6))
    batch = ragged_batch(rng, lens, DIM, scales=10.0 ** np.linspace(-3, 3, lens.size), first_id=300, id_step=2)
    want = reference_store([batch], DIM, F.FLAG_NORMALIZE)
    assert np.array_equal(want.rowptr, batch[1]) and (np.diff(want.rowptr) == 0).sum() == 6  # empty rows stay
    tol = row_rel_tol(want.src_nnz)
    assert abs(tol[want.src_nnz > 0].min() - 4.25 * 2.0 ** -23) < 1e-20 and abs(tol.max() - 15 * 2.0 ** -23) < 1e-20
    got = _both_paths(engine, [batch], flags=F.FLAG_NORMALIZE)
    worst = assert_store_equal(got, want, tol)
    print("case 2 (normalise): largest |got - ref| / ref = %.3f * 2^-23" % worst)


# ---- case 3: prune only, exact arithmetic, every keep pattern around the 16-lane sweeps
def _prune_pattern_batch(rng):
    rows, names = [], []
    for n in (16, 17, 32, 33, 100):
        k = np.arange(n)
        pats = {"all": k >= 0, "none": k < 0, "all but the first": k > 0, "all but the last": k < n - 1,
                "even": k % 2 == 0, "odd": k % 2 == 1, "lanes 15|16": (k == 15) | (k == 16)}
        if n > 32:
            pats["lanes 31|32"] = (k == 31) | (k == 32)
        if n > 96:
            pats["lanes 95|96"] = (k == 95) | (k == 96)
        for name, keep in pats.items():
            v = np.where(keep, rng.integers(17, 65, n), np.where(rng.random(n) < 0.5, 16, rng.integers(1, 16, n))) / 64.0
            drop = np.nonzero(~keep)[0]
            if drop.size:
                v[drop[0]] = 0.25  # at least one entry EQUAL to the threshold in every row that drops anything
            rows.append((np.sort(rng.choice(DIM, n, replace=False)), v))
            names.append((n, name, int(keep.sum())))
    return _rows(40_000 + 3 * np.arange(len(rows)), rows), names


def test_prune_is_strict_and_keeps_the_order(engine, F):
    batch, names = _prune_pattern_batch(np.random.default_rng(303))
    assert (batch[3] == 0.25).sum() >= len(names) - 5
    want = reference_store([batch], DIM, F.FLAG_VALUE_PRUNE, index_threshold=0.25)
    assert list(np.diff(want.rowptr)) == [kept for _, _, kept in names]  # "none": the row stays, empty
    assert want.values.min() > 0.25 and want.ext_ids.size == len(names)
    got = _both_paths(engine, [batch], flags=F.FLAG_VALUE_PRUNE, index_threshold=0.25)
    assert_store_equal(got, want)


# ---- case 4: normalise + prune: the pruned row is not normalised again
def test_normalise_then_prune(engine, F):
    rng = np.random.default_rng(404)
    lens = rng.permutation(np.repeat(RAGGED, 6))
    batch = ragged_batch(rng, lens, DIM, scales=10.0 ** rng.uniform(-3, 3, lens.size), first_id=11, id_step=7)
    flags, thr = F.FLAG_NORMALIZE | F.FLAG_VALUE_PRUNE, 0.1
    assert band_cases([batch], flags, 0.0, thr) == []
    want = reference_store([batch], DIM, flags, index_threshold=thr)
    kept = np.diff(want.rowptr)
    assert 0 < want.indices.size < batch[2].size and (kept[want.src_nnz == 700] == 0).all() and (kept[want.src_nnz == 1] == 1).all()
    norms = np.sqrt(np.add.reduceat(np.append(want.values, 0.0) ** 2, want.rowptr[:-1]))[kept > 0]
    assert norms.min() < 0.9  # rows that lost entries keep the weights of the WHOLE row's norm
    got = _both_paths(engine, [batch], flags=flags, index_threshold=thr)
    worst = assert_store_equal(got, want, row_rel_tol(want.src_nnz))
    print("case 4 (normalise + prune): largest |got - ref| / ref = %.3f * 2^-23" % worst)


# ---- case 5: admission around the single-kernel scan limit, exact sums
THETA_A = 1.5


def _admission_batch(rng, n, first_id, admitted=(), refused=()):
    """rows of 0..3 entries, values multiples of 1/1024 (every fp32 sum of them is exact in any order); the rows `admitted`
    sum to exactly theta, the rows `refused` to theta - 1/1024"""
    lens = rng.integers(0, 4, n)
    if n > 8192:
        lens[4096:8192] = 1  # one entry < 1 < theta: every row of this whole 4,096-block is refused
    lens[list(admitted) + list(refused)] = 3
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    # ascending indices inside a row: running sums of gaps in [1, 600), restarted at every row (3 * 599 < DIM)
    gaps = rng.integers(1, 600, int(rp[-1]))
    run = np.cumsum(gaps)
    idx = (run - np.repeat((run - gaps)[rp[:-1][lens > 0]], lens[lens > 0])).astype(np.int32)
    val = rng.integers(1, 1024, int(rp[-1])) / 1024.0
    for r in admitted:
        val[rp[r]:rp[r + 1]] = [0.5, 0.5, 0.5]
    for r in refused:
        val[rp[r]:rp[r + 1]] = [0.5, 0.5, 0.5 - 1.0 / 1024]
    return first_id + 3 * np.arange(n, dtype=np.int64), rp, idx, val


@pytest.mark.parametrize("n", [16384, 16385, 20480, 20481])
def test_admission_compacts_rows_and_ext_ids(engine, F, n):
    """both sides of scan_i64's single-kernel limit (16,384 rows), a whole and a ragged last 4,096-block; refused: the first
    row, the last row, every row of block 1; admitted: both neighbours of that block and both sides of later block edges"""
    refused = [0, 101, n - 1]
    admitted = sorted({r for r in (100, 4095, 8192, 12287, 12288, 16383) if r < n - 2} | {n - 2})
    batch = _admission_batch(np.random.default_rng(500 + n), n, 1_000_000, admitted, refused)
    second = _admission_batch(np.random.default_rng(77), 100, 5_000_000, [10], [11])
    for b in (batch, second):
        assert (np.diff(b[2])[np.diff(np.repeat(np.arange(b[0].size), np.diff(b[1]))) == 0] > 0).all() and b[2].max() < DIM
    want1 = reference_store([batch], DIM, F.FLAG_ADMISSION, theta=THETA_A)
    want2 = reference_store([batch, second], DIM, F.FLAG_ADMISSION, theta=THETA_A)
    stored = set(want1.ext_ids.tolist())
    assert all(int(batch[0][r]) in stored for r in admitted) and not any(int(batch[0][r]) in stored for r in refused)
    assert not stored & set(batch[0][4096:8192].tolist())
    assert n // 16 < want1.ext_ids.size < n // 2 and want1.ext_ids.size + 5 < want2.ext_ids.size < want1.ext_ids.size + 100
    with engine.ApssIndex(DIM, THETA_A, flags=F.FLAG_ADMISSION) as ix:
        ix.insert(*batch)
        assert_store_equal(read_store(ix), want1)
        ix.insert(*second)
        assert_store_equal(read_store(ix), want2)


# ---- case 6: a term shard stores the slice of the row, normalised by the whole row's norm
LO, HI = 700, 1300


def _shard_batch(rng):
    lens = rng.permutation(np.repeat(RAGGED, 3))
    spread = ragged_batch(rng, lens, DIM, scales=10.0 ** rng.uniform(-2, 2, lens.size), first_id=100)
    # rows with nothing in range: drawn over the dim without the range, then shifted past it
    o_ids, o_rp, o_idx, o_val = ragged_batch(rng, [1, 16, 17, 33, 100], DIM - (HI - LO), first_id=300)
    outside = (o_ids, o_rp, np.where(o_idx >= LO, o_idx + (HI - LO), o_idx).astype(np.int32), o_val)
    planted = _rows(400 + np.arange(7), [([LO - 1, LO, HI - 1, HI], [1.0, 2.0, 2.0, 4.0]), ([LO - 1, HI], [3.0, 4.0]), ([LO], [0.5]),
                                          ([HI - 1], [2.0]), ([0, DIM - 1], [1.0, 1.0]), ([LO - 1], [1.0]), ([HI], [1.0])])
    return _concat([spread, outside, planted]), planted[0]


@pytest.mark.parametrize("transform", [False, True])
def test_term_shard_stores_the_slice_of_the_whole_rows_weights(engine, F, transform):
    batch, planted_ids = _shard_batch(np.random.default_rng(606))
    flags, thr = (F.FLAG_NORMALIZE | F.FLAG_VALUE_PRUNE, 0.05) if transform else (0, 0.0)
    assert band_cases([batch], flags, 0.0, thr) == []
    want = reference_store([batch], DIM, flags, index_threshold=thr, term_range=(LO, HI))
    assert want.ext_ids.size == batch[0].size  # rows with nothing in range stay, empty
    assert want.indices.min() == LO and want.indices.max() == HI - 1 and (np.diff(want.rowptr) == 0).sum() >= 5 + 4
    r0 = int(np.nonzero(want.ext_ids == planted_ids[0])[0][0])
    b = want.rowptr[r0]
    assert list(want.indices[b:want.rowptr[r0 + 1]]) == [LO, HI - 1]
    assert np.allclose(want.values[b:b + 2], [0.4, 0.4] if transform else [2.0, 2.0], rtol=1e-15)  # |row| = 5, not the slice's 2.83
    got = _both_paths(engine, [batch], flags=flags, index_threshold=thr, term_range=(LO, HI))
    if transform:
        worst = assert_store_equal(got, want, row_rel_tol(want.src_nnz))
        print("case 6 (term shard, normalise + prune): largest |got - ref| / ref = %.3f * 2^-23" % worst)
    else:
        assert_store_equal(got, want)


# ---- case 7: the packed small message of upload(): (n + 1) * 8 + n * 8 + nnz * 12 <= 262,144 bytes
@pytest.mark.parametrize("nnz", [20511, 20512])
def test_small_message_packing_edge(engine, nnz):
    n = 1000
    assert ((n + 1) * 8 + n * 8 + nnz * 12 <= 262144) == (nnz == 20511)
    rng = np.random.default_rng(707)
    lens = np.full(n, nnz // n)
    lens[:nnz - lens.sum()] += 1
    batch = ragged_batch(rng, lens, DIM, first_id=123, id_step=11)
    assert batch[2].size == nnz
    want = reference_store([batch], DIM)
    assert np.array_equal(want.values, batch[3])
    assert_store_equal(_both_paths(engine, [batch]), want)


# ---- case 8: a store handed to apss_insert_stored_dev comes back bit for bit
def _filtered_batch(rng, F, n_each=4):
    lens = rng.permutation(np.repeat(RAGGED, n_each))
    batch = ragged_batch(rng, lens, DIM, scales=10.0 ** rng.uniform(-2, 2, lens.size), first_id=9000, id_step=13)
    return _with_negatives(batch, range(0, lens.size, 4))


def test_stored_rows_round_trip_unchanged(engine, F):
    flags, theta, thr = F.FLAG_NORMALIZE | F.FLAG_VALUE_PRUNE | F.FLAG_ADMISSION, 0.75, 0.125
    batch = _filtered_batch(np.random.default_rng(808), F)
    assert band_cases([batch], flags, theta, thr) == []
    want = reference_store([batch], DIM, flags, theta=theta, index_threshold=thr)
    kept = np.diff(want.rowptr)
    assert 10 < want.ext_ids.size < batch[0].size - 10 and (kept == 0).any() and ((kept > 0) & (kept < want.src_nnz)).any()
    cfg = dict(flags=flags, index_threshold=thr)
    with engine.ApssIndex(DIM, theta, **cfg) as src:
        src.insert(*batch)
        first = read_store(src)
        assert_store_equal(first, want, row_rel_tol(want.src_nnz))
        rp, idx, val, ext, rows, nnz = store_pointers(src)
        views = (rows, nnz, C.c_void_p(rp), C.c_void_p(idx), C.c_void_p(val), C.c_void_p(ext))
        with engine.ApssIndex(DIM, theta, **cfg) as dst:
            dst._chk(dst._L.apss_insert_stored_dev(dst._h, *views))
            assert_store_equal(read_store(dst), first)
        # the same views as NEW rows: filtered again, a pruned row normalised again changes -- the equality above says something
        with engine.ApssIndex(DIM, theta, **cfg) as again:
            again._chk(again._L.apss_insert_dev(again._h, *views))
            with pytest.raises(AssertionError):
                assert_store_equal(read_store(again), first)


# ---- case 9: the query side of the same filters
def _oracle_filtered(oracle, ids, rp, idx, val, theta, thr):
    """l2_normalize -> admission -> value_prune, as the reference's client, entry proxy and write worker do in turn"""
    nv = oracle.l2_normalize(rp, val)
    keep = oracle.admission(rp, nv, theta)
    prp, pidx, pval = oracle.value_prune(rp, idx, nv, thr)
    sel = np.repeat(keep, np.diff(prp))
    return ids[keep], np.concatenate([[0], np.cumsum(np.diff(prp)[keep])]).astype(np.int64), pidx[sel], pval[sel], keep


def test_query_batch_goes_through_the_same_filters(engine, F, oracle):
    flags, theta, thr, dim = F.FLAG_NORMALIZE | F.FLAG_VALUE_PRUNE | F.FLAG_ADMISSION, 0.75, 0.125, 400
    rng = np.random.default_rng(909)
    lens = rng.permutation(np.repeat([0, 1, 2, 5, 8, 15, 16, 17, 33], 36))
    store = _with_negatives(ragged_batch(rng, lens, dim, scales=rng.uniform(0.5, 4.0, lens.size), low=0.3), range(3, lens.size, 9))
    # queries: noisy copies of stored rows (so that pairs exist), with other ids; every fifth one with negative entries
    pick = rng.choice(lens.size, 250, replace=False)
    qrows = []
    for r in pick:
        b, e = store[1][r], store[1][r + 1]
        qrows.append((store[2][b:e], (np.abs(store[3][b:e]) * rng.uniform(0.9, 1.1, e - b)).astype(np.float32).astype(np.float64)))
    query = _with_negatives(_rows(50_000 + np.arange(pick.size), qrows), range(0, pick.size, 5))
    assert band_cases([store, query], flags, theta, thr) == []
    w = oracle.Worker(dim, theta)
    s_ids, s_rp, s_idx, s_val, _ = _oracle_filtered(oracle, *store, theta, thr)
    w.index_data(s_ids, s_rp, s_idx, s_val, build_only=True)
    q_ids, q_rp, q_idx, q_val, q_keep = _oracle_filtered(oracle, *query, theta, thr)
    want = to_map(*w.index_data(q_ids, q_rp, q_idx, q_val, query_only=True))
    refused = set(query[0][~q_keep].tolist())
    assert len(want) > 100 and 20 < len(refused) < 120
    with engine.ApssIndex(dim, theta, flags=flags, index_threshold=thr) as ix:
        ix.insert(*store)
        ref = reference_store([store], dim, flags, theta, thr)
        assert_store_equal(read_store(ix), ref, row_rel_tol(ref.src_nnz))
        q, c, s = ix.query(*query)
        assert ix.size()[0] == s_ids.size  # a query is not indexed
    assert not refused & set(q.tolist()), "a refused query row reported pairs"
    assert set(q.tolist()) <= set(q_ids.tolist()) and set(c.tolist()) <= set(s_ids.tolist())
    assert_same_pairs(to_map(q, c, s), want, theta)


# ---- case 10: the ingest summary word (non-empty stored rows) in the candidate count
def test_candidate_count_over_the_filtered_store(engine, F):
    import scipy.sparse as sp
    flags, theta, thr, dim, n = F.FLAG_NORMALIZE | F.FLAG_VALUE_PRUNE | F.FLAG_ADMISSION, 0.75, 0.125, 500, 2000
    rng = np.random.default_rng(1010)
    lens = rng.integers(4, 13, n)
    emptied = rng.choice(n, 150, replace=False)
    lens[emptied] = 100  # a hundred near-equal weights: each about 0.1 after normalisation, all below the prune threshold
    batch = ragged_batch(rng, lens, dim, low=0.9)
    short = np.setdiff1d(np.arange(n), emptied)
    ids, rp, idx, val = batch
    val = val.copy()
    for r in short:
        val[rp[r]:rp[r + 1]] = rng.uniform(0.3, 1.0, rp[r + 1] - rp[r]).astype(np.float32)
    batch = _with_negatives((ids, rp, idx, val), short[::10])
    assert band_cases([batch], flags, theta, thr) == []
    want = reference_store([batch], dim, flags, theta, thr)
    kept = np.diff(want.rowptr)
    assert n - short[::10].size <= want.ext_ids.size < n - 100 and (kept == 0).sum() == 150  # refused rows, emptied rows
    B = sp.csr_matrix((np.ones(want.indices.size, np.float32), want.indices, want.rowptr), shape=(want.ext_ids.size, dim))
    truth = (B @ B.T).nnz - int((kept > 0).sum())
    with engine.ApssIndex(dim, theta, flags=flags, index_threshold=thr, head_terms=-1) as ix:
        ix.insert_and_query(*batch)
        st = ix.stats()
        assert_store_equal(read_store(ix), want, row_rel_tol(want.src_nnz))
    assert truth > 100_000 and st["candidate_pairs"] == truth
