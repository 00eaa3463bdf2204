"""GPU tests of the T x D grids behind the C ABI (apss_group_create_grid, include/apss.h "GRIDS"): T term ranges x D row
ranges of member shards, the exchange inside each row range, a row range's own span joined with itself and the other spans
met as ONE outside batch, the symmetry across row ranges on a whole-store join.  All members share device 0 (the copies
exchange), at most 12 members per test.  The answer of every call is the list one plain handle gives.
Reference: WriteWorkerActor.scala:164-183 (dim % maxShardNum) + EntryProxyActor.scala:37-49 (dim % maxIndexEntryActorNum)."""
import numpy as np
import pytest

from apss import _lib, synth
from helpers import assert_same_pairs, to_map

pytestmark = pytest.mark.gpu


def _grid(dim, theta, T, D, **kw):
    from apss.engine import ApssGroup
    return ApssGroup(dim, theta, [0] * (T * D), row_ranges=D, **kw)


def _spans(n, D):
    """span k of a batch of n rows: [ceil(n k / D), ceil(n (k + 1) / D))"""
    return [(-(-n * k // D), -(-n * (k + 1) // D)) for k in range(D)]


def _rows_after(sizes, D):
    """rows per row range after batches of these sizes, by the rule of include/apss.h: span k goes to row range
    (first + k) mod D, first = the range holding the fewest rows (lowest index on ties)"""
    rows = [0] * D
    for n in sizes:
        first = rows.index(min(rows))
        for k, (lo, hi) in enumerate(_spans(n, D)):
            rows[(first + k) % D] += hi - lo
    return rows


def _batch(rp, idx, val, ids, b0, b1):
    sl = slice(rp[b0], rp[b1])
    return ids[b0:b1], rp[b0:b1 + 1] - rp[b0], idx[sl], val[sl]


GRID_CASES = [(1, 2, 0.0, 0.5, -1), (2, 2, 1.0, 0.6, 64), (1, 3, 1.0, 0.55, -1), (2, 3, 0.0, 0.5, -1), (4, 2, 0.0, 0.8, -1),
              (1, 4, 1.0, 0.5, -1), (2, 4, 0.0, 0.6, 700)]


def _grid_input(T, D, zipf):
    n, dim, nnz = 4000, 2000, 30
    rp, idx, val = synth.make_vectors(n, dim, nnz, zipf, seed=100 + 10 * T + D, dup_frac=0.1)
    ids = np.arange(n, dtype=np.int64) * 3 + 1000
    return n, dim, rp, idx, val, ids


@pytest.mark.parametrize("T,D,zipf,theta,head", GRID_CASES)
def test_grid_equals_the_oracle(oracle, T, D, zipf, theta, head):
    """a whole-store join through a T x D grid: the oracle's pairs (many of them across two spans), the symmetry across the
    row ranges used, rows spread by the span rule, the statistics add up, posting visits = sum df^2 without a head"""
    n, dim, rp, idx, val, ids = _grid_input(T, D, zipf)
    oq, oc, os_ = oracle.selfjoin_pairs(dim, theta, rp, idx, val)
    want = to_map(ids[oq], ids[oc], os_)
    spans = _spans(n, D)
    span_of = np.searchsorted([hi for _, hi in spans], np.arange(n), side="right")
    cross = int((span_of[oq] != span_of[oc]).sum())
    print("T=%d D=%d: %d pairs, %d across spans" % (T, D, len(want), cross))
    assert len(want) > 500 and cross > 200
    with _grid(dim, theta, T, D, head_terms=head, tile_rows=1024) as g:
        got = to_map(*g.insert_and_query(ids, rp, idx, val))
        st, gr = g.stats(), g.grid()
        assert_same_pairs(got, want, theta)
        assert gr["n_term_ranges"] == T and gr["n_row_ranges"] == D
        assert gr["symmetric_ranges"] == 1 and gr["mirrored_pairs"] > 0
        assert gr["rows_in_range"] == [hi - lo for lo, hi in spans]
        assert 0 < gr["outside_rows_max"] < n and gr["own_ms_max"] > 0 and gr["outside_ms_max"] > 0
        assert st["n_members"] == T * D and st["rows"] == n and st["result_pairs"] == len(got) == g.result_count()
        assert st["exchange"] == (_lib.EXCHANGE_COPIES if T > 1 else _lib.EXCHANGE_NONE)
        cuts = st["term_cuts"]
        assert len(cuts) == T + 1 and cuts[0] == 0 and cuts[-1] == dim and all(a < b for a, b in zip(cuts[:-1], cuts[1:]))
        assert st["head_terms"] == (0 if head <= 0 else min(head, dim))
        ms = [g.member_stats(m) for m in range(T * D)]
        assert sum(m["nnz"] for m in ms) == st["nnz"]
        assert [m["rows"] for m in ms] == [spans[m // T][1] - spans[m // T][0] for m in range(T * D)]
        if st["head_terms"] == 0:
            df = np.bincount(idx, minlength=dim).astype(np.int64)
            print("posting visits %d (device %d), sum df^2 %d" % (st["posting_visits"], st["device_posting_visits"], int((df ** 2).sum())))
            assert st["posting_visits"] == int((df ** 2).sum())
            assert st["device_posting_visits"] < st["posting_visits"]
        # the result list pages with the offset / count contract, across the row ranges' lists
        q = np.zeros(len(got), np.int64); c = np.zeros(len(got), np.int64); s = np.zeros(len(got), np.float32)
        step = 97
        for off in range(0, len(got), step):
            k = min(step, len(got) - off)
            g._chk(g._L.apss_group_fetch_results(g._g, off, k, q[off:].ctypes.data, c[off:].ctypes.data, s[off:].ctypes.data))
        assert to_map(q, c, s) == got
        g.clear()
        assert g.stats()["term_cuts"] == cuts and g.grid()["rows_in_range"] == [0] * D
        again = to_map(*g.insert_and_query(ids, rp, idx, val))
        assert again.keys() == got.keys() and g.stats()["term_cuts"] == cuts


@pytest.mark.parametrize("T,D,zipf,theta,head", [c for c in GRID_CASES if (c[0], c[1]) in ((2, 3), (1, 4))])
def test_grid_without_symmetric_ranges(oracle, T, D, zipf, theta, head):
    """APSS_GROUP_NO_SYMMETRIC_RANGES: every cell meets every other span, nothing is mirrored; the same pairs, more device work"""
    n, dim, rp, idx, val, ids = _grid_input(T, D, zipf)
    oq, oc, os_ = oracle.selfjoin_pairs(dim, theta, rp, idx, val)
    want = to_map(ids[oq], ids[oc], os_)
    with _grid(dim, theta, T, D, head_terms=head, tile_rows=1024) as g:
        sym = to_map(*g.insert_and_query(ids, rp, idx, val))
        sym_visits = g.stats()["device_posting_visits"]
        assert g.grid()["symmetric_ranges"] == 1
    with _grid(dim, theta, T, D, head_terms=head, tile_rows=1024, group_flags=_lib.GROUP_NO_SYMMETRIC_RANGES) as g:
        got = to_map(*g.insert_and_query(ids, rp, idx, val))
        st, gr = g.stats(), g.grid()
    assert_same_pairs(got, want, theta)
    assert_same_pairs(sym, want, theta)
    assert gr["symmetric_ranges"] == 0 and gr["mirrored_pairs"] == 0
    assert gr["outside_rows_max"] == n - min(hi - lo for lo, hi in _spans(n, D))
    print("device posting visits: %d without the symmetry across ranges, %d with" % (st["device_posting_visits"], sym_visits))
    assert st["device_posting_visits"] > sym_visits
    df = np.bincount(idx, minlength=dim).astype(np.int64)
    assert st["posting_visits"] == int((df ** 2).sum())  # nothing counted twice, every (query, posting) visited once


STREAM = [1, 1, 2, 5, 1, 64, 333, 1000, 1, 4592]


@pytest.mark.parametrize("T,D", [(2, 2), (1, 3), (3, 2)])
def test_grid_streams_equal_a_plain_handle_call_by_call(oracle, T, D):
    """batches shorter than D, not divisible by D, onto a non-empty store: every call's answer is the plain handle's, the last
    one also the oracle worker's replay of the stream; the rows land where the span rule puts them"""
    from apss.engine import ApssIndex
    n, dim, nnz, theta = 6000, 2500, 25, 0.5
    assert sum(STREAM) == n
    rp, idx, val = synth.make_vectors(n, dim, nnz, 0.5, seed=40 + T + D, dup_frac=0.15)
    ids = np.arange(n, dtype=np.int64) * 2 + 5
    w = oracle.Worker(dim, theta)
    with _grid(dim, theta, T, D, head_terms=-1, tile_rows=1024) as g, ApssIndex(dim, theta, tile_rows=1024) as ix:
        b0 = 0
        total = 0
        for k, sz in enumerate(STREAM):
            args = _batch(rp, idx, val, ids, b0, b0 + sz)
            ref = to_map(*ix.insert_and_query(*args))
            got = to_map(*g.insert_and_query(*args))
            want = to_map(*w.index_data(*args))
            assert_same_pairs(got, ref, theta, band=2e-5, tol=5e-6)
            assert g.grid()["symmetric_ranges"] == (1 if k == 0 else 0)
            total += len(got)
            b0 += sz
        assert_same_pairs(got, want, theta, band=2e-5, tol=2e-5)
        assert total > 500 and len(got) > 300
        rows = g.grid()["rows_in_range"]
        expect = _rows_after(STREAM, D)
        assert rows == expect and sum(rows) == n == g.stats()["rows"]
        assert max(rows) - min(rows) == max(expect) - min(expect)


def test_grid_single_vectors_fill_the_ranges_round_robin(oracle):
    """300 calls of one vector each on D = 3: exactly 100 rows per range, and the stream's pairs are the oracle worker's"""
    n, dim, nnz, theta, T, D = 300, 400, 12, 0.4, 2, 3
    rp, idx, val = synth.make_vectors(n, dim, nnz, 0.5, seed=9, dup_frac=0.3)
    ids = np.arange(n, dtype=np.int64) + 11
    w = oracle.Worker(dim, theta)
    got, want = {}, {}
    with _grid(dim, theta, T, D, head_terms=-1) as g:
        for r in range(n):
            args = _batch(rp, idx, val, ids, r, r + 1)
            got.update(to_map(*g.insert_and_query(*args)))
            want.update(to_map(*w.index_data(*args)))
        assert g.grid()["rows_in_range"] == [100, 100, 100]
    assert len(want) > 50
    assert_same_pairs(got, want, theta, band=2e-5, tol=2e-5)


@pytest.mark.parametrize("T,D", [(2, 2), (1, 3)])
def test_grid_frozen_query_equals_a_plain_handle(T, D):
    """a query batch against the frozen index: every row range is asked the whole batch, the lists are concatenated"""
    from apss.engine import ApssIndex
    n, nq, dim, nnz, theta = 4000, 500, 2000, 30, 0.5
    rp, idx, val = synth.make_vectors(n + nq, dim, nnz, 0.5, seed=60 + D, dup_frac=0.0)
    ids = np.arange(n + nq, dtype=np.int64) + 100
    store = _batch(rp, idx, val, ids, 0, n)
    qids, qrp, qidx, qval = _batch(rp, idx, val, ids, n, n + nq)
    qidx, qval = qidx.copy(), qval.copy()
    rng = np.random.default_rng(3)
    for r in range(0, nq, 3):  # every third query row is a near-duplicate of a stored row of the same length
        src = int(rng.integers(0, n))
        ln = qrp[r + 1] - qrp[r]
        if rp[src + 1] - rp[src] == ln:
            qidx[qrp[r]:qrp[r + 1]] = idx[rp[src]:rp[src + 1]]
            qval[qrp[r]:qrp[r + 1]] = val[rp[src]:rp[src + 1]] * (1.0 + 0.05 * rng.random(ln))
    with ApssIndex(dim, theta, tile_rows=1024) as ix:
        ix.insert(*store)
        ref = to_map(*ix.query(qids, qrp, qidx, qval))
    assert len(ref) > 100
    with _grid(dim, theta, T, D, head_terms=-1, tile_rows=1024) as g:
        g.insert(*store)
        got = to_map(*g.query(qids, qrp, qidx, qval))
        assert g.stats()["rows"] == n and g.grid()["symmetric_ranges"] == 0
        assert_same_pairs(got, ref, theta, band=2e-5, tol=5e-6)
        again = to_map(*g.query(qids, qrp, qidx, qval))
        assert again.keys() == got.keys()


@pytest.mark.parametrize("T,D", [(2, 2), (1, 4)])
def test_grid_device_entry_equals_the_host_entry(T, D):
    """the batch resident in HBM, handed whole to every member: the spans and the outside batches are cut on the device; the
    same lists as the host-pointer calls, for a whole-store join and for a second batch onto the store"""
    import torch
    n, dim, nnz, theta = 5001, 3000, 30, 0.55
    rp, idx, val = synth.make_vectors(n, dim, nnz, 0.5, seed=70 + T, dup_frac=0.15)
    ids = np.arange(n, dtype=np.int64) * 5 + 3
    dev = torch.device("cuda", 0)
    cut = 3002
    batches = [_batch(rp, idx, val, ids, 0, cut), _batch(rp, idx, val, ids, cut, n)]
    with _grid(dim, theta, T, D, head_terms=-1, tile_rows=1024) as gh, _grid(dim, theta, T, D, head_terms=-1, tile_rows=1024) as gd:
        for bi, brp, bidx, bval in batches:
            want = to_map(*gh.insert_and_query(bi, brp, bidx, bval))
            d = (torch.from_numpy(np.ascontiguousarray(bi)).to(dev), torch.from_numpy(np.ascontiguousarray(brp)).to(dev),
                 torch.from_numpy(np.ascontiguousarray(bidx)).to(dev), torch.from_numpy(bval.astype(np.float32)).to(dev))
            torch.cuda.synchronize()
            n_res = gd.insert_and_query_dev([d] * (T * D))
            got = to_map(*gd.fetch())
            assert n_res == len(got) and len(want) > 100
            assert_same_pairs(got, want, theta, band=2e-5, tol=5e-6)
            assert gd.grid()["rows_in_range"] == gh.grid()["rows_in_range"]
            assert gd.stats()["posting_visits"] == gh.stats()["posting_visits"]
            assert gd.stats()["term_cuts"] == gh.stats()["term_cuts"]


def _group_by_apss_group_create(dim, theta, T, head):
    """an ApssGroup whose object comes from apss_group_create itself (the Python class always calls apss_group_create_grid)"""
    import ctypes as C
    from apss.engine import ApssError, ApssGroup
    L = _lib.lib()
    cfg = _lib.Config()
    cfg.struct_size = C.sizeof(_lib.Config)
    cfg.dim, cfg.theta, cfg.head_terms = dim, theta, head
    devs = np.zeros(T, np.int32)
    h = C.c_void_p()
    rc = L.apss_group_create(C.byref(cfg), T, devs.ctypes.data, 0, C.byref(h))
    if rc != _lib.OK:
        raise ApssError(rc, (L.apss_group_last_error(None) or b"").decode())
    g = ApssGroup.__new__(ApssGroup)
    g._g, g._L, g.dim, g.theta = h, L, dim, theta
    g.n_members, g.term_ranges, g.row_ranges = T, T, 1
    return g


def test_one_row_range_is_the_group_it_was(oracle):
    """row_ranges = 1 through apss_group_create_grid and apss_group_create: the same statistics fields, cuts and pairs"""
    from apss.engine import ApssGroup
    n, dim, nnz, theta, T = 4000, 2000, 30, 0.55, 3
    rp, idx, val = synth.make_vectors(n, dim, nnz, 1.0, seed=23, dup_frac=0.1)
    ids = np.arange(n, dtype=np.int64) + 50
    oq, oc, os_ = oracle.selfjoin_pairs(dim, theta, rp, idx, val)
    want = to_map(ids[oq], ids[oc], os_)
    with ApssGroup(dim, theta, [0] * T, head_terms=64, row_ranges=1) as g:
        got = to_map(*g.insert_and_query(ids, rp, idx, val))
        st, gr = g.stats(), g.grid()
    with _group_by_apss_group_create(dim, theta, T, 64) as old:
        ref = to_map(*old.insert_and_query(ids, rp, idx, val))
        st_old, gr_old = old.stats(), old.grid()
    assert len(want) > 100
    assert_same_pairs(got, want, theta)
    assert got.keys() == ref.keys() and max(abs(got[k] - ref[k]) for k in got) == 0.0
    assert st.keys() == st_old.keys()
    for k in ("n_members", "exchange", "head_terms", "rows", "nnz", "posting_visits", "device_posting_visits", "member_touched_pairs",
              "candidates_sum", "candidates_max", "union_pairs", "result_pairs", "all_gather_bytes", "all_reduce_bytes", "term_cuts"):
        assert st[k] == st_old[k], k
    assert st["n_members"] == T and len(st["term_cuts"]) == T + 1 and st["head_terms"] == 64
    for x in (gr, gr_old):
        assert x["n_term_ranges"] == T and x["n_row_ranges"] == 1 and x["rows_in_range"] == [n]
        assert x["symmetric_ranges"] == 0 and x["mirrored_pairs"] == 0 and x["outside_rows_max"] == 0


@pytest.mark.parametrize("T,D", [(4, 2), (2, 4)])
def test_grid_c3_uniform_200k(T, D):
    """BASELINE.json configs[3]'s shape (dim 100k, nnz 100, uniform, theta 0.8) at N = 200k through grids of eight members: one
    plain handle's list"""
    from apss.engine import ApssIndex
    n, dim, nnz, theta = 200_000, 100_000, 100, 0.8
    rp, idx, val = synth.make_vectors(n, dim, nnz, 0.0, seed=synth.CONFIGS["c3"]["seed"])
    ids = np.arange(n, dtype=np.int64)
    with ApssIndex(dim, theta) as ix:
        ref = to_map(*ix.insert_and_query(ids, rp, idx, val))
    with _grid(dim, theta, T, D) as g:
        got = to_map(*g.insert_and_query(ids, rp, idx, val))
        st, gr = g.stats(), g.grid()
    assert len(ref) > 1000
    assert_same_pairs(got, ref, theta, band=2e-5, tol=5e-6)
    assert st["head_terms"] == 0 and st["posting_visits"] == int(synth.workload_counts(dim, rp, idx)[1])
    assert gr["symmetric_ranges"] == 1 and gr["rows_in_range"] == [n // D] * D


def test_grid_refusals(oracle):
    """shapes that do not fit are APSS_E_INVALID; re-layout of a grid is not built yet: APSS_GROUP_ADAPT_LAYOUT is refused at
    create and apss_group_relayout on a grid answers APSS_E_UNSUPPORTED and leaves the group working"""
    from apss.engine import ApssError, ApssGroup
    dim, theta = 2000, 0.5
    for T, D in ((13, 5), (65, 1), (1, 65)):
        with pytest.raises(ApssError) as e:
            ApssGroup(dim, theta, [0] * (T * D), row_ranges=D)
        assert e.value.code == _lib.E_INVALID
    for D in (0, -1):
        with pytest.raises(ApssError) as e:
            ApssGroup(dim, theta, [], row_ranges=D)
        assert e.value.code == _lib.E_INVALID
    with pytest.raises(ApssError) as e:
        ApssGroup(dim, theta, [], row_ranges=2)  # no term range
    assert e.value.code == _lib.E_INVALID
    with pytest.raises(ApssError) as e:
        ApssGroup(dim, theta, [0] * 4, row_ranges=2, group_flags=_lib.GROUP_ADAPT_LAYOUT)
    assert e.value.code == _lib.E_UNSUPPORTED
    n, nnz = 3000, 30
    rp, idx, val = synth.make_vectors(n, dim, nnz, 0.0, seed=8, dup_frac=0.1)
    ids = np.arange(n, dtype=np.int64)
    w = oracle.Worker(dim, theta)
    with _grid(dim, theta, 2, 2, head_terms=-1) as g:
        first = _batch(rp, idx, val, ids, 0, 2000)
        want = to_map(*w.index_data(*first))
        assert_same_pairs(to_map(*g.insert_and_query(*first)), want, theta, band=2e-5, tol=2e-5)
        cuts = g.stats()["term_cuts"]
        for arg in (None, [0, 1000, dim]):
            with pytest.raises(ApssError) as e:
                g.relayout(arg)
            assert e.value.code == _lib.E_UNSUPPORTED
        second = _batch(rp, idx, val, ids, 2000, n)
        want = to_map(*w.index_data(*second))
        assert len(want) > 50
        assert_same_pairs(to_map(*g.insert_and_query(*second)), want, theta, band=2e-5, tol=2e-5)
        assert g.stats()["term_cuts"] == cuts and g.grid()["rows_in_range"] == [1500, 1500]

