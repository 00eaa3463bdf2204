"""apss_query_stored: stored vectors named by external id become the query batch, selected and gathered on the device
(csrc/apss_query_stored.hpp).  The yardstick is the float64 oracle at the project's BAND and TOL (1e-5): the shape of
the removal tests (tests/remove_shape.py) for the paths, the float64 join of tests/store_view.reference_store's rows for the ingest
filters, helpers.scipy_pairs for the hand-built stores.

(The issue asks for the hand-built stores in dim 64 and for selected rows of 65 and 600 terms; a row's terms are distinct and below
dim, so the row-length store alone has dim 1024.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import remove_shape as rs
from apss import _lib
from apss.engine import ApssError, ApssIndex
from helpers import assert_same_pairs, scipy_pairs, to_map
from store_view import band_cases, ragged_batch, read_store, reference_store

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "all-pairs-similarity_amd", "host")
S, DIM, R = rs.STORED, rs.DIM, rs.R
I64 = np.iinfo(np.int64)
NEVER = np.concatenate([-1 - np.arange(20), (1 << 32) + 1 + np.arange(26), [5000, 1 << 40, I64.min, I64.max]]).astype(np.int64)
assert NEVER.size == 50 and not np.isin(NEVER, rs.IDS).any()


def named_list(seed=3):
    """every 3rd id of 0 .. 1999, shuffled, each 10th of them repeated, and the 50 ids that were never stored"""
    rng = np.random.default_rng(seed)
    third = rng.permutation(np.arange(0, S, 3, dtype=np.int64))
    ids = rng.permutation(np.concatenate([third, third[::10], NEVER]))
    return third, ids


def stored_expectation(oracle, theta, zipf, third, marked):
    """the oracle's pairs with q a named live row and c a stored live row"""
    orc = rs.whole_join(oracle, theta, zipf)
    named = np.zeros(rs.N, bool)
    named[third] = True
    dead = rs.IS_R if marked else np.zeros(rs.N, bool)
    visible = named[orc[0]] & ~dead[orc[0]] & (orc[1] < S)
    return rs.split(orc, theta, visible, ~dead[orc[1]])


# ---- 1. every path of a query-type call, with rows marked removed
PATHS = {
    "plain": dict(theta=0.5),
    "exact_accum": dict(theta=0.5, flags=_lib.FLAG_EXACT_ACCUM),
    "force_scan": dict(theta=0.5, flags=_lib.FLAG_FORCE_SCAN),
    "theta_zero": dict(theta=0.0),
    "dense_head": dict(theta=0.5, zipf=1.0, head_terms=64),
    "ids_on_device": dict(theta=0.5, dev=True),
    "no_marks": dict(theta=0.5, marked=False),
}


@pytest.mark.parametrize("path", list(PATHS))
def test_paths(oracle, path):
    p = PATHS[path]
    theta, zipf, marked = p["theta"], p.get("zipf", 0.0), p.get("marked", True)
    third, ids = named_list()
    _, want, dropped, band = stored_expectation(oracle, theta, zipf, third, marked)
    assert len(want) >= 20 and (dropped >= 5 or not marked), (len(want), dropped)
    v = rs.vectors(zipf)
    gone = np.intersect1d(third, R).size if marked else 0
    assert not marked or gone >= 100
    with ApssIndex(DIM, theta, tile_rows=rs.TILE, flags=p.get("flags", 0), head_terms=p.get("head_terms", 0)) as ix:
        ix.insert(rs.IDS[:S], *rs.rows_of(v, 0, S))
        if marked:
            assert ix.remove(R) == R.size
        if p.get("dev"):
            import torch
            got = ix.query_stored(torch.from_numpy(ids).cuda())
        else:
            got = ix.query_stored(ids)
        info, ri, st = ix.stored_query_info(), ix.removal_info(), ix.stats()
        assert ix.size()[0] == S  # nothing was inserted
    print(path, "pairs", len(got[0]), "oracle", len(want), "dropped", ri["pairs_dropped"], dropped, "band", band, info, st["probe_kernel"])
    assert_same_pairs(to_map(*got), want, theta)
    live = np.setdiff1d(third, R) if marked else third
    assert (info["ids_given"], info["ids_distinct"], info["ids_missing"]) == (ids.size, third.size + 50, 50 + gone)
    assert info["rows_selected"] == live.size == third.size - gone
    assert info["nnz_selected"] == int(np.diff(v[0])[live].sum())
    assert info["launches"] == 4 and info["select_ms"] > 0 and info["gather_ms"] > 0
    assert st["symmetric"] == 0 and st["symmetric_declined"] == _lib.SYM_NOT_WHOLE and st["result_pairs"] == len(got[0])
    if marked:
        assert ri["pairs_dropped"] > 0 and abs(ri["pairs_dropped"] - dropped) <= band and ri["drop_launches"] == 1
    else:
        assert ri["drop_launches"] == 0 and ri["pairs_dropped"] == 0
    if path == "dense_head":
        assert st["head_terms"] == 64


# ---- 2. the call takes the path apss_query_dev of the same rows takes: the same list, element by element
def device_list(ix):
    import torch
    n = ix.result_count()
    q, c = torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    s = torch.empty(n, dtype=torch.float32, device="cuda")
    if n:
        ix.results_to(q, c, s)
    torch.cuda.synchronize()
    return q.cpu().numpy(), c.cpu().numpy(), s.cpu().numpy()


@pytest.mark.parametrize("window", [0, 150000])
def test_same_path_as_query_dev(window):
    import torch
    third, ids = named_list(seed=4)
    v = rs.vectors()
    with ApssIndex(DIM, 0.5, tile_rows=rs.TILE, top_k=5, top_k_window=window) as ix:
        ix.insert(rs.IDS[:S], *rs.rows_of(v, 0, S))
        rows, n = ix.query_stored(ids, fetch=False)
        a, a_st, a_wi, a_tk = device_list(ix), ix.stats(), ix.topk_window_info(), ix.topk_info()
        ext_a = ix.fetch()
        store = read_store(ix)
        sel = np.nonzero(np.isin(store.ext_ids, ids))[0]
        assert rows == sel.size == third.size and n == len(a[0]) > 50
        lens = np.diff(store.rowptr)[sel]
        rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        take = np.concatenate([np.arange(store.rowptr[r], store.rowptr[r + 1]) for r in sel])
        dev = [torch.from_numpy(x).cuda() for x in (store.ext_ids[sel], rp, store.indices[take], store.values[take])]
        assert ix.query_dev(*dev) == n
        b, b_st, b_wi, b_tk = device_list(ix), ix.stats(), ix.topk_window_info(), ix.topk_info()
        ext_b = ix.fetch()
    for x, y in zip(a[:2] + ext_a[:2], b[:2] + ext_b[:2]):
        assert np.array_equal(x, y)
    assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    assert a_st["probe_kernel"] == b_st["probe_kernel"] != ""
    for key in ("posting_visits", "candidate_pairs", "filter_survivors", "probe_launches", "result_pairs", "query_chunk", "filter_tile_rows"):
        assert a_st[key] == b_st[key], key
    assert a_wi["windows"] == b_wi["windows"] and (a_wi["windows"] >= 3 if window else a_wi["windows"] == 0)
    assert a_tk["pairs_over_theta"] == b_tk["pairs_over_theta"] and a_tk["k"] == 5
    assert np.all(np.diff(a[0]) >= 0) and a[0].max() < rows  # grouped by the row within the batch


# ---- 3. the stored rows are not filtered twice
def filtered_batch():
    """rows of 5 .. 220 terms in dim 512, each followed by a copy scaled by 1/2 under another id (its normalised twin: their score
    is the squared mass the prune left), one row whose pruned sum falls below theta"""
    rng = np.random.default_rng(11)
    lengths = [5, 16, 33, 64, 100, 130, 150, 160, 220, 200]
    ids, rp, idx, val = ragged_batch(rng, lengths, 512)
    b, e = rp[9], rp[10]  # the last row: one heavy entry among light ones, which the prune takes
    val[b:e] = (0.05 + 0.1 * rng.random(e - b)).astype(np.float32).astype(np.float64)
    val[b + 7] = 0.75
    rows = []
    for r in range(len(lengths)):
        rows += [(2 * r, idx[rp[r]:rp[r + 1]], val[rp[r]:rp[r + 1]]), (2 * r + 1, idx[rp[r]:rp[r + 1]], 0.5 * val[rp[r]:rp[r + 1]])]
    return (np.array([r[0] for r in rows], np.int64), np.concatenate([[0], np.cumsum([r[1].size for r in rows])]).astype(np.int64),
            np.concatenate([r[1] for r in rows]).astype(np.int32), np.concatenate([r[2] for r in rows]))


def test_not_filtered_twice():
    theta, thr, dim = 0.5, 0.1, 512
    flags = _lib.FLAG_NORMALIZE | _lib.FLAG_VALUE_PRUNE | _lib.FLAG_ADMISSION
    batch = filtered_batch()
    assert band_cases([batch], flags, theta, thr) == []
    ref = reference_store([batch], dim, flags, theta, thr)
    assert ref.ext_ids.size == batch[0].size  # every row was admitted on its unpruned sum
    named = ref.ext_ids[::2].copy()
    by_row = scipy_pairs(dim, theta, ref.rowptr, ref.indices, ref.values)
    want = {(int(ref.ext_ids[i]), int(ref.ext_ids[j])): s for (i, j), s in by_row.items() if ref.ext_ids[i] in named}
    assert len(want) >= 5
    # the two statements the test stands on, for this seed: (a) re-normalising the stored rows moves the scores by far more than
    # 1e-5 and the prune took a third of some row's mass; (b) a stored row's pruned sum is below theta: re-admission would lose it
    mass = np.array([float(np.sum(ref.values[b:e] ** 2)) for b, e in zip(ref.rowptr[:-1], ref.rowptr[1:])])
    sums = np.array([float(np.sum(ref.values[b:e])) for b, e in zip(ref.rowptr[:-1], ref.rowptr[1:])])
    in_pairs = np.unique([i for (i, _) in by_row])
    assert (mass[in_pairs] <= 2.0 / 3.0).any()
    renorm = {k: s / np.sqrt(mass[i] * mass[j]) for (i, j), s in by_row.items() for k in [(int(ref.ext_ids[i]), int(ref.ext_ids[j]))] if k in want}
    assert sum(abs(renorm[k] - want[k]) > 1e-3 for k in want) >= 4  # (short rows lose nothing to the prune)
    low = np.nonzero((sums < theta) & (np.diff(ref.rowptr) > 0))[0]
    assert low.size >= 1 and np.isin(ref.ext_ids[low], named).any()
    with ApssIndex(dim, theta, flags=flags, index_threshold=thr) as ix:
        ix.insert(*batch)
        rows, n = ix.query_stored(named, fetch=False)
        got = ix.fetch()
        info = ix.stored_query_info()
    assert rows == named.size == info["rows_selected"] and info["ids_missing"] == 0  # the low row is a row of the batch
    assert info["nnz_selected"] == int(np.diff(ref.rowptr)[::2].sum())
    assert n == len(got[0])
    assert_same_pairs(to_map(*got), want, theta)


# ---- 4. the smallest shapes: hand-built stores, dyadic values, float64 expectation by row
class Model:
    """the store as the test knows it: rows (id, terms, weights) in slot order and their marks"""

    def __init__(self, ix, dim, theta):
        self.ix, self.dim, self.theta = ix, dim, theta
        self.rows, self.dead = [], []

    @staticmethod
    def csr(rows):
        rp = np.concatenate([[0], np.cumsum([len(r[1]) for r in rows])]).astype(np.int64)
        idx = np.concatenate([np.asarray(r[1], np.int32) for r in rows] + [np.zeros(0, np.int32)]).astype(np.int32)
        val = np.concatenate([np.asarray(r[2], np.float64) for r in rows] + [np.zeros(0)])
        return np.array([r[0] for r in rows], np.int64), rp, idx, val

    def insert(self, rows):
        self.ix.insert(*self.csr(rows))
        self.rows += rows
        self.dead += [False] * len(rows)

    def remove(self, ids):
        newly = sum(1 for r, d in zip(self.rows, self.dead) if r[0] in ids and not d)
        assert self.ix.remove(list(ids)) == newly
        self.dead = [d or r[0] in ids for r, d in zip(self.rows, self.dead)]

    def expect(self, queries, stored):
        """sorted (q id, c id, score) of the float64 join of `queries` (stored rows by slot, or outside rows) against the live store"""
        qs = [self.rows[q] for q in queries] if stored else queries
        if not qs:
            return []
        _, rp, idx, val = self.csr(self.rows + qs)
        n = len(self.rows)
        out = []
        for (i, j), s in scipy_pairs(self.dim, self.theta, rp, idx, val).items():
            if i >= n and j < n and not self.dead[j] and qs[i - n][0] != self.rows[j][0]:
                out.append((qs[i - n][0], self.rows[j][0], s))
        return sorted(out)

    def check(self, got, want):
        got = sorted(zip(got[0].tolist(), got[1].tolist(), got[2].tolist()))
        assert [g[:2] for g in got] == [w[:2] for w in want], (got, want)
        assert all(abs(g[2] - w[2]) <= 1e-5 for g, w in zip(got, want))

    def query_stored(self, ids, rows_expected):
        """the named live rows' pairs; then a plain query on the same handle still answers right"""
        slots = [s for s, (r, d) in enumerate(zip(self.rows, self.dead)) if r[0] in ids and not d]
        assert len(slots) == rows_expected
        rows, n = self.ix.query_stored(ids, fetch=False)
        assert rows == rows_expected == self.ix.stored_query_info()["rows_selected"]
        assert self.ix.result_count() == n
        want = self.expect(slots, True)
        self.check(self.ix.fetch(), want)
        if self.rows:
            outside = [(9000 + k, r[1], r[2]) for k, r in enumerate(self.rows[:3]) if len(r[1])]
            if outside:
                self.check(self.ix.query(*self.csr(outside)), self.expect(outside, False))
        return want


def row(i, terms, weight):
    return (i, sorted(terms), [weight] * len(terms))


def test_smallest_stores():
    dim, theta = 64, 0.25
    # one row; the only id named twice
    with ApssIndex(dim, theta) as ix:
        m = Model(ix, dim, theta)
        m.insert([row(7, [1, 2, 3], 0.5)])
        assert m.query_stored([7, 7], 1) == []
        info = ix.stored_query_info()
        assert (info["ids_given"], info["ids_distinct"], info["ids_missing"], info["nnz_selected"]) == (2, 1, 0, 3)
        assert m.query_stored([8], 0) == [] and ix.stored_query_info()["ids_missing"] == 1
    # three rows (the odd tail of the 16-B id loads): the last one named, then all of them
    with ApssIndex(dim, theta) as ix:
        m = Model(ix, dim, theta)
        m.insert([row(1, [1, 2, 3, 4], 0.5), row(2, [3, 4, 5, 6], 0.5), row(3, [1, 2, 3, 4], 0.25)])
        assert len(m.query_stored([3], 1)) == 2
        assert len(m.query_stored([3, 1, 2], 3)) == 6
        assert ix.stats()["symmetric"] == 0  # every stored id named: still no symmetric join
    # two live rows under one id: both selected, never paired with each other.  Then marked twins (a removal takes every row of
    # the id; the mark is the slot's) and a third row stored under the id afterwards: only that one is selected
    with ApssIndex(dim, theta) as ix:
        m = Model(ix, dim, theta)
        m.insert([row(5, [1, 2, 3, 4], 0.5), row(6, [1, 2, 3, 4], 0.5), row(5, [1, 2, 3, 4], 0.25), row(9, [1, 2, 3, 4], 0.5), row(10, [], 0.5)])
        want = m.query_stored([5], 2)
        assert len(want) == 4 and all(c != 5 for _, c, _ in want)
        m.remove({5})
        assert m.query_stored([5], 0) == [] and ix.stored_query_info()["ids_missing"] == 1
        m.insert([row(5, [1, 2, 3, 4], 0.5)])
        want = m.query_stored([5], 1)
        assert len(want) == 2 and ix.stored_query_info()["ids_missing"] == 0
        # a selected row with zero entries: a row of the batch with no pairs
        assert m.query_stored([10], 1) == [] and ix.stored_query_info()["nnz_selected"] == 0
        assert len(m.query_stored([10, 6], 2)) == 2


def test_row_lengths_and_waiting_rows():
    dim, theta = 1024, 0.25
    rng = np.random.default_rng(2)
    rows = []
    for k, (length, w) in enumerate([(1, 1.0), (63, 0.125), (64, 0.125), (65, 0.125), (600, 1.0 / 32)]):
        terms = rng.choice(dim, length, replace=False).tolist()
        rows += [row(100 + k, terms, w), row(200 + k, terms, w)]  # a selected row and its copy under another id
    rows += [row(300 + k, rng.choice(dim, 40, replace=False).tolist(), 0.125) for k in range(30)]
    with ApssIndex(dim, theta) as ix:
        m = Model(ix, dim, theta)
        m.insert(rows)
        want = m.query_stored([100, 101, 102, 103, 104], 5)
        assert {(q, c) for q, c, _ in want} >= {(100 + k, 200 + k) for k in range(5)}
        assert ix.stored_query_info()["nnz_selected"] == 1 + 63 + 64 + 65 + 600
        assert len(m.query_stored([104], 1)) >= 1  # the row of 600 terms alone: virtual rows
        # a selected row and its only partner both still waiting outside the tile index
        lone = rng.choice(np.arange(900, 1024), 20, replace=False).tolist()
        m.insert([row(400, lone, 0.25), row(401, lone, 0.25)] + [row(402 + k, [k], 0.125) for k in range(3)])
        assert [(q, c) for q, c, _ in m.query_stored([400], 1)] == [(400, 401)]
        assert len(m.query_stored([401, 100], 2)) >= 2


def test_nothing_to_ask():
    v = rs.vectors()
    with ApssIndex(DIM, 0.5, tile_rows=rs.TILE) as ix:
        for ids in ([], [1, 2, 3]):  # an empty handle
            assert ix.query_stored(ids, fetch=False) == (0, 0) and ix.result_count() == 0
            assert ix.stored_query_info()["ids_missing"] == len(ids) and ix.stored_query_info()["rows_selected"] == 0
        ix.insert(rs.IDS[:600], *rs.rows_of(v, 0, 600))
        for ids in ([], NEVER):  # n = 0; nothing found
            assert ix.query_stored(ids, fetch=False) == (0, 0) and ix.result_count() == 0
            assert all(a.size == 0 for a in ix.fetch())
            info = ix.stored_query_info()
            assert (info["ids_given"], info["ids_missing"], info["rows_selected"]) == (len(ids), len(ids), 0)
        got = ix.query(rs.IDS[600:700], *rs.rows_of(v, 600, 700))  # the staging is in order
        assert len(got[0]) > 0
        again = ix.query_stored(rs.IDS[:600])
        assert len(again[0]) > 0 and ix.stored_query_info()["rows_selected"] == 600


# ---- 5. refusals and state
def test_refusals_and_state(oracle):
    import torch
    v = rs.vectors()
    theta = 0.5
    with ApssIndex(DIM, theta, tile_rows=rs.TILE, term_range=(0, DIM // 2)) as shard:
        shard.insert(rs.IDS[:500], *rs.rows_of(v, 0, 500))
        for call in (lambda: shard.query_stored([1]), lambda: shard.query_stored(torch.zeros(1, dtype=torch.int64, device="cuda"))):
            with pytest.raises(ApssError) as e:
                call()
            assert e.value.code == _lib.E_UNSUPPORTED and "term shard" in str(e.value)
        assert shard.self_join(fetch=False) >= 0  # the handle works afterwards
    with ApssIndex(DIM, theta, tile_rows=rs.TILE) as ix:
        ix.insert(rs.IDS[:S], *rs.rows_of(v, 0, S))
        one = np.zeros(1, np.int64)
        rows, n = C.c_int64(7), C.c_int64(7)
        L, h = ix._L, ix._h
        assert L.apss_query_stored(h, -1, C.c_void_p(one.ctypes.data), C.byref(rows), C.byref(n)) == _lib.E_INVALID
        assert L.apss_query_stored(h, 1, None, None, None) == _lib.E_INVALID
        assert L.apss_query_stored(h, 1 << 31, C.c_void_p(one.ctypes.data), None, None) == _lib.E_INVALID
        assert L.apss_query_stored_dev(h, -1, None, None, None) == _lib.E_INVALID
        assert L.apss_query_stored_dev(h, 1, None, None, None) == _lib.E_INVALID
        assert L.apss_query_stored(h, 1, C.c_void_p(one.ctypes.data), None, None) == _lib.OK  # NULL counts
        assert ix.result_count() >= 0
        # after an insert the results are gone; the call is a query-type call: they answer again
        ix.insert(rs.IDS[S:S + 5], *rs.rows_of(v, S, S + 5))
        with pytest.raises(ApssError) as e:
            ix.result_count()
        assert e.value.code == _lib.E_STATE
        ix.query_stored([0, 1, 2])
        assert ix.result_count() >= 0
    # every stored id named: no symmetric join; a compaction changes nothing by external id
    third, _ = named_list()
    _, want, _, _ = stored_expectation(oracle, theta, 0.0, third, True)
    with ApssIndex(DIM, theta, tile_rows=rs.TILE) as ix:
        ix.insert(rs.IDS[:S], *rs.rows_of(v, 0, S))
        everything = ix.query_stored(rs.IDS[:S])
        st = ix.stats()
        assert st["symmetric"] == 0 and st["symmetric_declined"] == _lib.SYM_NOT_WHOLE and len(everything[0]) > 100
        assert ix.remove(R) == R.size
        before = ix.query_stored(third)
        ix.compact()
        with pytest.raises(ApssError) as e:
            ix.result_count()
        assert e.value.code == _lib.E_STATE
        after = ix.query_stored(third)
        assert ix.removal_info()["drop_launches"] == 0 and ix.size()[0] == S - R.size
    assert_same_pairs(to_map(*before), want, theta)
    assert_same_pairs(to_map(*after), want, theta)
    assert set(to_map(*before)) == set(to_map(*after))


# ---- 6. the host mirror
def test_host_mirror_query_stored():
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(HOST, "host_query_stored_selftest")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "host_query_stored_selftest: PASS" in out.stdout
