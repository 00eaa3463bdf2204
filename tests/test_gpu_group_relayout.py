"""GPU tests of the group's adaptive layout (include/apss.h: APSS_GROUP_ADAPT_LAYOUT, apss_group_relayout,
apss_group_layout_get; csrc/apss_group.hip): a group that re-decides its term cuts and shared dense head as a streamed store
grows, rebuilds the store in the new layout from whole rows reassembled out of the members' slices, and swaps only when
every member succeeded.  The reference's harness sends one vector per message (LoadGenerator.scala:58-74) into an index
that grows from empty (IndexingWorkerActor.scala:61-71).  Every member shares device 0 (exchange by copies)."""
import numpy as np
import pytest

from apss import _lib, synth
from helpers import assert_same_pairs, to_map

pytestmark = pytest.mark.gpu

BAND = TOL = 2e-5


def _group(dim, theta, T, adapt=True, **kw):
    from apss.engine import ApssGroup
    return ApssGroup(dim, theta, [0] * T, group_flags=_lib.GROUP_ADAPT_LAYOUT if adapt else 0, **kw)


def _batch(rp, idx, val, b0, b1, ids=None):
    sl = slice(rp[b0], rp[b1])
    return (np.arange(b0, b1) if ids is None else ids[b0:b1]), rp[b0:b1 + 1] - rp[b0], idx[sl], val[sl]


def _equal_cuts(dim, T):
    return [dim * g // T for g in range(T + 1)]


# the power-law stream (C3's shape with Zipf(1) terms, where a plain index takes a dense head by itself): one vector per call
# for the first 2000 rows, then batches of growing size up to 40k rows
N1, DIM1, NNZ1, THETA1 = 40_000, 100_000, 100, 0.8
STREAM1 = [1] * 2000 + [1000, 1000, 2000, 4000, 6000, 10000, 14000]


@pytest.mark.timeout(1500)
def test_stream_from_single_vectors_relayouts_to_balanced_cuts_and_a_head(oracle):
    """Every call equals the oracle: the call's answer is every pair (q in the batch, c stored so far, c != q) at or above
    theta, which the oracle's exact join over the rows stored so far gives for the batch's queries -- for the whole call up
    to 300 queries, for a sample of 300 beyond (the oracle's cost grows with the store) -- and every call equals a plain
    handle fed the same stream in full.  At the end the adaptive group has the head a plain index picks and balanced cuts;
    the same stream without the flag keeps the equal cuts and no head of its single-vector first call."""
    from apss.engine import ApssIndex
    rp, idx, val = synth.make_vectors(N1, DIM1, NNZ1, 1.0, seed=5, dup_frac=0.1)
    assert sum(STREAM1) == N1
    with ApssIndex(DIM1, THETA1) as ix:  # precondition: a plain index on all the rows takes a dense head
        ix.insert(np.arange(N1), rp, idx, val)
        ix.query(np.arange(100), rp[:101], idx[:rp[100]], val[:rp[100]])
        assert ix.stats()["head_terms"] > 0
    T = 4
    with _group(DIM1, THETA1, T) as g, ApssIndex(DIM1, THETA1) as plain:
        b0 = 0
        for B in STREAM1:
            b1 = b0 + B
            args = _batch(rp, idx, val, b0, b1)
            got = to_map(*g.insert_and_query(*args))
            assert_same_pairs(got, to_map(*plain.insert_and_query(*args)), THETA1, band=BAND, tol=TOL)
            qs = min(B, 300)
            oq, oc, os_ = oracle.selfjoin_pairs(DIM1, THETA1, rp[:b1 + 1], idx[:rp[b1]], val[:rp[b1]], b0, b0 + qs)
            assert_same_pairs({k: v for k, v in got.items() if k[0] < b0 + qs}, to_map(oq, oc, os_), THETA1, band=BAND, tol=TOL)
            b0 = b1
        lo = g.layout()
        st = g.stats()
    assert st["rows"] == N1
    assert lo["evaluations"] >= 5 and lo["relayouts"] >= 2, lo
    assert lo["head_terms"] > 0 and lo["layout_rows"] == N1, lo
    dfsq = np.array(lo["dfsq"])
    assert dfsq.min() > 0 and dfsq.max() / dfsq.mean() < 1.3, dfsq
    assert lo["term_cuts"] != _equal_cuts(DIM1, T)
    # the same stream without the flag: the layout of the first (single-vector) batch, for good
    with _group(DIM1, THETA1, T, adapt=False) as g:
        b0 = 0
        for B in STREAM1:
            g.insert(*_batch(rp, idx, val, b0, b0 + B))
            b0 += B
        lo = g.layout()
    assert lo["head_terms"] == 0 and lo["term_cuts"] == _equal_cuts(DIM1, T), lo
    assert lo["evaluations"] == 0 and lo["relayouts"] == 0 and lo["next_eval_rows"] == 0, lo


@pytest.mark.timeout(900)
def test_relayout_leaves_the_answers_and_the_store_unchanged(oracle):
    """a frozen-index query gives the same pairs before and after re-layouts to two explicit cut sets and to a decided one;
    rows and postings summed over the members do not change"""
    n, dim, nnz, theta, T = 6000, 4000, 20, 0.5, 3
    rp, idx, val = synth.make_vectors(n + 600, dim, nnz, 1.0, seed=41, dup_frac=0.1)
    ids = np.arange(n + 600, dtype=np.int64) * 7 + 3
    w = oracle.Worker(dim, theta)
    w.index_data(*_batch(rp, idx, val, 0, n, ids), build_only=True)
    qargs = _batch(rp, idx, val, n, n + 600, ids)
    want = to_map(*w.index_data(*qargs, query_only=True))
    assert len(want) > 50
    with _group(dim, theta, T, adapt=False) as g:
        g.insert(*_batch(rp, idx, val, 0, n, ids))

        def snapshot():
            ms = [g.member_stats(i) for i in range(T)]
            assert all(m["rows"] == n for m in ms)
            return sum(m["nnz"] for m in ms)

        nnz0 = snapshot()
        base = to_map(*g.query(*qargs))
        assert_same_pairs(base, want, theta, band=BAND, tol=TOL)
        for cuts in ([0, 100, 900, dim], [0, 2500, 3999, dim], None):
            g.relayout(cuts)
            lo = g.layout()
            if cuts is not None:
                assert lo["term_cuts"] == cuts
            assert snapshot() == nnz0 and g.stats()["rows"] == n
            assert_same_pairs(to_map(*g.query(*qargs)), base, theta, band=BAND, tol=TOL)
        assert lo["relayouts"] >= 3 and lo["evaluations"] == 3 and lo["layout_rows"] == n, lo


@pytest.mark.timeout(900)
@pytest.mark.parametrize("mode", ["normalize_prune", "admission"])
def test_ingest_flags_survive_relayouts(oracle, mode):
    """rows re-inserted by a re-layout are the STORED rows: not normalised, pruned or admitted a second time (a pruned row
    re-normalised would change its scores) -- every call of a stream across re-layouts equals the oracle on pre-filtered rows"""
    n, dim, nnz, theta, thr, T = 8000, 1500, 24, 0.55, 0.08, 3
    if mode == "admission":  # (test_group_admission_filter_drops_the_same_rows_on_every_member's shape)
        dim, nnz = 1200, 12
    rp, idx, val = synth.make_vectors(n, dim, nnz, 0.0, seed=8, dup_frac=0.15 if mode == "normalize_prune" else 0.4)
    rng = np.random.default_rng(1)
    if mode == "normalize_prune":
        raw = val * np.repeat(rng.uniform(0.5, 3.0, size=n), nnz)
        nv = oracle.l2_normalize(rp, raw)
        prp, pidx, pval = oracle.value_prune(rp, idx, nv, thr)
        kw = dict(flags=_lib.FLAG_NORMALIZE | _lib.FLAG_VALUE_PRUNE, index_threshold=thr, head_terms=-1)
    else:
        theta = 0.6
        raw = val * np.repeat(rng.uniform(0.12, 1.0, size=n), nnz)  # un-normalised: the row sums straddle theta
        keep = oracle.admission(rp, raw, theta)
        assert 0.2 * n < keep.sum() < 0.95 * n
        kw = dict(flags=_lib.FLAG_ADMISSION, head_terms=-1)
    w = oracle.Worker(dim, theta)
    with _group(dim, theta, T, **kw) as g:
        b0 = 0
        for B in (500, 600, 1200, 2500, 3200):
            b1 = b0 + B
            got = to_map(*g.insert_and_query(*_batch(rp, idx, raw, b0, b1)))
            if mode == "normalize_prune":
                want = to_map(*w.index_data(*_batch(prp, pidx, pval, b0, b1)))
            else:
                rows = b0 + np.nonzero(keep[b0:b1])[0]
                krp = np.concatenate([[0], np.cumsum(rp[rows + 1] - rp[rows])]).astype(np.int64)
                sel = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in rows])
                want = to_map(*w.index_data(rows, krp, idx[sel], raw[sel]))
            assert_same_pairs(got, want, theta, band=BAND, tol=TOL)
            b0 = b1
        lo = g.layout()
    assert lo["relayouts"] >= 2, lo


@pytest.mark.timeout(600)
def test_a_failed_relayout_leaves_the_old_layout(oracle, monkeypatch):
    """APSS_DEBUG=relayout_fail=1: member 1's re-insert fails during the re-layout the second batch triggers -- the call
    returns the error, the layout and store are the old ones and answer a frozen-index query; without the hook a new group
    replays the stream correctly"""
    from apss.engine import ApssError
    n, dim, nnz, theta, T = 1400, 3000, 16, 0.5, 3
    rp, idx, val = synth.make_vectors(n, dim, nnz, 1.0, seed=19, dup_frac=0.15)
    a1, a2, aq = _batch(rp, idx, val, 0, 600), _batch(rp, idx, val, 600, 1200), _batch(rp, idx, val, 1200, 1400)
    monkeypatch.setenv("APSS_DEBUG", "relayout_fail=1")
    w = oracle.Worker(dim, theta)
    with _group(dim, theta, T) as g:
        assert_same_pairs(to_map(*g.insert_and_query(*a1)), to_map(*w.index_data(*a1)), theta, band=BAND, tol=TOL)
        before = g.layout()
        assert before["next_eval_rows"] == 1200
        with pytest.raises(ApssError) as e:
            g.insert_and_query(*a2)
        assert "relayout_fail" in str(e.value)
        assert g.layout() == before
        assert g.stats()["rows"] == 600
        assert_same_pairs(to_map(*g.query(*aq)), to_map(*w.index_data(*aq, query_only=True)), theta, band=BAND, tol=TOL)
    monkeypatch.delenv("APSS_DEBUG")
    w = oracle.Worker(dim, theta)
    with _group(dim, theta, T) as g:
        for a in (a1, a2):
            assert_same_pairs(to_map(*g.insert_and_query(*a)), to_map(*w.index_data(*a)), theta, band=BAND, tol=TOL)
        assert g.layout()["relayouts"] == 1


@pytest.mark.timeout(900)
def test_schedule_edge_cases(oracle):
    """a large batch after a small first batch lands in a layout decided with it; named cuts never move while the head is
    re-decided; query-only calls never re-layout"""
    rp, idx, val = synth.make_vectors(N1 + 10_100, DIM1, NNZ1, 1.0, seed=5, dup_frac=0.1)
    T = 4
    with _group(DIM1, THETA1, T) as g:
        g.insert(*_batch(rp, idx, val, 0, 100))
        assert g.layout()["layout_rows"] == 100 and g.layout()["term_cuts"] == _equal_cuts(DIM1, T)
        g.insert(*_batch(rp, idx, val, 100, 50_100))
        lo = g.layout()
        assert lo["layout_rows"] >= 50_100 and lo["relayouts"] == 1 and lo["head_terms"] > 0, lo
        assert lo["next_eval_rows"] == 100_200
        q = _batch(rp, idx, val, 50_000, 50_100)
        oq, oc, os_ = oracle.selfjoin_pairs(DIM1, THETA1, rp[:50_101], idx[:rp[50_100]], val[:rp[50_100]], 50_000, 50_100)
        assert_same_pairs(to_map(*g.query(*q)), to_map(oq, oc, os_), THETA1, band=BAND, tol=TOL)  # (stored rows, same ids)
    named = [0, 300, 2000, 9000, DIM1]
    with _group(DIM1, THETA1, T, term_cuts=named) as g:
        g.insert(*_batch(rp, idx, val, 0, 100))
        assert g.layout()["head_terms"] == 0
        g.insert(*_batch(rp, idx, val, 100, N1))
        lo = g.layout()
        assert lo["term_cuts"] == named and lo["head_terms"] > 0 and lo["relayouts"] == 1, lo
    with _group(DIM1, THETA1, T) as g:
        g.insert(*_batch(rp, idx, val, 0, 600))
        before = g.layout()
        for b0 in range(600, 6600, 2000):
            g.query(*_batch(rp, idx, val, b0, b0 + 2000))
        assert g.layout() == before and before["evaluations"] == 0
        g.insert(*_batch(rp, idx, val, 600, 1100))  # 1100 rows: below max(1024, 2 x 600)
        assert g.layout()["evaluations"] == 0
        g.insert(*_batch(rp, idx, val, 1100, 1300))
        lo = g.layout()
        assert lo["evaluations"] == 1 and lo["layout_rows"] == 1300, lo
