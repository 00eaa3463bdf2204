"""Per-query top-k in windows of query rows (apss_set_top_k_window, csrc/apss_window.hpp): the plan against numpy, the list
against the oracle and, element by element, against the unwindowed call of a twin handle.

The figures pinned below were computed on the CPU from the generators' seeds and are recomputed here:
  b(q) = min(sum of df over the row's terms, stored rows), df = rows of the store holding the term;
  greedy cuts: a window is the longest run of rows from its start whose b sum to <= max_pairs;
  pairs per window: the off-diagonal structural non-zeros of X X^T with score >= theta."""
import numpy as np
import pytest

from apss import _lib, synth
from apss.engine import ApssError, ApssIndex
from test_gpu_topk import A_DIM, A_N, A_THETA, LOWER, _device_list, check_topk, rows_of

pytestmark = pytest.mark.gpu

Z_N, Z_DIM = 2000, 64
Z_PAIRS, Z_LONGEST, Z_BOUND_TOTAL, Z_CLAMPED = 2710116, 1431, 3974554, 1143
A_BOUND_TOTAL = 2248921
TIMING = {"probe_ms", "build_ms", "rescore_ms", "head_ms"}


def bounds(rp, idx, dim, store_idx, store_rows):
    df = np.bincount(store_idx, minlength=dim).astype(np.int64)
    per_entry = df[idx]
    b = np.array([per_entry[rp[r]:rp[r + 1]].sum() for r in range(len(rp) - 1)], dtype=np.int64)
    return np.minimum(b, store_rows)


def greedy_cuts(b, budget):
    cuts, run = [0], 0
    for q, v in enumerate(b):
        if q > cuts[-1] and run + int(v) > budget:
            cuts.append(q)
            run = 0
        run += int(v)
    cuts.append(len(b))
    return np.array(cuts, dtype=np.int64)


def pairs_per_row(rp, idx, val, dim, theta):
    import scipy.sparse as sp
    n = len(rp) - 1
    g = (sp.csr_matrix((val, idx, rp), shape=(n, dim), dtype=np.float64) @
         sp.csr_matrix((val, idx, rp), shape=(n, dim), dtype=np.float64).T).tocoo()
    keep = (g.row != g.col) & (g.data >= theta)
    return np.bincount(g.row[keep], minlength=n)


def per_window(x, cuts):
    return np.add.reduceat(x, cuts[:-1])


def assert_same_list(got, want):
    assert len(got[0]) == len(want[0])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))


@pytest.fixture(scope="module")
def zero(oracle):
    rp, idx, val = synth.make_vectors(Z_N, Z_DIM, 8, 0.0, seed=5, dup_frac=0.1)
    orc = oracle.selfjoin_pairs(Z_DIM, 0.0 - LOWER, rp, idx, val)
    b = bounds(rp, idx, Z_DIM, idx, Z_N)
    pr = pairs_per_row(rp, idx, val, Z_DIM, 0.0)
    assert len(orc[0]) == Z_PAIRS == int(pr.sum()) and int(pr.max()) == Z_LONGEST
    assert int(b.sum()) == Z_BOUND_TOTAL and int((b == Z_N).sum()) == Z_CLAMPED
    assert np.all(pr <= b)  # the bound does bound
    return dict(rp=rp, idx=idx, val=val, ids=np.arange(Z_N, dtype=np.int64), orc=orc, b=b, pr=pr)


@pytest.fixture(scope="module")
def zero_unwindowed(zero):
    """one fresh unwindowed handle, one call, k = 8: the statistics every windowed run is compared with"""
    z = zero
    with ApssIndex(Z_DIM, 0.0, top_k=8) as ix:
        ix.insert_and_query(z["ids"], z["rp"], z["idx"], z["val"])
        assert ix.topk_window_info()["windows"] == 0 and len(ix.topk_window_cuts()) == 0
        return ix.stats()


@pytest.fixture(scope="module")
def shape_a(oracle):
    rp, idx, val = synth.make_vectors(A_N, A_DIM, 12, 1.0, seed=21, dup_frac=0.1)
    ids = np.arange(A_N, dtype=np.int64) + 100
    oq, oc, os_ = oracle.selfjoin_pairs(A_DIM, A_THETA - LOWER, rp, idx, val)
    b = bounds(rp, idx, A_DIM, idx, A_N)
    assert int(b.sum()) == A_BOUND_TOTAL
    return dict(rp=rp, idx=idx, val=val, ids=ids, orc=(oq + 100, oc + 100, os_), b=b)


def run_a(a, k, window, flags=0, head_terms=0, self_join=False):
    """shape A into a fresh handle; returns fetched triples, device list, topk info, window info, cuts, stats"""
    with ApssIndex(A_DIM, A_THETA, tile_rows=512, flags=flags, head_terms=head_terms, top_k=k, top_k_window=window) as ix:
        if self_join:
            ix.insert(a["ids"], a["rp"], a["idx"], a["val"])
            got = ix.self_join()
        else:
            got = ix.insert_and_query(a["ids"], a["rp"], a["idx"], a["val"])
        return dict(got=got, dev=_device_list(ix), tk=ix.topk_info(), tw=ix.topk_window_info(), cuts=ix.topk_window_cuts(),
                    st=ix.stats())


@pytest.fixture(scope="module")
def a_unwindowed(shape_a):
    """the unwindowed two-directional self-join of shape A per k, run once"""
    cache = {}

    def get(k):
        if k not in cache:
            cache[k] = run_a(shape_a, k, 0, flags=_lib.FLAG_NO_SYMMETRY, self_join=True)
        return cache[k]
    return get


# ---- 1. theta = 0, 40 windows of 50 rows: the plan, the list, the statistics, the memory
@pytest.mark.parametrize("k", [1, 8, 64])
def test_theta_zero_forty_windows(zero, zero_unwindowed, k):
    z = zero
    cuts = greedy_cuts(z["b"], 100000)
    assert len(cuts) == 41 and np.all(np.diff(cuts) == 50)
    assert int(per_window(z["b"], cuts).max()) == 99676 and int(per_window(z["pr"], cuts).max()) == 68031
    with ApssIndex(Z_DIM, 0.0, top_k=k, top_k_window=100000) as ix:
        got = ix.insert_and_query(z["ids"], z["rp"], z["idx"], z["val"])
        tk, tw, st, dev_cuts = ix.topk_info(), ix.topk_window_info(), ix.stats(), ix.topk_window_cuts()
        assert ix.result_count() == len(got[0])
    print("theta 0, 40 windows, k=%d: %s %s hbm %d (unwindowed %d)" % (k, tw, tk, st["hbm_bytes"], zero_unwindowed["hbm_bytes"]))
    assert np.array_equal(dev_cuts, cuts)
    assert tw["windows"] == 40 and tw["max_pairs"] == 100000 and tw["rows_window_min"] == tw["rows_window_max"] == 50
    assert tw["bound_total"] == Z_BOUND_TOTAL and tw["bound_window_max"] == 99676 and tw["pairs_window_max"] == 68031
    assert tw["single_row_over"] == 0 and tw["overflow_reruns"] == 0
    assert tw["plan_launches"] == 2 and tw["plan_ms"] > 0
    check_topk(got, z["orc"], k, 0.0, z["ids"])
    assert tk["k"] == k and tk["pairs_over_theta"] == Z_PAIRS and tk["queries_cut"] == Z_N and tk["longest_segment"] == Z_LONGEST
    assert tk["kept"] == Z_N * k == len(got[0]) == st["result_pairs"]
    assert tk["select_launches"] == 4 * 40 and tk["select_ms"] > 0
    assert st["posting_visits"] == zero_unwindowed["posting_visits"]
    assert st["candidate_pairs"] == zero_unwindowed["candidate_pairs"]
    if k == 8:
        # the unwindowed handle holds three 4-byte arrays of the whole list; the windowed one needs no more than the 2^20-pair
        # floor of a first result reservation
        assert zero_unwindowed["hbm_bytes"] - st["hbm_bytes"] >= 12 * (Z_PAIRS - (1 << 20))


# ---- 2. two large windows: lists above the 2^20-pair floor, only the up-front reservation keeps the probe from running twice
def test_theta_zero_two_windows(zero):
    z = zero
    cuts = greedy_cuts(z["b"], 2000000)
    assert sorted(np.diff(cuts)) == [994, 1006]
    assert int(per_window(z["b"], cuts).max()) == 1999157 and int(per_window(z["pr"], cuts).max()) == 1362237 > (1 << 20)
    with ApssIndex(Z_DIM, 0.0, top_k=8, top_k_window=2000000) as ix:
        got = ix.insert_and_query(z["ids"], z["rp"], z["idx"], z["val"])
        tw, dev_cuts = ix.topk_window_info(), ix.topk_window_cuts()
    print("theta 0, 2 windows: %s" % tw)
    assert np.array_equal(dev_cuts, cuts)
    assert tw["windows"] == 2 and tw["bound_window_max"] == 1999157 and tw["pairs_window_max"] == 1362237
    assert tw["overflow_reruns"] == 0
    check_topk(got, z["orc"], 8, 0.0, z["ids"])


# ---- 3. the two-pass path: shape A in 38 windows equals the unwindowed two-directional self-join element by element
@pytest.mark.parametrize("k", [3, 64])
def test_two_pass_thirty_eight_windows(shape_a, a_unwindowed, k):
    a = shape_a
    cuts = greedy_cuts(a["b"], 60000)
    rows = np.diff(cuts)
    assert len(rows) == 38 and rows.min() == 20 and rows.max() == 40 and int(per_window(a["b"], cuts).max()) == 60000
    plain = a_unwindowed(k)
    win = run_a(a, k, 60000, flags=_lib.FLAG_NO_SYMMETRY, self_join=True)
    print("shape A, 38 windows, k=%d: %s" % (k, win["tw"]))
    assert plain["tw"]["windows"] == 0
    assert np.array_equal(win["cuts"], cuts)
    tw = win["tw"]
    assert tw["windows"] == 38 and tw["rows_window_min"] == 20 and tw["rows_window_max"] == 40
    assert tw["bound_total"] == A_BOUND_TOTAL and tw["bound_window_max"] == 60000 and tw["single_row_over"] == 0
    assert tw["overflow_reruns"] == 0
    assert_same_list(win["dev"], plain["dev"])
    check_topk(win["got"], a["orc"], k, A_THETA, a["ids"])
    for key in ("pairs_over_theta", "kept", "queries_cut", "longest_segment"):
        assert win["tk"][key] == plain["tk"][key], key
    assert win["st"]["candidate_pairs"] == plain["st"]["candidate_pairs"]
    assert win["st"]["posting_visits"] == plain["st"]["posting_visits"]
    assert win["st"]["result_pairs"] == len(win["got"][0])


# ---- 4. the other probe paths
@pytest.mark.parametrize("flags", [_lib.FLAG_EXACT_ACCUM, _lib.FLAG_FORCE_GENERAL], ids=["exact_accum", "general"])
def test_probe_paths(shape_a, flags):
    a = shape_a
    plain = run_a(a, 8, 0, flags=flags)
    win = run_a(a, 8, 60000, flags=flags)
    assert win["tw"]["windows"] == 38 and plain["tw"]["windows"] == 0
    check_topk(win["got"], a["orc"], 8, A_THETA, a["ids"])
    assert win["tk"]["kept"] == plain["tk"]["kept"] == len(win["got"][0])


# ---- 5. a dense-head block: both filters, twice the reservation
def test_dense_head(shape_a):
    a = shape_a
    plain = run_a(a, 8, 0, head_terms=32)
    win = run_a(a, 8, 60000, head_terms=32)
    assert plain["st"]["head_terms"] > 0 and win["st"]["head_terms"] > 0
    assert win["tw"]["windows"] == 38 and win["tw"]["overflow_reruns"] == 0
    assert_same_list(win["dev"], plain["dev"])
    assert win["tk"]["kept"] == plain["tk"]["kept"] and win["tk"]["pairs_over_theta"] == plain["tk"]["pairs_over_theta"]


# ---- 6. every row over the budget: windows of one
def test_single_rows_over_the_budget(shape_a):
    a = shape_a
    rp, idx, val = rows_of(a["rp"], a["idx"], a["val"], 0, 8)
    qids = np.arange(8, dtype=np.int64) + 900000
    b = bounds(rp, idx, A_DIM, a["idx"], A_N)
    assert 1179 <= int(b.min()) and int(b.max()) <= 1500
    lists = []
    for window in (0, 1000):
        with ApssIndex(A_DIM, A_THETA, tile_rows=512, top_k=8, top_k_window=window) as ix:
            ix.insert(a["ids"], a["rp"], a["idx"], a["val"])
            ix.query(qids, rp, idx, val)
            lists.append(_device_list(ix))
            tw, cuts = ix.topk_window_info(), ix.topk_window_cuts()
    assert tw["windows"] == 8 and tw["single_row_over"] == 8 and tw["bound_total"] == int(b.sum())
    assert tw["rows_window_min"] == tw["rows_window_max"] == 1
    assert np.array_equal(cuts, np.arange(9))
    assert len(lists[0][0]) > 8  # (row r of the batch finds stored row r at least)
    assert_same_list(lists[1], lists[0])


# ---- 7. streams: every batch sees itself and everything before it
def test_streamed_batches(shape_a, oracle):
    a = shape_a
    w = oracle.Worker(A_DIM, A_THETA - LOWER)
    with ApssIndex(A_DIM, A_THETA, tile_rows=512, top_k=3, top_k_window=60000) as ix, \
            ApssIndex(A_DIM, A_THETA, tile_rows=512, top_k=3) as twin:
        for batch in range(3):
            lo, hi = 500 * batch, 500 * (batch + 1)
            rp, idx, val = rows_of(a["rp"], a["idx"], a["val"], lo, hi)
            got = ix.insert_and_query(a["ids"][lo:hi], rp, idx, val)
            mine = _device_list(ix)
            twin.insert_and_query(a["ids"][lo:hi], rp, idx, val)
            assert_same_list(mine, _device_list(twin))
            orc = w.index_data(a["ids"][lo:hi], rp, idx, val)
            check_topk(got, orc, 3, A_THETA, a["ids"][lo:hi])
            # every batch is windowed: 500 x 500 > 60000 already.  The plan sees the store WITH the batch
            cuts = greedy_cuts(bounds(rp, idx, A_DIM, a["idx"][:a["rp"][hi]], hi), 60000)
            assert len(cuts) - 1 == (5, 9, 13)[batch]
            assert ix.topk_window_info()["windows"] == len(cuts) - 1 and np.array_equal(ix.topk_window_cuts(), cuts)
            assert twin.topk_window_info()["windows"] == 0
    w.close()


# ---- 8. the regrow hook: no up-front reservation, the lists overflow window by window
def test_regrow_hook(shape_a, a_unwindowed, monkeypatch):
    plain = a_unwindowed(3)
    monkeypatch.setenv("APSS_DEBUG", "res_cap=256")
    win = run_a(shape_a, 3, 60000, flags=_lib.FLAG_NO_SYMMETRY, self_join=True)
    print("regrow hook: %s" % win["tw"])
    assert win["tw"]["windows"] == 38 and win["tw"]["overflow_reruns"] > 0
    assert_same_list(win["dev"], plain["dev"])


# ---- 9. edges
def test_edges(shape_a):
    a = shape_a
    one = rows_of(a["rp"], a["idx"], a["val"], 0, 1)
    with ApssIndex(A_DIM, A_THETA, tile_rows=512, top_k=3) as ix:
        with pytest.raises(ApssError) as e:
            ix.set_top_k_window(-1)
        assert e.value.code == _lib.E_INVALID
        ix.set_top_k_window(60000)
        ix.clear()  # the setting survives clear
        got = ix.insert_and_query(a["ids"], a["rp"], a["idx"], a["val"])
        assert ix.topk_window_info()["windows"] == 38 and ix.topk_window_info()["max_pairs"] == 60000
        check_topk(got, a["orc"], 3, A_THETA, a["ids"])
        n = ix.result_count()
        ix.set_top_k_window(0)  # changing the setting leaves the last call's results alone
        assert ix.result_count() == n and ix.topk_window_info()["windows"] == 38
        # nq x rows <= max_pairs: one window, nothing planned
        ix.set_top_k_window(A_N)
        ix.query(np.array([7], np.int64), *one)
        tw = ix.topk_window_info()
        assert tw["windows"] == 0 and tw["plan_launches"] == 0 and tw["max_pairs"] == A_N and len(ix.topk_window_cuts()) == 0
        ix.set_top_k_window(A_N - 1)
        ix.query(np.array([7], np.int64), *one)
        assert ix.topk_window_info()["windows"] == 1 and list(ix.topk_window_cuts()) == [0, 1]
        # nq = 0
        q, c, s = ix.query(np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0))
        assert len(q) == 0 and ix.topk_window_info()["windows"] == 0 and ix.topk_info()["kept"] == 0
    with ApssIndex(A_DIM, A_THETA, term_range=(0, A_DIM // 2)) as shard:
        with pytest.raises(ApssError) as e:
            shard.set_top_k_window(1000)
        assert e.value.code == _lib.E_UNSUPPORTED and "term shard" in str(e.value)
        shard.set_top_k_window(0)


def test_window_without_k_costs_nothing(shape_a):
    a = shape_a
    stats = []
    for window in (0, 60000):
        with ApssIndex(A_DIM, A_THETA, tile_rows=512, top_k_window=window) as ix:
            ix.insert_and_query(a["ids"], a["rp"], a["idx"], a["val"])
            tw, tk = ix.topk_window_info(), ix.topk_info()
            assert tw["windows"] == 0 and tw["plan_launches"] == 0 and tw["plan_ms"] == 0 and tw["max_pairs"] == window
            assert tk["select_launches"] == 0 and tk["k"] == 0 and tk["kept"] == ix.result_count()
            stats.append(ix.stats())
    for key in stats[0]:
        if key not in TIMING:
            assert stats[0][key] == stats[1][key], key
