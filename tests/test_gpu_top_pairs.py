"""The global top-K on the device (apss_set_top_pairs, csrc/apss_top_pairs.hpp).

The yardstick throughout is the list the same handle gives with top_pairs = 0, read from the device (query row, slot, fp32 score),
sorted on the host with np.lexsort by (-score as float64 with -0.0 as +0.0, query id, candidate id, query row, slot) and cut to K.
The device list must equal it element by element: query rows, slots and score bits.

Planted scores (test 2).  The issue asks for the bit positions {0, 7, 8, 15, 16, 22, 23, 29} with every weight in (0.05, 1).  Two
floats in (0.05, 1) have exponent fields 122 .. 126 and share every bit above 25, so no two of them differ first at bit 29; the
highest case here is bit 25 (the highest bit at which two scores of this range can differ), the others are as asked."""
import os
import subprocess

import numpy as np
import pytest

from apss import _lib, synth
from apss.engine import ApssError, ApssIndex
from helpers import TOL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "all-pairs-similarity_amd", "host")

A_N, A_DIM, A_THETA, A_PAIRS = 1500, 300, 0.45, 45562
A_KS = (1, 7, 1024, 1025, A_PAIRS - 1, A_PAIRS, A_PAIRS + 1, 1 << 20)


def device_list(ix):
    import torch
    _, _, _, n = ix.results_dev()
    q = torch.empty(n, dtype=torch.int32, device="cuda")
    c = torch.empty(n, dtype=torch.int32, device="cuda")
    s = torch.empty(n, dtype=torch.float32, device="cuda")
    if n:
        ix.results_to(q, c, s)
    torch.cuda.synchronize()
    return q.cpu().numpy(), c.cpu().numpy(), s.cpu().numpy()


def ranked(lst, q_ext, c_ext, K):
    """the first K of the list in the total order.  (The pairs that can be among them -- score at or above the K-th -- are picked
    first, so that a list of millions sorts ten thousand entries: the same K as sorting it whole)"""
    q, c, s = lst
    s = np.where(s == 0, np.float32(0.0), s).astype(np.float32)  # -0.0 counts as, and is reported as, +0.0
    neg = -s.astype(np.float64)
    if 0 < K < len(s):
        kth = np.partition(neg, K - 1)[K - 1]
        pick = np.nonzero(neg <= kth)[0]
    else:
        pick = np.arange(len(s))
    q, c, s, neg = q[pick], c[pick], s[pick], neg[pick]
    order = np.lexsort((c, q, c_ext[c], q_ext[q], neg))[:K]
    return q[order], c[order], s[order]


def assert_same_list(got, want):
    assert len(got[0]) == len(want[0]), (len(got[0]), len(want[0]))
    assert np.array_equal(got[0], want[0]), "query rows differ at %s" % np.nonzero(got[0] != want[0])[0][:5]
    assert np.array_equal(got[1], want[1]), "slots differ at %s" % np.nonzero(got[1] != want[1])[0][:5]
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), "score bits differ"


def check_info(info, K, n, want):
    assert info["k_pairs"] == K and info["pairs_in"] == n and info["kept"] == min(K, n) == len(want[0])
    assert info["launches"] > 0 and info["select_ms"] > 0
    if K < n:
        assert info["above"] + info["tied_kept"] == info["kept"] and info["tied"] >= info["tied_kept"] > 0
        assert info["above"] < K
        assert np.float32(info["kth_score"]).view(np.uint32) == want[2][-1].view(np.uint32)
    else:  # nothing was cut
        assert info["above"] == info["tied"] == info["tied_kept"] == 0 and info["kth_score"] == 0


@pytest.fixture(scope="module")
def shape_a():
    rp, idx, val = synth.make_vectors(A_N, A_DIM, 12, 1.0, seed=21, dup_frac=0.1)
    ext = 5000 - np.arange(A_N, dtype=np.int64)  # external ids DESCEND with the slot: id order and slot order disagree
    return dict(rp=rp, idx=idx, val=val, ext=ext)


# ---- 1. shape A: K below, at and above the list's length, two probe paths, the grid-stride loops' later trips
@pytest.mark.parametrize("flags,debug", [(0, None), (_lib.FLAG_EXACT_ACCUM, None), (0, "tp_grid=2")],
                         ids=["default", "exact_accum", "tp_grid_2"])
def test_shape_a(shape_a, flags, debug, monkeypatch):
    a = shape_a
    if debug:
        monkeypatch.setenv("APSS_DEBUG", debug)
    with ApssIndex(A_DIM, A_THETA, tile_rows=512, flags=flags) as ix:
        ix.insert(a["ext"], a["rp"], a["idx"], a["val"])
        assert ix.self_join(fetch=False) == A_PAIRS
        full = device_list(ix)
        for K in A_KS:
            ix.set_top_pairs(K)
            assert ix.self_join(fetch=False) == min(K, A_PAIRS)
            got, info, st = device_list(ix), ix.top_pairs_info(), ix.stats()
            want = ranked(full, a["ext"], a["ext"], K)
            assert_same_list(got, want)
            print("shape A K=%d flags=%d %s: %s" % (K, flags, debug, info))
            check_info(info, K, A_PAIRS, want)
            assert st["result_pairs"] == ix.result_count() == min(K, A_PAIRS)
            if K >= A_PAIRS:  # nothing dropped, the list in rank order
                assert np.all(np.diff(got[2].astype(np.float64)) <= 0)
                assert sorted(zip(got[0].tolist(), got[1].tolist())) == sorted(zip(full[0].tolist(), full[1].tolist()))
        # what fetch() gives is that list with the ids looked up
        fq, fc, fs = ix.fetch()
        assert np.array_equal(fq, a["ext"][got[0]]) and np.array_equal(fc, a["ext"][got[1]]) and np.array_equal(fs, got[2])


# ---- 2. planted scores: a store whose rows meet the query rows in ONE term, so that a score is one fp32 product 1.0f * w_c
P_ROWS, P_Q, P_K, P_THETA = 3000, 5, 4097, 0.05


def planted_store(w, ids):
    """rows of two terms: term 0 with weight w[c], term 1 + c % 64 with sqrt(1 - w[c]^2)"""
    import torch
    n = len(w)
    rp = 2 * np.arange(n + 1, dtype=np.int64)
    idx = np.stack([np.zeros(n, np.int32), (1 + np.arange(n) % 64).astype(np.int32)], axis=1).ravel()
    val = np.stack([w, np.sqrt(1.0 - w.astype(np.float64) ** 2).astype(np.float32)], axis=1).ravel().astype(np.float32)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    return dev(ids), dev(rp), dev(idx), dev(val)


def planted_queries(qids):
    import torch
    n = len(qids)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    return dev(qids), dev(np.arange(n + 1, dtype=np.int64)), dev(np.zeros(n, np.int32)), dev(np.ones(n, np.float32))


def planted_weights(bit):
    """3,000 float32 in (0.05, 1) that share every bit above `bit`; the 820th largest DISTINCT-by-rank weight (the one whose five
    scores hold rank K = 4,097) has `bit` set and zeros below it, 819 weights lie above it and the rest have `bit` clear: the K-th
    score and the next lower one differ first at `bit`"""
    rng = np.random.Generator(np.random.PCG64(100 + bit))
    one = 1 << bit
    if bit <= 22:    # mantissa bits of [0.5, 1)
        base, lo_min, hi_max = 0x3F000000, 0, one << 1
    elif bit == 23:  # exponent fields 124 | 125: [0.125, 0.5)
        base, lo_min, hi_max = 124 << 23, 0, one << 1
    else:            # bit 25: exponent fields 123 (clear) | 124 .. 126 (set): [0.0625, 1)
        assert bit == 25
        base, lo_min, hi_max = 120 << 23, 3 << 23, 7 << 23
    if bit == 0:     # two values only: the cut runs through 5,000 equal scores
        pat = np.concatenate([np.ones(1000, np.int64), np.zeros(2000, np.int64)])
    else:
        above = rng.integers(one + 1, hi_max, size=819)
        below = rng.integers(lo_min, one, size=P_ROWS - 820)
        pat = np.concatenate([above, [one], below])
    w = (base + rng.permutation(pat)).astype(np.uint32).view(np.float32)
    assert w.min() > 0.05 and w.max() < 1.0
    top = np.sort(w)[::-1].view(np.uint32).astype(np.int64)
    assert (int(top[819]) ^ int(top[top < top[819]][0])).bit_length() == bit + 1
    return w


def run_planted(w, store_ids, qids, Ks):
    ids, rp, idx, val = planted_store(w, store_ids)
    out = []
    with ApssIndex(66, P_THETA, head_terms=-1) as ix:
        ix.insert_dev(ids, rp, idx, val)
        assert ix.query_dev(*planted_queries(qids)) == P_ROWS * P_Q
        full = device_list(ix)
        # first: a score IS its candidate's weight, bit for bit (a different summation shows up here, not as a wrong cut)
        assert np.array_equal(full[2].view(np.uint32), w[full[1]].view(np.uint32))
        for K in Ks:
            ix.set_top_pairs(K)
            assert ix.query_dev(*planted_queries(qids)) == K
            got, info = device_list(ix), ix.top_pairs_info()
            want = ranked(full, qids, store_ids, K)
            assert_same_list(got, want)
            check_info(info, K, P_ROWS * P_Q, want)
            out.append(info)
    return out


@pytest.mark.parametrize("bit", [0, 7, 8, 15, 16, 22, 23, 25])
def test_planted_scores_every_digit(bit):
    w = planted_weights(bit)
    store_ids = np.random.Generator(np.random.PCG64(7)).permutation(P_ROWS).astype(np.int64) + 10
    qids = 1000000 + 10 * np.arange(P_Q, 0, -1, dtype=np.int64)  # query ids DESCEND with the row
    info, = run_planted(w, store_ids, qids, [P_K])
    print("planted bit %d: %s" % (bit, info))
    # the cut runs through the five scores of one weight (or, bit 0, of a thousand): query ids break it
    assert info["tied"] == (5000 if bit == 0 else 5) and info["tied_kept"] == (P_K if bit == 0 else 2)


# ---- 3. ties all the way down: one score, store ids in pairs (slot breaks), two query rows under one id (row breaks)
def test_ties_all_the_way_down():
    w = np.full(P_ROWS, 0.75, np.float32)
    store_ids = np.random.Generator(np.random.PCG64(8)).permutation(P_ROWS // 2).astype(np.int64)[np.arange(P_ROWS) % (P_ROWS // 2)] + 10
    qids = 1000000 + np.array([40, 30, 30, 20, 10], dtype=np.int64)
    Ks = [1, P_K, P_ROWS * P_Q - 1]
    for K, info in zip(Ks, run_planted(w, store_ids, qids, Ks)):
        print("all tied K=%d: %s" % (K, info))
        assert info["above"] == 0 and info["tied"] == P_ROWS * P_Q and info["tied_kept"] == K


# ---- 4. theta <= 0 and signed scores: 2.7 M pairs, negative scores and zeros through the key
@pytest.mark.parametrize("signed", [False, True], ids=["theta_zero", "signed"])
def test_theta_zero_and_signed(signed):
    rp, idx, val = synth.make_vectors(2000, 64, 8, 0.0, seed=5, dup_frac=0.1)
    if signed:
        val = val * np.where(np.random.Generator(np.random.PCG64(9)).random(val.size) < 0.5, -1.0, 1.0)
    ids = np.arange(2000, dtype=np.int64)
    with ApssIndex(64, -0.2 if signed else 0.0) as ix:
        ix.insert(ids, rp, idx, val)
        n = ix.self_join(fetch=False)
        assert n > 1000000 and (signed or n == 2710116)
        full = device_list(ix)
        if signed:
            assert (full[2] < 0).any()
        for K in (10, 100000):
            ix.set_top_pairs(K)
            assert ix.self_join(fetch=False) == K
            got, info = device_list(ix), ix.top_pairs_info()
            want = ranked(full, ids, ids, K)
            assert_same_list(got, want)
            print("theta<=0 signed=%s K=%d: %s" % (signed, K, info))
            check_info(info, K, n, want)


# ---- 5. composition, on shape A
def test_behind_per_query_top_k_and_windows(shape_a):
    a = shape_a
    lists = []
    for window in (0, 60000):
        with ApssIndex(A_DIM, A_THETA, tile_rows=512, top_k=8, top_k_window=window) as ix:
            ix.insert(a["ext"], a["rp"], a["idx"], a["val"])
            ix.self_join(fetch=False)
            per_query, tk0 = device_list(ix), ix.topk_info()
            ix.set_top_pairs(500)
            assert ix.self_join(fetch=False) == 500
            got, tk1, info = device_list(ix), ix.topk_info(), ix.top_pairs_info()
            assert (ix.topk_window_info()["windows"] >= 3) == (window > 0)
        want = ranked(per_query, a["ext"], a["ext"], 500)
        assert_same_list(got, want)
        check_info(info, 500, len(per_query[0]), want)
        assert info["pairs_in"] == tk1["kept"]
        for key in tk0:  # the per-query stage reports itself as without the global cut
            if key != "select_ms":
                assert tk0[key] == tk1[key], key
        lists.append(got)
    assert_same_list(lists[1], lists[0])


def test_behind_removal(shape_a):
    a = shape_a
    with ApssIndex(A_DIM, A_THETA, tile_rows=512) as ix:
        ix.insert(a["ext"], a["rp"], a["idx"], a["val"])
        ix.self_join(fetch=False)
        top50 = ranked(device_list(ix), a["ext"], a["ext"], 50)
        ends = np.unique(a["ext"][top50[0][:3]])  # endpoints of the best pairs are among the hundred
        gone = np.concatenate([ends, np.setdiff1d(a["ext"][::15], ends)])[:100]
        assert len(gone) == 100 and np.isin(a["ext"][top50[0]], gone).any()
        assert ix.remove(gone) == 100
        ix.self_join(fetch=False)
        full, dropped = device_list(ix), ix.removal_info()["pairs_dropped"]
        assert dropped > 0
        ix.set_top_pairs(50)
        assert ix.self_join(fetch=False) == 50
        got, info = device_list(ix), ix.top_pairs_info()
        want = ranked(full, a["ext"], a["ext"], 50)
        assert_same_list(got, want)
        check_info(info, 50, len(full[0]), want)
        assert not np.isin(a["ext"][got[0]], gone).any() and not np.isin(a["ext"][got[1]], gone).any()
        assert ix.removal_info()["pairs_dropped"] == dropped


def test_query_stored_and_repeated_query_ids(shape_a):
    a = shape_a
    with ApssIndex(A_DIM, A_THETA, tile_rows=512) as ix:
        ix.insert(a["ext"], a["rp"], a["idx"], a["val"])
        # (d) stored rows as the batch: the batch's rows are the named rows in slot order
        named = a["ext"][np.random.Generator(np.random.PCG64(4)).permutation(A_N)[:200]]
        rows, n = ix.query_stored(named, fetch=False)
        assert rows == 200 and n > 64
        full = device_list(ix)
        batch_ids = a["ext"][np.sort(5000 - named)]  # (the slot of id e is 5000 - e)
        ix.set_top_pairs(64)
        assert ix.query_stored(named, fetch=False) == (200, 64)
        got, info = device_list(ix), ix.top_pairs_info()
        want = ranked(full, batch_ids, a["ext"], 64)
        assert_same_list(got, want)
        check_info(info, 64, n, want)
        fq, fc, _ = ix.fetch()
        assert np.array_equal(fq, batch_ids[got[0]]) and np.array_equal(fc, a["ext"][got[1]])
        # (e) an outside batch whose rows repeat one external id: the query row breaks what the ids leave tied
        ix.set_top_pairs(0)
        lo, hi = a["rp"][100], a["rp"][140]
        rp, idx, val = a["rp"][100:141] - lo, a["idx"][lo:hi], a["val"][lo:hi]
        rp, idx, val = np.concatenate([rp, rp[1:] + rp[-1]]), np.concatenate([idx, idx]), np.concatenate([val, val])  # every row twice
        qids = np.full(80, 777777, dtype=np.int64)
        ix.query(qids, rp, idx, val)
        full = device_list(ix)
        assert len(full[0]) > 300
        ix.set_top_pairs(300)
        ix.query(qids, rp, idx, val)
        got, info = device_list(ix), ix.top_pairs_info()
        want = ranked(full, qids, a["ext"], 300)
        assert_same_list(got, want)
        check_info(info, 300, len(full[0]), want)
        twins = got[0][:-1] + 40 == got[0][1:]
        assert (twins & (got[1][:-1] == got[1][1:])).any()  # a row and its copy, neighbours in rank order


# ---- 5b. every stage behind the join at once: removal, per-query cut in windows, global cut; two kinds of call
ALL_SPLIT, ALL_K, ALL_WINDOW = 1000, 8, 60000


def insert_and_query_count(ix, ids, rp, idx, val):
    """apss_insert_and_query's own n_results (the engine's wrapper fetches instead of returning it)"""
    import ctypes as C
    from apss.engine import _ptr
    ids, rp, idx, val = ix._csr(ids, rp, idx, val)
    n = C.c_int64(-1)
    ix._chk(ix._L.apss_insert_and_query(ix._h, ids.size, _ptr(rp), _ptr(idx), _ptr(val), _ptr(ids), C.byref(n)))
    return n.value


def drive_all_stages(ix, a, named):
    """first 1000 rows stored; then the two calls under test.  Yields after each call"""
    lo = a["rp"][ALL_SPLIT]
    ix.insert(a["ext"][:ALL_SPLIT], a["rp"][:ALL_SPLIT + 1], a["idx"][:lo], a["val"][:lo])
    yield "stored", None
    yield "insert_and_query", insert_and_query_count(ix, a["ext"][ALL_SPLIT:], a["rp"][ALL_SPLIT:] - lo, a["idx"][lo:], a["val"][lo:])
    yield "query_stored", ix.query_stored(named, fetch=False)[1]


def host_stages(lst, q_ext, c_ext, gone, k):
    """what the stages make of an unstaged list, on the host, up to the global cut: the removed rows dropped (a removed query row
    is no row of the batch: the rows after it move up), every query row cut to its k best by (score descending, candidate id,
    slot).  Returns the list and the live rows' ids"""
    from helpers import topk
    q, c, s = lst
    live = ~np.isin(q_ext, gone)
    keep = live[q] & ~np.isin(c_ext[c], gone)
    q, c, s = (np.cumsum(live) - 1)[q[keep]], c[keep], s[keep]
    out = []
    for row in np.unique(q):
        sel = np.nonzero(q == row)[0]
        best = topk({(int(c_ext[c[i]]), int(c[i])): float(s[i]) for i in sel}, k)
        out += [(int(row), slot, v) for (_, slot), v in best]
    cut = (np.array([o[0] for o in out], np.int32), np.array([o[1] for o in out], np.int32), np.array([o[2] for o in out], np.float32))
    return cut, q_ext[live], int(keep.size - keep.sum())


@pytest.fixture(scope="module")
def all_stages_yardstick(shape_a):
    """per call: the per-query-cut list a handle with NO stage on leads to, and the ids of its batch's rows"""
    a = shape_a
    rng = np.random.Generator(np.random.PCG64(12))
    gone = a["ext"][:ALL_SPLIT][rng.permutation(ALL_SPLIT)[:100]]
    distinct = a["ext"][rng.permutation(A_N)[:136]]
    named = rng.permutation(np.concatenate([distinct, distinct[:32], 9000 + np.arange(32, dtype=np.int64)]))  # 64 repeat or are missing
    assert named.size == 200 and 0 < np.isin(distinct, gone).sum() < 136
    cut = {}
    with ApssIndex(A_DIM, A_THETA, tile_rows=512) as ix:
        for call, n in drive_all_stages(ix, a, named):
            if call == "stored":
                continue
            full = device_list(ix)
            assert n == len(full[0]) > 0
            q_ext = a["ext"][ALL_SPLIT:] if call == "insert_and_query" else a["ext"][np.sort(5000 - np.unique(named[named < 9000]))]
            cut[call] = host_stages(full, q_ext, a["ext"], gone, ALL_K)
            assert cut[call][2] > 0  # the removal has pairs to drop
    return dict(gone=gone, named=named, cut=cut)


@pytest.mark.parametrize("K", [7, 1025])
def test_all_stages_at_once(shape_a, all_stages_yardstick, K):
    a, y = shape_a, all_stages_yardstick
    with ApssIndex(A_DIM, A_THETA, tile_rows=512, top_k=ALL_K, top_k_window=ALL_WINDOW, top_pairs=K) as ix:
        for call, n in drive_all_stages(ix, a, y["named"]):
            if call == "stored":
                assert ix.remove(y["gone"]) == 100
                continue
            per_query, q_ext, _ = y["cut"][call]
            want = ranked(per_query, q_ext, a["ext"], K)
            got, info, wi = device_list(ix), ix.top_pairs_info(), ix.topk_window_info()
            print("all stages K=%d %s: n=%d windows=%d %s" % (K, call, n, wi["windows"], info))
            assert_same_list(got, want)
            assert n == ix.result_count() == len(got[0]) == ix.stats()["result_pairs"] == info["kept"] == min(K, len(per_query[0]))
            # 500 / 129 or so query rows, each bounded by its terms' 700 or so postings, against 60 000 pairs a window
            assert wi["windows"] >= 2 and ix.removal_info()["pairs_dropped"] > 0 and ix.topk_info()["k"] == ALL_K
            if call == "query_stored":
                qi = ix.stored_query_info()
                assert (qi["ids_given"], qi["ids_distinct"], qi["rows_selected"]) == (200, 168, len(q_ext))
                assert qi["ids_missing"] == 168 - len(q_ext)


# ---- 6. the setting and the edges
def test_setting_and_edges(shape_a):
    a = shape_a
    with ApssIndex(A_DIM, A_THETA, tile_rows=512) as ix:
        # K = 0 on a fresh handle: nothing launched, nothing reserved by the setting
        ix.insert(a["ext"], a["rp"], a["idx"], a["val"])
        ix.self_join(fetch=False)
        hbm0 = ix.stats()["hbm_bytes"]
        ix.set_top_pairs(0)
        ix.self_join(fetch=False)
        info = ix.top_pairs_info()
        assert info["launches"] == 0 and info["k_pairs"] == 0 and info["select_ms"] == 0 and ix.stats()["hbm_bytes"] == hbm0
        full = device_list(ix)
        for bad in (-1, (1 << 20) + 1):
            with pytest.raises(ApssError) as e:
                ix.set_top_pairs(bad)
            assert e.value.code == _lib.E_INVALID
        ix.set_top_pairs(9)
        assert ix.result_count() == A_PAIRS  # the setting leaves the last call's results alone
        assert ix.self_join(fetch=False) == 9 and ix.stats()["hbm_bytes"] > hbm0
        # an empty batch, and a batch that matches nothing
        q, c, s = ix.query(np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0))
        assert len(q) == 0 and ix.top_pairs_info()["launches"] == 0 and ix.top_pairs_info()["k_pairs"] == 9
        q, c, s = ix.query(np.array([7], np.int64), np.array([0, 1], np.int64), np.array([5], np.int32), np.array([1e-6]))
        assert len(q) == 0 and ix.result_count() == 0 and ix.top_pairs_info()["launches"] == 0
        # K = 0 again: the unordered full set
        ix.set_top_pairs(0)
        assert ix.self_join(fetch=False) == A_PAIRS
        again = device_list(ix)
        assert ix.top_pairs_info()["launches"] == 0
        assert sorted(zip(again[0].tolist(), again[1].tolist())) == sorted(zip(full[0].tolist(), full[1].tolist()))
        # the setting survives clear; an empty store answers nothing
        ix.set_top_pairs(9)
        ix.clear()
        assert ix.self_join(fetch=False) == 0 and ix.top_pairs_info()["launches"] == 0
        ix.insert(a["ext"], a["rp"], a["idx"], a["val"])
        assert ix.self_join(fetch=False) == 9 and ix.top_pairs_info()["k_pairs"] == 9
        assert_same_list(device_list(ix), ranked(full, a["ext"], a["ext"], 9))
    with ApssIndex(A_DIM, A_THETA, top_pairs=11) as ix:  # the constructor's argument
        ix.insert(a["ext"], a["rp"], a["idx"], a["val"])
        assert ix.self_join(fetch=False) == 11
    with ApssIndex(A_DIM, A_THETA, term_range=(0, A_DIM // 2)) as shard:
        with pytest.raises(ApssError) as e:
            shard.set_top_pairs(3)
        assert e.value.code == _lib.E_UNSUPPORTED and "term shard" in str(e.value)
        shard.set_top_pairs(0)
        assert len(shard.insert_and_query(a["ext"], a["rp"], a["idx"], a["val"])[0]) > 0 and shard.top_pairs_info()["launches"] == 0


# ---- 7. against the double-precision oracle, once: the tolerance rule of tests/test_gpu_topk.py's check_topk over the whole call
def test_against_the_oracle(shape_a, oracle):
    a = shape_a
    K, cut = 1000, 2e-5  # twice the project's score tolerance: two fp32 scores are being compared
    oq, oc, os_ = oracle.selfjoin_pairs(A_DIM, A_THETA - cut, a["rp"], a["idx"], a["val"])
    t = np.sort(os_[os_ >= A_THETA])[::-1][K - 1]
    orc = {(int(x), int(y)): float(v) for x, y, v in zip(oq, oc, os_)}
    with ApssIndex(A_DIM, A_THETA, tile_rows=512, top_pairs=K) as ix:
        ix.insert(a["ext"], a["rp"], a["idx"], a["val"])
        assert ix.self_join(fetch=False) == K
        q, c, s = device_list(ix)
    got = {(int(x), int(y)): float(v) for x, y, v in zip(q, c, s)}
    assert len(got) == K
    for pair, v in got.items():
        assert pair in orc and abs(orc[pair] - v) <= TOL and orc[pair] >= t - cut, (pair, v)
    assert all(pair in got for pair, v in orc.items() if v > t + cut)


# ---- 8. the host mirror: cpslab.allpair.gpu.topPairs
def test_host_mirror_top_pairs():
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(HOST, "host_top_pairs_selftest")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "host_top_pairs_selftest: PASS" in out.stdout
