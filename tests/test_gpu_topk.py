"""Per-query top-k on the device (apss_set_top_k, csrc/apss_topk.hpp) against the double-precision oracle.

The comparison rule (check_topk): for a query with oracle scores sorted descending let t be the k-th (theta if there are fewer
than k).  The device's list for that query must contain every oracle pair with score > t + 2e-5, no pair whose oracle score is
< t - 2e-5, exactly min(k, count) pairs (count allowed the usual +-(pairs inside |score - theta| <= 1e-5)), and every reported
score within 1e-5 of the oracle's.  2e-5 is twice the project's score tolerance: two fp32 scores are being compared.  The
oracle is run at theta - 2e-5 so that it knows the pairs just below the threshold too."""
import os
import subprocess

import numpy as np
import pytest

from apss import _lib, synth
from apss.engine import ApssError, ApssGroup, ApssIndex
from helpers import BAND, TOL, assert_same_pairs, to_map

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "all-pairs-similarity_amd", "host")
CUT = 2e-5
LOWER = 2e-5  # the oracle's threshold is this much below the device's

A_N, A_DIM, A_THETA = 1500, 300, 0.45
A_CUT = {1: 1378, 3: 1236, 8: 981, 64: 211, 1024: 0}  # query rows of shape A with more than k pairs (oracle, counted on the CPU)
A_LONGEST = 277
A_PAIRS = 45562


def check_topk(got, orc, k, theta, query_ids):
    """got: (q ids, c ids, scores) as fetched; orc: the oracle's triples at theta - LOWER; query_ids: the batch's ids in row order"""
    gq, gc, gs = (np.asarray(a) for a in got)
    oq, oc, os_ = (np.asarray(a) for a in orc)
    order = np.lexsort((oc, oq))
    oq, oc, os_ = oq[order], oc[order], os_[order]
    # output order: grouped by query row ascending, rank order inside a row
    row_of = {int(v): i for i, v in enumerate(query_ids)}
    rows = np.array([row_of[int(v)] for v in gq], dtype=np.int64)
    assert np.all(np.diff(rows) >= 0), "the list is not grouped by query row ascending"
    starts = np.searchsorted(rows, np.arange(len(query_ids) + 1))
    for r, qid in enumerate(query_ids):
        c, s = gc[starts[r]:starts[r + 1]], gs[starts[r]:starts[r + 1]].astype(np.float64)
        lo, hi = np.searchsorted(oq, qid), np.searchsorted(oq, qid, side="right")
        ocq, osq = oc[lo:hi], os_[lo:hi]
        certain, possible = int((osq >= theta + BAND).sum()), int((osq >= theta - BAND).sum())
        assert min(k, certain) <= len(c) <= min(k, possible), (qid, len(c), certain, possible)
        over = np.sort(osq[osq >= theta])[::-1]
        t = over[k - 1] if len(over) >= k else theta
        if len(c):
            assert np.all(np.diff(s) <= 0), ("scores of one query must not ascend", qid)
            ties = np.diff(s) == 0
            assert np.all(np.diff(c)[ties] > 0), ("equal scores are ordered by candidate id", qid)
            pos = np.searchsorted(ocq, c)
            assert np.all(pos < len(ocq)) and np.all(ocq[np.minimum(pos, len(ocq) - 1)] == c), ("pair unknown to the oracle", qid)
            assert np.abs(osq[pos] - s).max() <= TOL, (qid, np.abs(osq[pos] - s).max())
            assert osq[pos].min() >= t - CUT, (qid, osq[pos].min(), t)
        must = ocq[osq > t + CUT]
        assert np.isin(must, c).all(), (qid, "a pair clearly above the cut is missing")


def rows_of(rp, idx, val, a, b):
    return rp[a:b + 1] - rp[a], idx[rp[a]:rp[b]], val[rp[a]:rp[b]]


@pytest.fixture(scope="module")
def shape_a(oracle):
    rp, idx, val = synth.make_vectors(A_N, A_DIM, 12, 1.0, seed=21, dup_frac=0.1)
    ids = np.arange(A_N, dtype=np.int64) + 100
    oq, oc, os_ = oracle.selfjoin_pairs(A_DIM, A_THETA - LOWER, rp, idx, val)
    orc = (oq + 100, oc + 100, os_)
    cnt = np.bincount(oq[os_ >= A_THETA], minlength=A_N)
    assert int((os_ >= A_THETA).sum()) == A_PAIRS and int(cnt.max()) == A_LONGEST and int((cnt == 0).sum()) == 54
    assert {k: int((cnt > k).sum()) for k in A_CUT} == A_CUT
    return dict(rp=rp, idx=idx, val=val, ids=ids, orc=orc, certain=int((os_ >= A_THETA + BAND).sum()),
                possible=int((os_ >= A_THETA - BAND).sum()))


# ---- 1. parity on shape A: three tiles, three probe paths, segments shorter than / equal to / longer than k, and empty ones
@pytest.mark.parametrize("flags", [0, _lib.FLAG_EXACT_ACCUM, _lib.FLAG_FORCE_GENERAL], ids=["default", "exact_accum", "general"])
@pytest.mark.parametrize("k", [1, 3, 8, 64, 1024])
def test_parity_shape_a(shape_a, flags, k):
    a = shape_a
    with ApssIndex(A_DIM, A_THETA, tile_rows=512, flags=flags, top_k=k) as ix:
        got = ix.insert_and_query(a["ids"], a["rp"], a["idx"], a["val"])
        info, st = ix.topk_info(), ix.stats()
        assert ix.result_count() == len(got[0])
    check_topk(got, a["orc"], k, A_THETA, a["ids"])
    print("shape A k=%d flags=%d: %s" % (k, flags, info))
    assert info["k"] == k and info["select_launches"] > 0 and info["select_ms"] > 0
    assert a["certain"] <= info["pairs_over_theta"] <= a["possible"]
    assert info["kept"] == len(got[0]) == st["result_pairs"]
    assert info["queries_cut"] == A_CUT[k]
    assert info["longest_segment"] == A_LONGEST
    if k == 1024:  # nothing is cut: the k = 0 set
        assert_same_pairs(to_map(*got), {kk: v for kk, v in to_map(*a["orc"]).items() if v >= A_THETA}, A_THETA)


# ---- 2. theta <= 0: every query is cut, segments of more than 1024 pairs; then signed scores through the key
@pytest.fixture(scope="module")
def shape_zero(oracle):
    rp, idx, val = synth.make_vectors(2000, 64, 8, 0.0, seed=5, dup_frac=0.1)
    orc = oracle.selfjoin_pairs(64, 0.0 - LOWER, rp, idx, val)
    assert len(orc[0]) == 2710116 and int(np.bincount(orc[0]).max()) == 1431
    sign = np.where(np.random.Generator(np.random.PCG64(9)).random(val.size) < 0.5, -1.0, 1.0)
    orc_signed = oracle.selfjoin_pairs(64, -0.2 - LOWER, rp, idx, val * sign)
    return dict(rp=rp, idx=idx, val=val, ids=np.arange(2000, dtype=np.int64), orc=orc, val_signed=val * sign, orc_signed=orc_signed)


@pytest.mark.parametrize("k", [1, 8, 64])
def test_theta_zero(shape_zero, k):
    z = shape_zero
    with ApssIndex(64, 0.0, top_k=k) as ix:
        got = ix.insert_and_query(z["ids"], z["rp"], z["idx"], z["val"])
        info = ix.topk_info()
    check_topk(got, z["orc"], k, 0.0, z["ids"])
    print("theta 0 k=%d: %s" % (k, info))
    assert info["pairs_over_theta"] == 2710116 and info["queries_cut"] == 2000 and info["longest_segment"] == 1431
    assert info["kept"] == 2000 * k


@pytest.mark.parametrize("k", [1, 8, 64])
def test_negative_scores(shape_zero, k):
    z = shape_zero
    with ApssIndex(64, -0.2, top_k=k) as ix:
        got = ix.insert_and_query(z["ids"], z["rp"], z["idx"], z["val_signed"])
        full = ix.topk_info()["pairs_over_theta"]
    check_topk(got, z["orc_signed"], k, -0.2, z["ids"])
    assert full > len(got[0]) > 0


# ---- 3. exact order: the k = 8 list equals the k = 0 list sorted by (query row, -score, candidate ext id, slot) and cut
def _device_list(ix):
    import torch
    _, _, _, n = ix.results_dev()
    q = torch.empty(n, dtype=torch.int32, device="cuda")
    c = torch.empty(n, dtype=torch.int32, device="cuda")
    s = torch.empty(n, dtype=torch.float32, device="cuda")
    if n:
        ix.results_to(q, c, s)
    torch.cuda.synchronize()
    return q.cpu().numpy(), c.cpu().numpy(), s.cpu().numpy()


def test_exact_order_on_one_handle(shape_a):
    a = shape_a
    ext = 5000 - np.arange(A_N, dtype=np.int64)  # external ids DESCEND with the slot: id order and slot order disagree
    with ApssIndex(A_DIM, A_THETA, tile_rows=512) as ix:
        ix.insert(ext, a["rp"], a["idx"], a["val"])
        ix.self_join(fetch=False)
        q0, c0, s0 = _device_list(ix)
        ix.set_top_k(8)
        assert ix.result_count() == len(q0)  # changing the setting leaves the last call's results alone
        ix.self_join(fetch=False)
        q1, c1, s1 = _device_list(ix)
    order = np.lexsort((c0, ext[c0], -s0.astype(np.float64), q0))
    q0, c0, s0 = q0[order], c0[order], s0[order]
    first = np.searchsorted(q0, q0)  # index of each row's first pair
    keep = np.arange(len(q0)) - first < 8
    assert np.array_equal(q1, q0[keep]) and np.array_equal(c1, c0[keep])
    assert np.array_equal(s1.view(np.uint32), s0[keep].view(np.uint32))


# ---- 4. planted ties across the cut: 40 identical rows, every copy sees 39 candidates at one top score
def test_planted_ties_across_the_cut(shape_a):
    a = shape_a
    src = 7
    r0, r1 = a["rp"][src], a["rp"][src + 1]
    copies = 39  # + the row itself = 40 identical rows
    rp = np.concatenate([a["rp"], a["rp"][-1] + (r1 - r0) * np.arange(1, copies + 1)])
    idx = np.concatenate([a["idx"]] + [a["idx"][r0:r1]] * copies)
    val = np.concatenate([a["val"]] + [a["val"][r0:r1]] * copies)
    copy_ids = 90000 + np.random.Generator(np.random.PCG64(3)).permutation(copies).astype(np.int64)  # not in slot order
    ids = np.concatenate([a["ids"], copy_ids])
    same = np.concatenate([[a["ids"][src]], copy_ids])
    with ApssIndex(A_DIM, A_THETA, tile_rows=512, top_k=8) as ix:
        q, c, s = ix.insert_and_query(ids, rp, idx, val)
    for qid in same:
        mine = q == qid
        assert mine.sum() == 8, (qid, mine.sum())
        want = np.sort(same[same != qid])[:8]
        assert np.array_equal(c[mine], want), (qid, c[mine], want)
        assert np.all(s[mine] == s[mine][0]) and abs(float(s[mine][0]) - 1.0) <= TOL


# ---- 5. one long segment, streamed from global memory per digit pass (k_topk_select's radix select): 70,000 > 1024 pairs
@pytest.fixture(scope="module")
def long_store():
    n, dim = 70000, 4096
    rng = np.random.Generator(np.random.PCG64(17))

    def rows(m):
        w = (dim - 1) // 3  # one random term from each third of [1, dim): distinct and ascending by construction
        other = 1 + np.arange(3)[None, :] * w + rng.integers(0, w, size=(m, 3))
        idx = np.concatenate([np.zeros((m, 1), np.int64), other], axis=1).astype(np.int32)
        val = rng.random((m, 4)) + 0.05
        val /= np.linalg.norm(val, axis=1, keepdims=True)
        return np.arange(m + 1, dtype=np.int64) * 4, idx.ravel(), val.ravel()

    rp, idx, val = rows(n)
    qrp, qidx, qval = rows(4)
    import scipy.sparse as sp
    x = sp.csr_matrix((val, idx, rp), shape=(n, dim), dtype=np.float64)
    qm = sp.csr_matrix((qval, qidx, qrp), shape=(4, dim), dtype=np.float64)
    scores = np.asarray((qm @ x.T).todense())  # every pair shares term 0
    keep = scores >= 0.05 - LOWER
    oq, oc = np.nonzero(keep)
    orc = (oq.astype(np.int64) + 1000000, oc.astype(np.int64), scores[keep])
    return dict(n=n, dim=dim, store=(rp, idx, val), query=(qrp, qidx, qval), orc=orc,
                longest=(int((scores >= 0.05 + BAND).sum(axis=1).max()), int((scores >= 0.05 - BAND).sum(axis=1).max())))


@pytest.mark.parametrize("k", [1, 10, 1024])
def test_one_long_segment(long_store, k):
    ls = long_store
    assert ls["longest"][0] > 60000
    qids = np.arange(4, dtype=np.int64) + 1000000
    with ApssIndex(ls["dim"], 0.05, head_terms=-1, top_k=k) as ix:
        ix.insert(np.arange(ls["n"], dtype=np.int64), *ls["store"])
        got = ix.query(qids, *ls["query"])
        info = ix.topk_info()
    check_topk(got, ls["orc"], k, 0.05, qids)
    print("long segment k=%d: %s" % (k, info))
    assert len(got[0]) == 4 * k and info["queries_cut"] == 4
    assert ls["longest"][0] <= info["longest_segment"] <= ls["longest"][1]  # (pairs inside the threshold band)


# ---- 6. edges
def test_edges(shape_a):
    a = shape_a
    with ApssIndex(A_DIM, A_THETA, tile_rows=512) as ix:
        ix.set_top_k(3)
        for bad in (1025, -1):
            with pytest.raises(ApssError) as e:
                ix.set_top_k(bad)
            assert e.value.code == _lib.E_INVALID and "1024" in str(e.value)
        ix.insert(a["ids"], a["rp"], a["idx"], a["val"])
        # nq = 0
        q, c, s = ix.query(np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0))
        assert len(q) == 0 and ix.topk_info()["kept"] == 0
        # a batch that matches nothing (a term no stored row's neighbourhood reaches the threshold with)
        q, c, s = ix.query(np.array([7], np.int64), np.array([0, 1], np.int64), np.array([5], np.int32), np.array([1e-6]))
        assert len(q) == 0 and ix.result_count() == 0
        assert ix._L.apss_fetch_results(ix._h, 0, 0, None, None, None) == _lib.OK
        got3 = ix.self_join()
        assert ix.topk_info()["k"] == 3 and len(got3[0]) < A_PAIRS
        ix.set_top_k(0)
        full = ix.self_join()
        assert_same_pairs(to_map(*full), {kk: v for kk, v in to_map(*a["orc"]).items() if v >= A_THETA}, A_THETA)
        assert ix.topk_info()["k"] == 0 and ix.topk_info()["kept"] == len(full[0])
        # the setting survives clear
        ix.set_top_k(3)
        ix.clear()
        again = ix.insert_and_query(a["ids"], a["rp"], a["idx"], a["val"])
        check_topk(again, a["orc"], 3, A_THETA, a["ids"])
    with ApssIndex(A_DIM, A_THETA, term_range=(0, A_DIM // 2)) as shard:
        with pytest.raises(ApssError) as e:
            shard.set_top_k(3)
        assert e.value.code == _lib.E_UNSUPPORTED and "term shard" in str(e.value)
        shard.set_top_k(0)


# ---- 7. streams: three batches of 500, every batch sees itself and everything before it (rows waiting in the tail included)
def test_streamed_batches(shape_a, oracle):
    a = shape_a
    w = oracle.Worker(A_DIM, A_THETA - LOWER)
    with ApssIndex(A_DIM, A_THETA, tile_rows=512, top_k=3) as ix:
        for b in range(3):
            lo, hi = 500 * b, 500 * (b + 1)
            rp, idx, val = rows_of(a["rp"], a["idx"], a["val"], lo, hi)
            got = ix.insert_and_query(a["ids"][lo:hi], rp, idx, val)
            orc = w.index_data(a["ids"][lo:hi], rp, idx, val)
            check_topk(got, orc, 3, A_THETA, a["ids"][lo:hi])
            assert len(got[0]) > 500
    w.close()


# ---- 8. regrowth: the result list overflows and the probe re-runs; the pass runs once, on the final list
def test_regrowth_runs_one_pass(shape_a, monkeypatch):
    a = shape_a
    with ApssIndex(A_DIM, A_THETA, tile_rows=512, top_k=3) as ix:
        plain = ix.insert_and_query(a["ids"], a["rp"], a["idx"], a["val"])
        info0, st0 = ix.topk_info(), ix.stats()
    monkeypatch.setenv("APSS_DEBUG", "res_cap=256")
    with ApssIndex(A_DIM, A_THETA, tile_rows=512, top_k=3) as ix:
        small = ix.insert_and_query(a["ids"], a["rp"], a["idx"], a["val"])
        info1, st1 = ix.topk_info(), ix.stats()
    assert st1["probe_launches"] > st0["probe_launches"]  # the hook did make the probe run again
    for x, y in zip(plain, small):
        assert np.array_equal(x, y)
    assert info1["select_launches"] == info0["select_launches"] > 0
    assert info1["pairs_over_theta"] == info0["pairs_over_theta"] and info1["kept"] == info0["kept"]


# ---- 9. k = 0 costs nothing
def test_k_zero_costs_nothing(shape_a):
    a = shape_a
    stats = []
    for touched in (False, True):
        with ApssIndex(A_DIM, A_THETA, tile_rows=512) as ix:
            if touched:
                ix.set_top_k(3)
                ix.set_top_k(0)
            ix.insert_and_query(a["ids"], a["rp"], a["idx"], a["val"])
            info = ix.topk_info()
            assert info["select_launches"] == 0 and info["select_ms"] == 0 and info["k"] == 0
            assert info["pairs_over_theta"] == info["kept"] == ix.result_count()
            stats.append(ix.stats())
    timing = {"probe_ms", "build_ms", "rescore_ms", "head_ms"}
    for key in stats[0]:
        if key not in timing:
            assert stats[0][key] == stats[1][key], key


# ---- 10. groups: the cut behind the exchange, in the one member's handle, and refused on a grid
@pytest.mark.parametrize("devices,gflags", [([0, 0, 0], 0), ([0], _lib.GROUP_FORCE_EXCHANGE), ([0], 0)],
                         ids=["three_members", "one_member_exchange", "one_member_plain"])
def test_group(shape_a, devices, gflags):
    a = shape_a
    with ApssGroup(A_DIM, A_THETA, devices, tile_rows=512, group_flags=gflags, top_k=3) as g:
        got = g.insert_and_query(a["ids"], a["rp"], a["idx"], a["val"])
        info, st = g.topk_info(), g.stats()
    check_topk(got, a["orc"], 3, A_THETA, a["ids"])
    assert info["k"] == 3 and info["kept"] == len(got[0]) == st["result_pairs"]
    assert a["certain"] <= info["pairs_over_theta"] <= a["possible"]
    assert info["queries_cut"] == A_CUT[3] and info["longest_segment"] == A_LONGEST and info["select_launches"] > 0


def test_grid_refuses_and_keeps_working(shape_a):
    a = shape_a
    with ApssGroup(A_DIM, A_THETA, [0, 0, 0, 0], tile_rows=512, row_ranges=2) as g:
        with pytest.raises(ApssError) as e:
            g.set_top_k(3)
        assert e.value.code == _lib.E_UNSUPPORTED and "row range" in str(e.value)
        got = g.insert_and_query(a["ids"], a["rp"], a["idx"], a["val"])
        assert g.topk_info()["k"] == 0
    assert_same_pairs(to_map(*got), {kk: v for kk, v in to_map(*a["orc"]).items() if v >= A_THETA}, A_THETA)


# ---- 11. the host mirror: cpslab.allpair.gpu.topK
def test_host_mirror_topk():
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(HOST, "host_topk_selftest")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "host_topk_selftest: PASS" in out.stdout
