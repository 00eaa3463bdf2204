"""Removal of stored vectors on the device (apss_remove / apss_compact / apss_set_auto_compact, csrc/apss_remove.hpp) against the
double-precision oracle: the expected answer of a call is the oracle's list for the whole history with every pair that touches a
removed row deleted in numpy (tests/remove_shape.py).  Every test asserts the oracle-side counts it stands on first, so that
none can pass on an empty list: at least 20 dropped and 50 kept pairs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import remove_shape as rs
from apss import _lib
from apss.engine import ApssError, ApssIndex
from helpers import BAND, assert_same_pairs, to_map
from store_view import read_store
from test_gpu_topk import check_topk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "all-pairs-similarity_amd", "host")
S, N, DIM, R = rs.STORED, rs.N, rs.DIM, rs.R


def floors(want, dropped):
    assert dropped >= 20 and len(want) >= 50, (len(want), dropped)


def batch_expectation(oracle, theta, zipf=0.0, frozen=False):
    """insert rows 0 .. 1999, remove R, then rows 2000 .. 2999 as a query-insert (or as a frozen query: the batch does not see
    itself)"""
    orc = rs.whole_join(oracle, theta, zipf, S)
    visible = orc[1] < S if frozen else np.ones(orc[0].size, bool)
    return orc, rs.split(orc, theta, visible, ~rs.IS_R[orc[1]])


def stored_then_removed(ix, v):
    ix.insert(rs.IDS[:S], *rs.rows_of(v, 0, S))
    assert ix.remove(R) == R.size
    info = ix.removal_info()
    assert info["rows_removed"] == R.size and info["rows_live"] == S - R.size and info["removed_total"] == R.size
    assert ix.size()[0] == S  # physical rows


# ---- 1. every path of a query-type call
PATHS = {
    "plain": dict(theta=0.5),
    "exact_accum": dict(theta=0.5, flags=_lib.FLAG_EXACT_ACCUM),
    "force_scan": dict(theta=0.5, flags=_lib.FLAG_FORCE_SCAN),
    "theta_zero": dict(theta=0.0),
    "dense_head": dict(theta=0.5, zipf=1.0, head_terms=64),
    "frozen_query": dict(theta=0.5, frozen=True),
    "ids_on_device": dict(theta=0.5, dev=True),
}


@pytest.mark.parametrize("path", list(PATHS))
def test_paths(oracle, path):
    p = PATHS[path]
    theta, zipf, frozen = p["theta"], p.get("zipf", 0.0), p.get("frozen", False)
    _, (_, want, dropped, band) = batch_expectation(oracle, theta, zipf, frozen)
    if path in ("plain", "exact_accum", "force_scan", "ids_on_device"):
        assert (len(want) + dropped, dropped) == (125, 30)
    if path == "theta_zero":
        assert (len(want) + dropped, dropped) == (1098144, 266143)
    floors(want, dropped)
    v = rs.vectors(zipf)
    with ApssIndex(DIM, theta, tile_rows=rs.TILE, flags=p.get("flags", 0), head_terms=p.get("head_terms", 0)) as ix:
        if p.get("dev"):
            import torch
            ix.insert(rs.IDS[:S], *rs.rows_of(v, 0, S))
            assert ix.remove(torch.from_numpy(R).cuda()) == R.size
        else:
            stored_then_removed(ix, v)
        call = ix.query if frozen else ix.insert_and_query
        got = call(rs.IDS[S:], *rs.rows_of(v, S, N))
        info, st = ix.removal_info(), ix.stats()
    print(path, "kept", len(got[0]), "dropped", info["pairs_dropped"], "oracle", len(want), dropped, "band", band,
          "drop_ms %.3f probe_ms %.3f" % (info["drop_ms"], st["probe_ms"]), st["probe_kernel"])
    assert_same_pairs(to_map(*got), want, theta)
    assert abs(info["pairs_dropped"] - dropped) <= band
    assert info["drop_launches"] == 1 and st["result_pairs"] == len(got[0])
    if path == "dense_head":
        assert st["head_terms"] == 64
    if path == "theta_zero":
        assert info["pairs_dropped"] == dropped and len(got[0]) == len(want)


# ---- 2. a self-join: removed QUERY rows drop out too, on the symmetric join's mirrored half as well
def test_self_join_drops_both_ends(oracle):
    theta = 0.5
    orc = rs.whole_join(oracle, theta)
    visible = (orc[0] < S) & (orc[1] < S)
    _, want, dropped, band = rs.split(orc, theta, visible, ~rs.IS_R[orc[0]] & ~rs.IS_R[orc[1]])
    assert (len(want) + dropped, dropped, len(want)) == (376, 272, 104)
    floors(want, dropped)
    with ApssIndex(DIM, theta, tile_rows=rs.TILE) as ix:
        stored_then_removed(ix, rs.vectors())
        got = ix.self_join()
        st, info = ix.stats(), ix.removal_info()
    assert st["symmetric"] == 1
    assert_same_pairs(to_map(*got), want, theta)
    assert not (rs.IS_R[got[0]].any() or rs.IS_R[got[1]].any())
    assert abs(info["pairs_dropped"] - dropped) <= band and st["result_pairs"] == len(got[0])


# ---- 3. top-k: the drop runs before the cut
def first3_removed(orc, theta):
    """query rows whose first 3 pairs >= theta, by (score descending, candidate ascending), hold a removed candidate"""
    oq, oc, os_ = (a[orc[2] >= theta] for a in orc)
    order = np.lexsort((oc, -os_, oq))
    oq, oc = oq[order], oc[order]
    rank = np.arange(oq.size) - np.searchsorted(oq, oq)
    return int(np.unique(oq[(rank < 3) & rs.IS_R[oc]]).size)


@pytest.mark.parametrize("theta", [0.1, 0.0])
def test_topk_keeps_the_best_live_pairs(oracle, theta):
    k = 3
    orc, (live, want, dropped, band) = batch_expectation(oracle, theta)
    assert (len(want) + dropped, dropped) == {0.1: (35376, 8510), 0.0: (1098144, 266143)}[theta]
    assert first3_removed(orc, theta) == 547
    floors(want, dropped)
    cnt_certain = np.bincount(live[0][live[2] >= theta + BAND] - S, minlength=N - S)
    cnt_possible = np.bincount(live[0][live[2] >= theta - BAND] - S, minlength=N - S)
    assert cnt_certain.min() > k  # every row has more than 3 live pairs
    v = rs.vectors()
    lists = {}
    variants = ["plain"] if theta > 0 else ["plain", "tile_cut", "window"]
    for variant in variants:
        with ApssIndex(DIM, theta, tile_rows=rs.TILE, top_k=k, top_k_tile_cut=variant == "tile_cut",
                       top_k_window=300000 if variant == "window" else 0) as ix:
            stored_then_removed(ix, v)
            got = ix.insert_and_query(rs.IDS[S:], *rs.rows_of(v, S, N))
            tk, ci, wi, ri = ix.topk_info(), ix.topk_tile_cut_info(), ix.topk_window_info(), ix.removal_info()
        print(theta, variant, tk, ci, ri)
        check_topk(got, live, k, theta, rs.IDS[S:])
        assert len(got[0]) == (N - S) * k == tk["kept"]
        assert int(cnt_certain.sum()) <= tk["pairs_over_theta"] <= int(cnt_possible.sum())
        assert tk["queries_cut"] == N - S
        assert int(cnt_certain.max()) <= tk["longest_segment"] <= int(cnt_possible.max())
        assert abs(ri["pairs_dropped"] - dropped) <= band
        if variant == "tile_cut":
            assert ci["declined"] == _lib.TILE_CUT_REMOVED and ci["applied"] == 0
        if variant == "window":
            assert wi["windows"] >= 3 and ri["drop_launches"] == wi["windows"]
        lists[variant] = got
    for variant in variants[1:]:  # element by element the list without the setting
        for a, b in zip(lists[variant], lists["plain"]):
            assert np.array_equal(a, b), variant


# ---- 4. the mark belongs to the slot, not to the id
def test_the_mark_is_the_slots(oracle):
    theta = 0.5
    v = rs.vectors()
    orc = rs.whole_join(oracle, theta)
    data = np.array([5, 600, 2000, 2001])  # the query batch: the two removed rows' vectors and the two new ones
    q_ids = np.array([9005, 9600, 9000, 9001], dtype=np.int64)
    id_of = {int(d): int(i) for d, i in zip(data, q_ids)}
    ext_of = lambda c: {2000: 5, 2001: 600}.get(int(c), int(c))  # noqa: E731

    def expectation(dead):
        want = {}
        for a, b, s in zip(*orc):
            if int(a) in id_of and s >= theta and (b < S or b in (2000, 2001)) and int(b) not in dead:
                want[(id_of[int(a)], ext_of(b))] = float(s)
        for d in (2000, 2001):  # a query's own vector is stored under another id: found, score 1
            if d not in dead:
                want[(id_of[d], ext_of(d))] = 1.0
        return want

    rp = np.concatenate([[0], np.cumsum([v[0][d + 1] - v[0][d] for d in data])]).astype(np.int64)
    idx = np.concatenate([v[1][v[0][d]:v[0][d + 1]] for d in data])
    val = np.concatenate([v[2][v[0][d]:v[0][d + 1]] for d in data])
    with ApssIndex(DIM, theta, tile_rows=rs.TILE) as ix:
        ix.insert(rs.IDS[:S], *rs.rows_of(v, 0, S))
        assert ix.remove([5, 600]) == 2
        ix.insert(np.array([5, 600], dtype=np.int64), *rs.rows_of(v, 2000, 2002))
        assert ix.size()[0] == S + 2
        got = to_map(*ix.query(q_ids, rp, idx, val))
        want = expectation({5, 600})
        assert_same_pairs(got, want, theta)
        assert abs(got[(9000, 5)] - 1.0) <= 1e-5 and abs(got[(9001, 600)] - 1.0) <= 1e-5  # the new rows are found
        assert got.get((9005, 5), 0.0) < 0.999 and got.get((9600, 600), 0.0) < 0.999      # the old ones are not
        assert ix.remove([5]) == 1          # only the new row under id 5 was live
        assert ix.remove([123456]) == 0     # an id that is not stored
        assert ix.remove([5, 600, 600]) == 1
        assert ix.removal_info()["rows_removed"] == 4
        got = to_map(*ix.query(q_ids, rp, idx, val))
        assert_same_pairs(got, expectation({5, 600, 2000, 2001}), theta)
        assert (9000, 5) not in got and (9001, 600) not in got


# ---- 5. compaction: the store of a handle that was only ever given the live rows, bit for bit
def test_compaction(oracle):
    theta, flags = 0.5, _lib.FLAG_NORMALIZE
    _, (_, want, dropped, _) = batch_expectation(oracle, theta)
    floors(want, dropped)
    v = rs.vectors()
    live_rows = np.nonzero(~rs.IS_R[:S])[0]
    lrp = np.concatenate([[0], np.cumsum(np.diff(v[0])[live_rows])]).astype(np.int64)
    lidx = np.concatenate([v[1][v[0][r]:v[0][r + 1]] for r in live_rows])
    lval = np.concatenate([v[2][v[0][r]:v[0][r + 1]] for r in live_rows])
    with ApssIndex(DIM, theta, tile_rows=rs.TILE, flags=flags) as fresh:
        fresh.insert(rs.IDS[live_rows], lrp, lidx, lval)
        ref = read_store(fresh)
        fresh_stats = fresh.stats()
    with ApssIndex(DIM, theta, tile_rows=rs.TILE, flags=flags) as ix:
        ix.insert(rs.IDS[:S], *rs.rows_of(v, 0, S))
        ix.self_join(fetch=False)
        assert ix.remove(R) == R.size
        assert ix.result_count() > 0  # a removal leaves the last results alone
        ix.compact()
        assert ix.size() == (S - R.size, int(lrp[-1])) and S - R.size == 1274
        got = read_store(ix)
        assert np.array_equal(got.rowptr, ref.rowptr) and np.array_equal(got.indices, ref.indices)
        assert np.array_equal(got.values.view(np.uint32), ref.values.view(np.uint32)) and np.array_equal(got.ext_ids, ref.ext_ids)
        with pytest.raises(ApssError) as e:
            ix.fetch()
        assert e.value.code == _lib.E_STATE
        assert ix.stats()["tiles"] == fresh_stats["tiles"]
        info = ix.removal_info()
        assert (info["rows_removed"], info["rows_live"], info["compactions"], info["compacted_rows"]) == (0, 1274, 1, R.size)
        assert info["compact_ms"] > 0
        pairs = ix.insert_and_query(rs.IDS[S:], *rs.rows_of(v, S, N))
        assert_same_pairs(to_map(*pairs), want, theta)
        assert ix.removal_info()["drop_launches"] == 0  # nothing is marked any more
        ix.compact()  # nothing marked: a no-op that keeps the last results
        again = ix.fetch()
        assert all(np.array_equal(a, b) for a, b in zip(pairs, again))
        assert ix.removal_info()["compactions"] == 1 and ix.size()[0] == 1274 + N - S


# ---- 6. a sliding stream with auto-compaction
def test_sliding_stream(oracle):
    theta, B, f = 0.5, 250, 0.25
    orc = rs.whole_join(oracle, theta)
    oq, oc, os_ = orc
    v = rs.vectors()
    wants, kept_total, dropped_total = [], 0, 0
    for i in range(N // B):
        visible = (oq >= i * B) & (oq < (i + 1) * B) & (oc < (i + 1) * B)
        _, want, dropped, band = rs.split(orc, theta, visible, oc >= (i - 3) * B)  # batches 0 .. i - 4 were removed
        assert band == 0
        wants.append(want)
        kept_total += len(want)
        dropped_total += dropped
    assert (kept_total, dropped_total) == (251, 97)
    seen_dropped = 0
    with ApssIndex(DIM, theta, tile_rows=rs.TILE, auto_compact=f) as ix:
        assert ix.removal_info()["auto_compact"] == f
        for i in range(N // B):
            info = ix.removal_info()
            assert info["rows_removed"] <= 4 * B and info["rows_live"] <= 4 * B
            got = ix.insert_and_query(rs.IDS[i * B:(i + 1) * B], *rs.rows_of(v, i * B, (i + 1) * B))
            assert_same_pairs(to_map(*got), wants[i], theta)
            info = ix.removal_info()
            seen_dropped += info["pairs_dropped"]
            rows = ix.size()[0]
            assert rows <= 1583, (i, rows)  # 1000 / 0.75 + 250
            assert info["rows_removed"] <= f * (rows - B) + 1e-9, (i, info)  # before the insert at most a quarter was marked
            if i >= 3:
                assert ix.remove(rs.IDS[(i - 3) * B:(i - 2) * B]) == B
        info = ix.removal_info()
    print("stream:", info, "dropped", seen_dropped)
    assert info["compactions"] >= 1 and info["removed_total"] == N - 3 * B
    assert seen_dropped <= dropped_total  # (pairs with a row that a compaction discarded are never found at all)


# ---- 7. no removal costs nothing
def test_no_removal_costs_nothing():
    v = rs.vectors()
    stats = []
    for touched in (False, True):
        with ApssIndex(DIM, 0.5, tile_rows=rs.TILE) as ix:
            if touched:
                assert ix.remove([]) == 0
                ix.set_auto_compact(0.5)
            ix.insert_and_query(rs.IDS[:1000], *rs.rows_of(v, 0, 1000))
            if touched:
                info = ix.removal_info()
                assert info["drop_launches"] == 0 and info["pairs_dropped"] == 0 and info["compactions"] == 0
                assert ix.topk_tile_cut_info()["declined"] == _lib.TILE_CUT_OFF
            stats.append(ix.stats())
    times = ("probe_ms", "build_ms", "rescore_ms", "head_ms")
    for key in stats[0]:
        if key not in times:
            assert stats[0][key] == stats[1][key], key
    assert stats[0]["result_pairs"] > 0


# ---- 8. refusals
def test_refusals():
    v = rs.vectors()
    import torch
    with ApssIndex(DIM, 0.5, tile_rows=rs.TILE, term_range=(0, DIM // 2)) as shard:
        calls = [lambda: shard.remove([1]), lambda: shard.remove(torch.zeros(1, dtype=torch.int64, device="cuda")), shard.compact,
                 lambda: shard.set_auto_compact(0.1), shard.removal_info]
        for call in calls:
            with pytest.raises(ApssError) as e:
                call()
            assert e.value.code == _lib.E_UNSUPPORTED and "term shard" in str(e.value)
        shard.insert_and_query(rs.IDS[:500], *rs.rows_of(v, 0, 500))  # the handle works afterwards
        assert shard.size()[0] == 500
    with ApssIndex(DIM, 0.5, tile_rows=rs.TILE) as ix:
        ix.insert(rs.IDS[:500], *rs.rows_of(v, 0, 500))
        one = np.zeros(1, np.int64)
        n = C.c_int64(7)
        assert ix._L.apss_remove(ix._h, -1, C.c_void_p(one.ctypes.data), C.byref(n)) == _lib.E_INVALID
        assert ix._L.apss_remove(ix._h, 1, None, None) == _lib.E_INVALID
        assert ix._L.apss_remove_dev(ix._h, -1, None, None) == _lib.E_INVALID
        assert ix._L.apss_remove_dev(ix._h, 1, None, None) == _lib.E_INVALID
        for bad in (1.0, -0.1, 2.0, float("nan")):
            with pytest.raises(ApssError) as e:
                ix.set_auto_compact(bad)
            assert e.value.code == _lib.E_INVALID
        assert ix.removal_info()["auto_compact"] == 0.0
        assert ix.remove([3]) == 1 and ix._L.apss_remove(ix._h, 1, C.c_void_p(one.ctypes.data), None) == _lib.OK  # NULL count
        assert ix.removal_info()["rows_removed"] == 2
        assert ix.self_join(fetch=False) >= 0


# ---- 9. the host mirror
def test_host_mirror_remove():
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(HOST, "host_remove_selftest")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "host_remove_selftest: PASS" in out.stdout
