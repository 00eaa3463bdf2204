"""Near-duplicate groups across a removal and a compaction (apss_set_components_repair, csrc/apss_components_repair.hpp): a remove
re-joins the components it touched, a compaction renumbers the forest, and in both the labels stay those of a fresh self-join
over the live rows -- without a second self-join.

The reference of every label check is the CPU union-find of tests/test_gpu_components.py over the float64 oracle's pairs whose
two ends are live; the slots of the dead set get -1.  Where theta > 0 the fixtures keep that file's guard: no oracle score within
100 x BAND of theta, so fp32 and float64 agree about every pair.  At theta = 0 with positive weights a pair is a result exactly when
its rows share a term -- every such score is > 0 in both precisions -- and the guard is that every oracle score is positive."""
import ctypes

import numpy as np
import pytest

from apss import _lib, synth
from apss.engine import ApssError, ApssIndex
from helpers import BAND
from test_gpu_components import check_labels, path_rows, rows_of, uf_labels

pytestmark = pytest.mark.gpu

TILE = 512
N, MID = 2001, 1000
S1_N, S1_DIM, S1_THETA = 3000, 2000, 0.5
S5_N = 1000
BUDGET = 5000


def live_labels(n, oq, oc, dead, ext=None):
    """the reference: union-find over the pairs whose two ends are live (and, with ext, lie under different ids)"""
    gone = np.zeros(n, bool)
    gone[list(dead)] = True
    keep = ~(gone[oq] | gone[oc])
    if ext is not None:
        keep &= ext[oq] != ext[oc]
    return uf_labels(n, oq[keep], oc[keep], dead)


def path_index(budget, n=N, **kw):
    rp, idx, val = path_rows(np.arange(n))
    ext = np.arange(n, dtype=np.int64) + 300
    ix = ApssIndex(n + 1, 0.4, tile_rows=TILE, components=True, components_repair=budget, **kw)
    ix.insert(ext, rp, idx, val)
    assert ix.self_join(fetch=False) == 2 * (n - 1)
    return ix, ext


def path_labels(n, dead):
    """a path without the slots in `dead`: every run of live slots is a component, labelled by its first slot"""
    want = np.empty(n, np.int32)
    first = 0
    for x in range(n):
        if x in dead:
            want[x] = -1
            first = x + 1
        else:
            want[x] = first
    return want


@pytest.fixture(scope="module")
def shape1(oracle):
    rp, idx, val = synth.make_vectors(S1_N, S1_DIM, 16, 0.0, seed=7, dup_frac=0.4)
    ext = 9000 - 2 * np.arange(S1_N, dtype=np.int64)  # ids descend with the slot
    oq, oc, os_ = oracle.selfjoin_pairs(S1_DIM, S1_THETA - 0.02, rp, idx, val)
    assert float(np.abs(os_ - S1_THETA).min()) > 100 * BAND
    keep = os_ >= S1_THETA
    return dict(rp=rp, idx=idx, val=val, ext=ext, oq=oq[keep], oc=oc[keep])


@pytest.fixture(scope="module")
def shape5(oracle):
    """1,000 rows of shape 1's kind, with the oracle's pairs at theta = 0.5 and at theta = 0"""
    rp, idx, val = synth.make_vectors(S5_N, S1_DIM, 16, 0.0, seed=7, dup_frac=0.4)
    ext = 9000 - 2 * np.arange(S5_N, dtype=np.int64)
    oq, oc, os_ = oracle.selfjoin_pairs(S1_DIM, -1e-3, rp, idx, val)  # (dense accumulation: the pairs that share a term)
    assert float(os_.min()) > 0 and float(np.abs(os_ - S1_THETA).min()) > 100 * BAND
    keep = os_ >= S1_THETA
    return dict(rp=rp, idx=idx, val=val, ext=ext, pairs={S1_THETA: (oq[keep], oc[keep]), 0.0: (oq, oc)})


def removal_batches(ext, calls=4, per_call=50, seed=3):
    order = np.random.default_rng(seed).permutation(len(ext))[:calls * per_call]
    return [order[c * per_call:(c + 1) * per_call] for c in range(calls)]


# ---- 1. the path of 2,001 rows: its middle, its root, its last leaf, an id again
def test_a_path_loses_its_middle_its_root_and_a_leaf():
    ix, ext = path_index(BUDGET)
    with ix:
        before = check_labels(ix, np.zeros(N, np.int32), ext, complete=1)
        assert ix.remove([ext[MID]]) == 1
        info = check_labels(ix, path_labels(N, {MID}), ext, complete=1)  # (no second join)
        assert info["components"] == 2 and info["largest"] == 1000 and info["resets"] == before["resets"]
        ri = ix.components_repair_info()
        print("middle:", ri)
        assert ri["declined"] == _lib.CCR_RAN and ri["max_rows"] == BUDGET and ri["rows_marked"] == 1
        assert ri["rows_rejoined"] == 2000 and ri["components_touched"] == 1 and ri["pairs_rejoined"] == 2 * 1998
        assert ri["repairs"] == 1 and ri["budget_resets"] == 0 and ri["launches"] > 0 and ri["detach_ms"] > 0 and ri["rejoin_ms"] > 0
        with pytest.raises(ApssError) as e:  # the re-join was a probe: the last call's results are gone
            ix.result_count()
        assert e.value.code == _lib.E_STATE
        assert ix.remove([ext[0]]) == 1  # a root that is the component's label: the new label is slot 1
        info = check_labels(ix, path_labels(N, {0, MID}), ext, complete=1)
        ri = ix.components_repair_info()
        assert ri["rows_rejoined"] == 999 and ri["components_touched"] == 1 and info["resets"] == before["resets"]
        assert ix.remove([ext[N - 1]]) == 1  # a leaf
        check_labels(ix, path_labels(N, {0, MID, N - 1}), ext, complete=1)
        ri = ix.components_repair_info()
        assert ri["rows_rejoined"] == 999 and ri["components_touched"] == 1 and ri["repairs"] == 3
        assert ix.remove([ext[MID]]) == 0  # an id again: nothing newly marked, nothing launched
        ri = ix.components_repair_info()
        assert ri["declined"] == _lib.CCR_NOTHING and ri["launches"] == 0 and ri["rows_marked"] == 0 and ri["repairs"] == 3
        check_labels(ix, path_labels(N, {0, MID, N - 1}), ext, complete=1)


# ---- 2. a singleton goes: nothing is re-joined, the last call's results stay
def test_a_singleton_removal_leaves_the_results():
    # (term N belongs to the path's last row: the row that shares no term gets term N + 1)
    rp, idx, val = path_rows(np.arange(N))
    ext = np.arange(N, dtype=np.int64) + 300
    with ApssIndex(N + 2, 0.4, tile_rows=TILE, components=True, components_repair=BUDGET) as ix:
        ix.insert(ext, rp, idx, val)
        ix.insert(np.array([7], np.int64), np.array([0, 1], np.int64), np.array([N + 1], np.int32), np.array([1.0]))
        want_list = ix.self_join()
        assert len(want_list[0]) == 2 * (N - 1)
        all_ext = np.concatenate([ext, [7]])
        want = np.zeros(N + 1, np.int32)
        want[N] = N
        before = check_labels(ix, want, all_ext, complete=1)
        assert ix.remove([7]) == 1
        ri = ix.components_repair_info()
        assert ri["declined"] == _lib.CCR_RAN and ri["rows_rejoined"] == 0 and ri["components_touched"] == 1 and ri["pairs_rejoined"] == 0
        assert ix.result_count() == 2 * (N - 1)
        for got, was in zip(ix.fetch(), want_list):
            assert np.array_equal(got, was)
        want[N] = -1
        info = check_labels(ix, want, all_ext, complete=1)
        assert info["resets"] == before["resets"]


# ---- 3. the budget
def test_the_budget_and_its_boundary():
    ix, ext = path_index(10)
    with ix:
        before = ix.components_info()
        assert ix.remove([ext[MID]]) == 1
        want = np.arange(N, dtype=np.int32)
        want[MID] = -1
        info = check_labels(ix, want, ext, complete=0)  # exactly the rule without the repair
        assert info["resets"] == before["resets"] + 1 and info["unions_total"] == 0 and info["singletons"] == N - 1
        ri = ix.components_repair_info()
        assert ri["declined"] == _lib.CCR_BUDGET and ri["budget_resets"] == 1 and ri["repairs"] == 0 and ri["rows_rejoined"] == 0
    ix, ext = path_index(2000)  # A == max_rows
    with ix:
        before = ix.components_info()
        assert ix.remove([ext[MID]]) == 1
        info = check_labels(ix, path_labels(N, {MID}), ext, complete=1)
        ri = ix.components_repair_info()
        assert ri["declined"] == _lib.CCR_RAN and ri["rows_rejoined"] == 2000 and ri["budget_resets"] == 0
        assert info["resets"] == before["resets"]
        ix.set_components_repair(1999)  # (the setting may change at any time) one row too many now
        assert ix.remove([ext[0]]) == 1
        assert ix.components_repair_info()["declined"] == _lib.CCR_RAN  # 999 rows
        ix.set_components_repair(998)
        assert ix.remove([ext[N - 1]]) == 1
        ri = ix.components_repair_info()
        assert ri["declined"] == _lib.CCR_BUDGET and ri["budget_resets"] == 1
        assert ix.components_info()["complete"] == 0


# ---- 4. shape 1 of the components tests
def test_shape_1_in_four_removals(shape1):
    s = shape1
    dead = set()
    with ApssIndex(S1_DIM, S1_THETA, tile_rows=TILE, components=True, components_repair=BUDGET) as ix:
        ix.insert(s["ext"], s["rp"], s["idx"], s["val"])
        assert ix.self_join(fetch=False) == len(s["oq"])
        resets = check_labels(ix, live_labels(S1_N, s["oq"], s["oc"], dead), s["ext"], complete=1)["resets"]
        for batch in removal_batches(s["ext"]):
            assert ix.remove(s["ext"][batch]) == len(batch)
            dead |= set(batch.tolist())
            info = check_labels(ix, live_labels(S1_N, s["oq"], s["oc"], dead), s["ext"], complete=1)
            ri = ix.components_repair_info()
            print(ri)
            assert ri["declined"] == _lib.CCR_RAN and ri["rows_marked"] == len(batch) and 0 < ri["components_touched"] <= len(batch)
            assert info["resets"] == resets
        # ... and a fresh handle that was given only the live rows and joined once, slot for slot after compact()
        live = np.array(sorted(set(range(S1_N)) - dead))
        ix.compact()
        got, rep = ix.components()
        info = ix.components_info()
        assert info["complete"] == 1 and info["resets"] == resets and ix.components_repair_info()["remaps"] == 1
        lrp = np.concatenate([[0], np.cumsum(np.diff(s["rp"])[live])]).astype(np.int64)
        take = np.concatenate([np.arange(s["rp"][r], s["rp"][r + 1]) for r in live])
        with ApssIndex(S1_DIM, S1_THETA, tile_rows=TILE, components=True) as fresh:
            fresh.insert(s["ext"][live], lrp, s["idx"][take], s["val"][take])
            fresh.self_join(fetch=False)
            flabels, frep = fresh.components()
            assert np.array_equal(got, flabels) and np.array_equal(rep, frep)
            finfo = fresh.components_info()
            assert (info["components"], info["largest"], info["unions_total"]) == (finfo["components"], finfo["largest"], finfo["unions_total"])
        # (the reference once more, renumbered by rank)
        rank = np.cumsum(np.isin(np.arange(S1_N), live)) - 1
        want = live_labels(S1_N, s["oq"], s["oc"], dead)[live]
        assert np.array_equal(got, rank[want].astype(np.int32))


# ---- 5. every join path
@pytest.mark.parametrize("kw", [
    dict(flags=_lib.FLAG_EXACT_ACCUM), dict(flags=_lib.FLAG_FORCE_SCAN), dict(theta=0.0), dict(head_terms=64), dict(ragged=40),
    dict(top_k=3), dict(top_k=3, top_k_window=2000)],
    ids=["exact_accum", "force_scan", "theta_0", "head_64", "ragged_tail", "top_k", "top_k_windows"])
def test_every_join_path(shape5, kw):
    s = shape5
    kw = dict(kw)
    theta = kw.pop("theta", S1_THETA)
    ragged = kw.pop("ragged", 0)
    oq, oc = s["pairs"][theta]
    dead = set()
    with ApssIndex(S1_DIM, theta, tile_rows=TILE, components=True, components_repair=BUDGET, **kw) as ix:
        r0 = S5_N - ragged
        ix.insert(s["ext"][:r0], *rows_of(s["rp"], s["idx"], s["val"], 0, r0))
        ix.self_join(fetch=False)
        if ragged:  # a ragged last batch: its rows wait outside the tile index while the removals re-join
            ix.insert_and_query(s["ext"][r0:], *rows_of(s["rp"], s["idx"], s["val"], r0, S5_N))
        check_labels(ix, live_labels(S5_N, oq, oc, dead), s["ext"], complete=1)
        windows = 0
        for batch in removal_batches(s["ext"]):
            assert ix.remove(s["ext"][batch]) == len(batch)
            dead |= set(batch.tolist())
            check_labels(ix, live_labels(S5_N, oq, oc, dead), s["ext"], complete=1)
            ri = ix.components_repair_info()
            assert ri["declined"] == _lib.CCR_RAN and ri["rows_rejoined"] > 0
            if "top_k" in kw:  # the re-join's list is the forest's alone: no cut selected from it
                tk = ix.topk_info()
                assert tk["select_launches"] == 0 and tk["kept"] == 0 and tk["pairs_over_theta"] == ri["pairs_rejoined"]
            if "top_k_window" in kw:
                windows = max(windows, ix.topk_window_info()["windows"])
        if "top_k_window" in kw:
            assert windows > 1  # (the re-join ran in windows of its query rows)
        if ragged:  # the last batch still waits outside the tile index: the filter's rendering ends where the self-join left it
            view = _lib.IndexView()
            view.struct_size = ctypes.sizeof(view)
            assert ix._L.apss_index_view_get(ix._h, 1, ctypes.byref(view)) == _lib.OK
            assert view.built_rows == r0 < ix.size()[0] == S5_N
        print(kw, theta, ix.components_repair_info(), ix.stats()["probe_kernel"])


# ---- 6. twins: two stored rows under one id
def test_twins(oracle):
    n = 40
    rp, idx, val = path_rows(np.arange(n))
    # two more rows, identical, on a term of their own, under one id: they never pair with each other
    rp = np.concatenate([rp, rp[-1] + np.array([1, 2])]).astype(np.int64)
    idx = np.concatenate([idx, [n + 5, n + 5]]).astype(np.int32)
    val = np.concatenate([val, [1.0, 1.0]])
    ext = np.arange(n + 2, dtype=np.int64) + 100
    ext[20] = ext[10]  # twins inside the path's component
    ext[n + 1] = ext[n]  # the twins that stay
    oq, oc, _ = oracle.selfjoin_pairs(n + 8, 0.4, rp, idx, val)
    assert (((oq == n) & (oc == n + 1)) | ((oq == n + 1) & (oc == n))).any()  # (the oracle knows no ids: it pairs them)
    with ApssIndex(n + 8, 0.4, tile_rows=TILE, components=True, components_repair=BUDGET) as ix:
        ix.insert(ext, rp, idx, val)
        ix.self_join(fetch=False)
        check_labels(ix, live_labels(n + 2, oq, oc, (), ext), ext, complete=1)
        assert ix.remove([ext[10]]) == 2  # both rows under the id
        want = live_labels(n + 2, oq, oc, (10, 20), ext)
        assert want[9] == 0 and want[11] == 11 and want[21] == 21 and want[n] == n and want[n + 1] == n + 1
        check_labels(ix, want, ext, complete=1)
        ri = ix.components_repair_info()
        assert ri["rows_marked"] == 2 and ri["components_touched"] == 1 and ri["rows_rejoined"] == n - 2


# ---- 7. a structure that was incomplete stays incomplete, and right about every edge it holds
def test_incomplete_before(oracle):
    na, nb, dim = 1000, 500, S1_DIM
    n = na + nb
    rp, idx, val = synth.make_vectors(n, dim, 16, 0.0, seed=7, dup_frac=0.4)
    ext = np.arange(n, dtype=np.int64) + 10
    oq, oc, os_ = oracle.selfjoin_pairs(dim, S1_THETA - 0.02, rp, idx, val)
    assert float(np.abs(os_ - S1_THETA).min()) > 100 * BAND
    oq, oc = oq[os_ >= S1_THETA], oc[os_ >= S1_THETA]
    inside = (oq < na) & (oc < na)
    forest = uf_labels(n, oq[inside], oc[inside])  # what the structure holds before the removal
    sizes = np.bincount(forest, minlength=n)
    # a cluster of A with an edge into B, so that the re-join brings edges the forest never held
    reach = np.zeros(n, bool)
    reach[forest[oq[~inside]]] = True
    reach[forest[oc[~inside]]] = True
    root = int(np.nonzero((sizes >= 3) & reach & (np.arange(n) < na))[0][0])
    members = np.nonzero(forest == root)[0]
    cross = (~inside) & (np.isin(oq, members) | np.isin(oc, members))
    assert cross.any()
    victim = int(members[1])
    rejoined = np.isin(np.arange(n), members)
    rejoined[victim] = False
    live = (oq != victim) & (oc != victim)
    held = live & (inside | rejoined[oq] | rejoined[oc])
    want = uf_labels(n, oq[held], oc[held], (victim,))
    assert (want != uf_labels(n, oq[live & inside], oc[live & inside], (victim,))).any()  # (rows of B join the cluster)
    with ApssIndex(dim, S1_THETA, tile_rows=TILE, components=True, components_repair=BUDGET) as ix:
        ix.insert(ext[:na], *rows_of(rp, idx, val, 0, na))
        ix.self_join(fetch=False)
        ix.insert(ext[na:], *rows_of(rp, idx, val, na, n))
        check_labels(ix, forest, ext, complete=0)
        assert ix.remove([ext[victim]]) == 1
        info = check_labels(ix, want, ext, complete=0)
        ri = ix.components_repair_info()
        print("incomplete:", ri, "cross edges of the component:", int(cross.sum()))
        assert ri["declined"] == _lib.CCR_RAN and ri["rows_rejoined"] == len(members) - 1 and info["complete"] == 0


# ---- 8. compaction: the forest is renumbered
def test_compaction_renumbers_the_forest():
    packed = np.where(np.arange(N - 1) < MID, 0, MID).astype(np.int32)
    ix, ext = path_index(BUDGET)
    live = np.delete(ext, MID)
    with ix:
        ix.remove([ext[MID]])
        before = check_labels(ix, path_labels(N, {MID}), ext, complete=1)
        ix.compact()
        info = check_labels(ix, packed, live, complete=1)  # (no self_join in between)
        ri = ix.components_repair_info()
        print("compact:", ri)
        assert info["rows"] == N - 1 and info["resets"] == before["resets"] and ri["remaps"] == 1 and ri["remap_ms"] > 0
        assert info["unions_total"] == N - 3
    # the same through auto-compaction and one far row (term N + 1: the path's last row holds term N)
    far = (np.array([9], np.int64), np.array([0, 1], np.int64), np.array([N + 1], np.int32), np.array([1.0]))
    rp, idx, val = path_rows(np.arange(N))
    for call, complete in (("insert_and_query", 1), ("insert", 0)):
        with ApssIndex(N + 2, 0.4, tile_rows=TILE, components=True, components_repair=BUDGET, auto_compact=0.0001) as ix:
            ix.insert(ext, rp, idx, val)
            ix.self_join(fetch=False)
            resets = ix.components_info()["resets"]
            assert ix.remove([ext[MID]]) == 1
            getattr(ix, call)(*far)
            assert ix.removal_info()["compactions"] == 1
            want = np.concatenate([packed, [N - 1]]).astype(np.int32)
            info = check_labels(ix, want, np.concatenate([live, [9]]), complete=complete)
            assert info["rows"] == N and info["resets"] == resets and ix.components_repair_info()["remaps"] == 1


# ---- 9. the setting off, the components off, a term shard
def test_setting_off_components_off_and_a_term_shard():
    rp, idx, val = path_rows(np.arange(N))
    ext = np.arange(N, dtype=np.int64) + 300
    singles = np.arange(N, dtype=np.int32)
    with ApssIndex(N + 1, 0.4, tile_rows=TILE, components=True, components_repair=0) as ix:  # test_removal_and_compaction's numbers
        ix.insert(ext, rp, idx, val)
        ix.self_join(fetch=False)
        before = check_labels(ix, np.zeros(N, np.int32), ext, complete=1)
        assert ix.components_repair_info()["declined"] == _lib.CCR_OFF
        assert ix.remove([ext[MID]]) == 1
        want = singles.copy()
        want[MID] = -1
        info = check_labels(ix, want, ext, complete=0)
        assert info["resets"] == before["resets"] + 1 and info["unions_total"] == 0 and info["singletons"] == N - 1
        ri = ix.components_repair_info()
        assert ri["declined"] == _lib.CCR_OFF and ri["rows_marked"] == 1 and ri["launches"] == 0 and ri["repairs"] == 0 and ri["max_rows"] == 0
        ix.self_join(fetch=False)
        joined = check_labels(ix, path_labels(N, {MID}), ext, complete=1)
        ix.compact()
        packed = check_labels(ix, np.arange(N - 1, dtype=np.int32), np.delete(ext, MID), complete=0)
        assert packed["rows"] == 2000 and packed["resets"] == joined["resets"] + 1 and ix.components_repair_info()["remaps"] == 0
    with ApssIndex(N + 1, 0.4, tile_rows=TILE, components_repair=BUDGET) as ix:  # the components off: the setting has no effect
        ix.insert(ext, rp, idx, val)
        ix.self_join(fetch=False)
        assert ix.remove([ext[MID]]) == 1
        ri = ix.components_repair_info()
        assert ri["declined"] == _lib.CCR_NO_COMPONENTS and ri["launches"] == 0 and ri["max_rows"] == BUDGET
        assert ix.result_count() == 2 * (N - 1)  # (nothing probed)
        ix.clear()  # the setting survives
        assert ix.components_repair_info()["max_rows"] == BUDGET
        for bad in (-1, 1 << 31):
            with pytest.raises(ApssError) as e:
                ix.set_components_repair(bad)
            assert e.value.code == _lib.E_INVALID
        ix.set_components_repair((1 << 31) - 1)
        bad = _lib.ComponentsRepairInfo()
        for size in (0, 4, 1 << 20):
            bad.struct_size = size
            assert ix._L.apss_components_repair_get(ix._h, ctypes.byref(bad)) == _lib.E_INVALID
    with pytest.raises(ApssError) as e:
        ApssIndex(S1_DIM, S1_THETA, term_range=(0, S1_DIM // 2), components_repair=BUDGET)
    assert e.value.code == _lib.E_UNSUPPORTED and "term shard" in str(e.value)
