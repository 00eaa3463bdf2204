"""Near-duplicate groups on the device (apss_set_components, csrc/apss_components.hpp): label[slot] = the smallest slot of the
slot's connected component in the graph whose edges are the pairs of the calls' final lists.

The reference labels come from the union-find below (smallest member as root) over pairs mapped from external ids back to slots.
Labels are canonical, so the device's array must equal it exactly, whatever the order its hooks ran in.  Shapes 1 and 2 were
counted on the CPU with the float64 oracle: shape 1 has 2,416 ordered pairs, 2,129 components, the largest of 7 rows, 178 of three
rows or more, and no score within 7.2e-3 of theta; shape 2 has 7,196 pairs, one component of 1,576 rows, and a score 1.8e-5 from
theta -- its reference is the list the call itself fetched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from apss import _lib, synth
from apss.engine import ApssError, ApssIndex
from helpers import BAND

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "all-pairs-similarity_amd", "host")
TILE = 512  # components span tiles

S1_N, S1_DIM, S1_THETA = 3000, 2000, 0.5


def uf_labels(n, u, v, dead=()):
    """label[x] = smallest member of x's component under the edges u[i] - v[i]; -1 for the slots in `dead`"""
    p = list(range(n))

    def find(x):
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x
    for a, b in zip(np.asarray(u).tolist(), np.asarray(v).tolist()):
        a, b = find(a), find(b)
        if a != b:
            p[max(a, b)] = min(a, b)
    lab = np.array([find(x) for x in range(n)], np.int32)
    lab[list(dead)] = -1
    return lab


def slots_of(ext):
    """external id -> slot, for a store whose ids are distinct"""
    return {int(e): s for s, e in enumerate(np.asarray(ext).tolist())}


def pair_slots(q, c, at):
    return [at[int(a)] for a in q], [at[int(b)] for b in c]


def check_labels(ix, want, ext, complete=None):
    """labels, representatives, the device view and the counts against the reference labels `want`"""
    labels, rep = ix.components()
    assert labels.dtype == np.int32 and rep.dtype == np.int64
    bad = np.nonzero(labels != want)[0]
    assert bad.size == 0, "%d labels differ, e.g. slots %s: %s for %s" % (bad.size, bad[:5], labels[bad[:5]], want[bad[:5]])
    ext = np.asarray(ext, np.int64)
    assert np.array_equal(rep, np.where(want >= 0, ext[np.maximum(want, 0)], ext))
    assert np.array_equal(ix.components_dev().cpu().numpy(), want)
    info = ix.components_info()
    live = want[want >= 0]
    sizes = np.bincount(live, minlength=1)
    sizes = sizes[sizes > 0]
    assert info["on"] == 1 and info["rows"] == len(want) and info["rows_live"] == len(live)
    assert info["components"] == len(sizes) and info["singletons"] == int((sizes == 1).sum())
    assert info["largest"] == (int(sizes.max()) if len(sizes) else 0)
    assert info["components"] == info["rows_live"] - info["unions_total"], info
    if complete is not None:
        assert info["complete"] == complete, info
    return info


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


@pytest.fixture(scope="module")
def shape1(oracle):
    rp, idx, val = synth.make_vectors(S1_N, S1_DIM, 16, 0.0, seed=7, dup_frac=0.4)
    ext = 9000 - 2 * np.arange(S1_N, dtype=np.int64)  # ids descend with the slot: id order and slot order disagree
    # the oracle's scores a little below theta too: none lies in the band where fp32 and float64 may disagree about a pair
    oq, oc, os_ = oracle.selfjoin_pairs(S1_DIM, S1_THETA - 0.02, rp, idx, val)
    gap = float(np.abs(os_ - S1_THETA).min())
    print("shape 1: nearest score %.3g from theta" % gap)
    assert gap > 100 * BAND
    keep = os_ >= S1_THETA
    labels = uf_labels(S1_N, oq[keep], oc[keep])
    return dict(rp=rp, idx=idx, val=val, ext=ext, pairs=int(keep.sum()), labels=labels)


def rows_of(rp, idx, val, r0, r1):
    return rp[r0:r1 + 1] - rp[r0], idx[rp[r0]:rp[r1]], val[rp[r0]:rp[r1]]


# ---- 1. against float64
def test_against_the_oracle(shape1):
    s = shape1
    sizes = np.bincount(s["labels"])
    assert (s["pairs"], int((sizes > 0).sum()), int(sizes.max()), int((sizes >= 3).sum())) == (2416, 2129, 7, 178)
    with ApssIndex(S1_DIM, S1_THETA, tile_rows=TILE, components=True) as ix:
        ix.insert(s["ext"], s["rp"], s["idx"], s["val"])
        assert ix.components_info()["complete"] == 0
        assert ix.self_join(fetch=False) == s["pairs"]
        info = check_labels(ix, s["labels"], s["ext"], complete=1)
        print("shape 1:", info)
        assert info["declined"] == _lib.CC_RAN and info["pairs_absorbed"] == s["pairs"] and info["hook_launches"] == 1
        assert info["components"] == 2129 and info["largest"] == 7 and info["unions_total"] == S1_N - 2129


# ---- 2. a giant component: the reference is the union-find over the list this call fetched
def test_a_giant_component():
    n, dim, theta = 3000, 400, 0.4
    rp, idx, val = synth.make_vectors(n, dim, 12, 0.0, seed=2, dup_frac=0.2)
    ext = np.arange(n, dtype=np.int64) + 50
    with ApssIndex(dim, theta, tile_rows=TILE, components=True) as ix:
        ix.insert(ext, rp, idx, val)
        q, c, _ = ix.self_join()
        want = uf_labels(n, q - 50, c - 50)
        info = check_labels(ix, want, ext, complete=1)
        print("giant:", len(q), info)
        assert len(q) > 7000 and info["largest"] > 1500


# ---- 3. adversarial orders, built by hand
def path_rows(order, base=0):
    """row i of a path: terms {base + i, base + i + 1}, both 1/sqrt(2) -- neighbours score 0.5, all others 0; in the given order"""
    order = np.asarray(order, np.int64)
    n = len(order)
    rp = 2 * np.arange(n + 1, dtype=np.int64)
    idx = np.stack([base + order, base + order + 1], axis=1).astype(np.int32).ravel()
    val = np.full(2 * n, 1.0 / np.sqrt(2.0))
    return rp, idx, val


@pytest.mark.timeout(20)  # (a hang guard for the labelling's walk, not a speed target)
def test_a_path_in_reverse_order():
    n = 20000
    rp, idx, val = path_rows(np.arange(n)[::-1])
    ext = np.arange(n, dtype=np.int64)
    with ApssIndex(n + 1, 0.4, tile_rows=TILE, components=True) as ix:
        ix.insert(ext, rp, idx, val)
        assert ix.self_join(fetch=False) == 2 * (n - 1)
        info = check_labels(ix, np.zeros(n, np.int32), ext, complete=1)
        print("path:", info)
        assert info["components"] == 1 and info["largest"] == n and info["unions_total"] == n - 1


def test_two_paths_with_interleaved_slots():
    m = 1500
    a, b = path_rows(np.arange(m)[::-1]), path_rows(np.arange(m), base=m + 5)
    rp = 2 * np.arange(2 * m + 1, dtype=np.int64)
    idx, val = np.empty(4 * m, np.int32), np.empty(4 * m)
    for half, (_, i, v) in enumerate((a, b)):  # path A in the even slots, path B in the odd ones
        idx.reshape(2 * m, 2)[half::2] = i.reshape(m, 2)
        val.reshape(2 * m, 2)[half::2] = v.reshape(m, 2)
    ext = np.arange(2 * m, dtype=np.int64) * 7
    with ApssIndex(2 * m + 10, 0.4, tile_rows=TILE, components=True) as ix:
        ix.insert(ext, rp, idx, val)
        assert ix.self_join(fetch=False) == 4 * (m - 1)
        info = check_labels(ix, (np.arange(2 * m) % 2).astype(np.int32), ext, complete=1)
        assert info["components"] == 2 and info["largest"] == m


def test_a_star_duplicates_and_isolated_rows():
    """a hub of 16 terms at 1/4 in slot 300 and 16 x 40 leaves that share one hub term at 0.9 plus a private term (theta 0.2: hub -
    leaf 0.225); 50 rows stored twice under different ids; 30 rows that share nothing"""
    rows, priv = [], 100

    def add(terms, weights):
        rows.append((list(terms), list(weights)))
    for leaf in range(640):
        if leaf == 300:
            add(range(16), [0.25] * 16)
        add([leaf % 16, priv + leaf], [0.9, np.sqrt(1 - 0.81)])
    star = len(rows)
    for d in range(50):
        add([1000 + 2 * d, 1001 + 2 * d], [0.6, 0.8])
    for d in range(50):
        add([1000 + 2 * d, 1001 + 2 * d], [0.6, 0.8])
    for d in range(30):
        add([2000 + d], [1.0])
    n = len(rows)
    rp = np.concatenate([[0], np.cumsum([len(t) for t, _ in rows])]).astype(np.int64)
    idx = np.concatenate([t for t, _ in rows]).astype(np.int32)
    val = np.concatenate([w for _, w in rows]).astype(np.float64)
    ext = np.arange(n, dtype=np.int64) + 10_000
    want = np.arange(n, dtype=np.int32)
    want[:star] = 0
    want[star + 50:star + 100] = np.arange(star, star + 50)
    with ApssIndex(2100, 0.2, tile_rows=TILE, components=True) as ix:
        ix.insert(ext, rp, idx, val)
        q, c, _ = ix.self_join()
        assert np.array_equal(want, uf_labels(n, q - 10_000, c - 10_000))  # (the hand-made shape is what it was meant to be)
        info = check_labels(ix, want, ext, complete=1)
        assert info["largest"] == star == 641 and info["singletons"] == 30 and info["components"] == 1 + 50 + 30


# ---- 4. every join path gives the same labels
@pytest.mark.parametrize("kw", [
    dict(), dict(flags=_lib.FLAG_NO_SYMMETRY), dict(flags=_lib.FLAG_EXACT_ACCUM), dict(flags=_lib.FLAG_FORCE_SCAN), dict(head_terms=64),
    dict(top_k=3, top_k_window=2000), dict(top_pairs=7)],
    ids=["default", "no_symmetry", "exact_accum", "force_scan", "head_64", "top_k_windows", "top_pairs"])
def test_every_join_path(shape1, kw):
    s = shape1
    cut = "top_k" in kw or "top_pairs" in kw
    with ApssIndex(S1_DIM, S1_THETA, tile_rows=TILE, **kw) as off:
        off.insert(s["ext"], s["rp"], s["idx"], s["val"])
        n_off = off.self_join(fetch=False)
        want_list = device_list(off)
    with ApssIndex(S1_DIM, S1_THETA, tile_rows=TILE, components=True, **kw) as ix:
        ix.insert(s["ext"], s["rp"], s["idx"], s["val"])
        assert ix.self_join(fetch=False) == n_off
        got_list = device_list(ix)
        info = check_labels(ix, s["labels"], s["ext"], complete=1)
        print(kw, info)
        assert info["pairs_absorbed"] == s["pairs"]  # (the uncut graph, whatever the cuts keep afterwards)
        if "top_k_window" in kw:
            tw = ix.topk_window_info()
            assert tw["windows"] > 1 and 1 < info["hook_launches"] <= tw["windows"]  # (a window without a pair hooks nothing)
        if cut:  # the result list is untouched, element by element
            assert n_off < s["pairs"]
            for g, w in zip(got_list, want_list):
                assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
        else:
            assert sorted(zip(*[a.tolist() for a in got_list])) == sorted(zip(*[a.tolist() for a in want_list]))
        on_bytes = ix.stats()["hbm_bytes"]
        ix.set_components(False)  # (what the stage reserved -- at most 12 B per stored slot and its four words -- is returned)
        assert 0 < on_bytes - ix.stats()["hbm_bytes"] <= 12 * S1_N + 64


# ---- 5. streams
def test_a_stream_of_insert_and_query_calls(shape1):
    s = shape1
    at = slots_of(s["ext"])
    us, vs = [], []
    with ApssIndex(S1_DIM, S1_THETA, tile_rows=TILE, components=True) as ix:
        r0 = 0
        for rows in (1, 1, 1, 61, 500, 1000, 1436):
            r1 = r0 + rows
            q, c, _ = ix.insert_and_query(s["ext"][r0:r1], *rows_of(s["rp"], s["idx"], s["val"], r0, r1))
            u, v = pair_slots(q, c, at)
            us += u
            vs += v
            info = check_labels(ix, uf_labels(r1, us, vs), s["ext"][:r1], complete=1)
            assert info["pairs_absorbed"] == len(q) and info["hook_launches"] == (1 if len(q) else 0)
            r0 = r1
        assert r0 == S1_N
        check_labels(ix, s["labels"], s["ext"], complete=1)
        # a plain insert: new singletons, and nobody has seen their edges
        xrp, xidx, xval = synth.make_vectors(100, S1_DIM, 16, 0.0, seed=9, dup_frac=0.4)
        xext = np.arange(100, dtype=np.int64) + 20_000
        ix.insert(xext, xrp, xidx, xval)
        ext = np.concatenate([s["ext"], xext])
        check_labels(ix, np.concatenate([s["labels"], np.arange(S1_N, S1_N + 100, dtype=np.int32)]), ext, complete=0)
        # a self-join makes it complete again: the labels of a fresh handle over the same rows
        q, c, _ = ix.self_join()
        all_at = slots_of(ext)
        joined = check_labels(ix, uf_labels(S1_N + 100, *pair_slots(q, c, all_at)), ext, complete=1)
        with ApssIndex(S1_DIM, S1_THETA, tile_rows=TILE, components=True) as fresh:
            fresh.insert(ext, np.concatenate([s["rp"], s["rp"][-1] + xrp[1:]]), np.concatenate([s["idx"], xidx]), np.concatenate([s["val"], xval]))
            fresh.self_join(fetch=False)
            assert np.array_equal(fresh.components()[0], ix.components()[0])
            assert fresh.components_info()["components"] == joined["components"]


def test_a_stream_with_admission(oracle):
    """tests/test_gpu_group_relayout.py's admission data at n = 2000: un-normalised rows whose sums straddle theta; the rows that
    are not admitted get no slot, and the labels speak of the admitted rows' slots"""
    n, dim, nnz, theta = 2000, 1200, 12, 0.6
    rp, idx, val = synth.make_vectors(n, dim, nnz, 0.0, seed=8, dup_frac=0.4)
    raw = val * np.repeat(np.random.default_rng(1).uniform(0.12, 1.0, size=n), nnz)
    keep = np.asarray(oracle.admission(rp, raw, theta)).astype(bool)
    assert 0.2 * n < keep.sum() < 0.95 * n
    slot = np.cumsum(keep) - 1  # of an admitted row
    ext = np.arange(n, dtype=np.int64)
    us, vs = [], []
    with ApssIndex(dim, theta, tile_rows=TILE, flags=_lib.FLAG_ADMISSION, head_terms=-1, components=True) as ix:
        r0, pairs = 0, 0
        for rows in (300, 700, 1000):
            r1 = r0 + rows
            q, c, _ = ix.insert_and_query(ext[r0:r1], *rows_of(rp, idx, raw, r0, r1))
            assert keep[q].all() and keep[c].all()
            us += slot[q].tolist()
            vs += slot[c].tolist()
            pairs += len(q)
            stored = int(keep[:r1].sum())
            assert ix.size()[0] == stored
            check_labels(ix, uf_labels(stored, us, vs), ext[:r1][keep[:r1]], complete=1)
            r0 = r1
        assert pairs > 50


# ---- 6. removal and compaction, on the path of 2,001 rows
def test_removal_and_compaction():
    n, mid = 2001, 1000
    rp, idx, val = path_rows(np.arange(n))
    ext = np.arange(n, dtype=np.int64) + 300
    singles = np.arange(n, dtype=np.int32)
    with ApssIndex(n + 1, 0.4, tile_rows=TILE, components=True) as ix:
        ix.insert(ext, rp, idx, val)
        ix.self_join(fetch=False)
        before = check_labels(ix, np.zeros(n, np.int32), ext, complete=1)
        assert ix.remove([ext[mid]]) == 1
        want = singles.copy()
        want[mid] = -1
        info = check_labels(ix, want, ext, complete=0)  # (the removed row: -1 and its own id)
        assert info["resets"] == before["resets"] + 1 and info["unions_total"] == 0 and info["singletons"] == n - 1
        assert ix.remove([ext[mid]]) == 0 and ix.components_info()["resets"] == info["resets"]  # (nothing newly marked: no reset)
        ix.self_join(fetch=False)
        want = np.where(singles < mid, 0, mid + 1).astype(np.int32)
        want[mid] = -1
        info = check_labels(ix, want, ext, complete=1)
        assert info["components"] == 2 and info["largest"] == 1000 and info["singletons"] == 0
        ix.compact()
        live = np.delete(ext, mid)
        packed = check_labels(ix, np.arange(n - 1, dtype=np.int32), live, complete=0)
        assert packed["rows"] == 2000 and packed["resets"] == info["resets"] + 1
        ix.self_join(fetch=False)
        check_labels(ix, np.where(np.arange(n - 1) < mid, 0, mid).astype(np.int32), live, complete=1)
    # the same through auto-compaction: the insert that follows the removal compacts first
    with ApssIndex(n + 1, 0.4, tile_rows=TILE, components=True, auto_compact=0.0001) as ix:
        ix.insert(ext, rp, idx, val)
        ix.self_join(fetch=False)
        resets = ix.components_info()["resets"]
        assert ix.remove([ext[mid]]) == 1
        ix.insert(np.array([9], np.int64), np.array([0, 1], np.int64), np.array([n], np.int32), np.array([1.0]))
        assert ix.removal_info()["compactions"] == 1
        info = check_labels(ix, np.arange(n, dtype=np.int32), np.concatenate([np.delete(ext, mid), [9]]), complete=0)
        assert info["rows"] == n and info["resets"] == resets + 2  # (the removal's and the compaction's)


# ---- 7. query_stored and outside batches
def test_query_stored_and_outside_batches(shape1):
    s = shape1
    at = slots_of(s["ext"])
    with ApssIndex(S1_DIM, S1_THETA, tile_rows=TILE, components=True) as ix:
        ix.insert(s["ext"], s["rp"], s["idx"], s["val"])
        ids = s["ext"][100:300]
        q, c, _ = ix.query_stored(ids)
        assert len(q) > 50
        want = uf_labels(S1_N, *pair_slots(q, c, at))
        info = check_labels(ix, want, s["ext"], complete=0)
        assert info["declined"] == _lib.CC_RAN and info["pairs_absorbed"] == len(q)
        # the same rows as an outside batch: nothing absorbed, nothing changed
        q2, _, _ = ix.query(ids, *rows_of(s["rp"], s["idx"], s["val"], 100, 300))
        assert len(q2) >= len(q)
        again = check_labels(ix, want, s["ext"], complete=0)
        assert again["declined"] == _lib.CC_OUTSIDE and again["pairs_absorbed"] == 0 and again["hook_launches"] == 0
        assert again["unions_total"] == info["unions_total"]


def test_a_call_whose_probe_cut_its_rounds():
    """theta = 0 with top_k = 5 and the tile cut (tests/test_gpu_topk_tile_cut.py's shape): the list is not every pair"""
    n, dim = 2000, 64
    rp, idx, val = synth.make_vectors(n, dim, 8, 0.0, seed=5, dup_frac=0.1)
    ext = np.arange(n, dtype=np.int64)
    with ApssIndex(dim, 0.0, tile_rows=TILE, top_k=5, top_k_tile_cut=True, components=True) as ix:
        ix.insert(ext, rp, idx, val)
        ix.self_join(fetch=False)
        assert ix.topk_tile_cut_info()["applied"] == 1
        info = check_labels(ix, np.arange(n, dtype=np.int32), ext, complete=0)
        assert info["declined"] == _lib.CC_TILE_CUT and info["pairs_absorbed"] == 0 and info["unions_total"] == 0


# ---- 8. the setting and the edges
def test_setting_off_on_off(shape1):
    s = shape1
    with ApssIndex(S1_DIM, S1_THETA, tile_rows=TILE) as never, ApssIndex(S1_DIM, S1_THETA, tile_rows=TILE) as ix:
        for h in (never, ix):
            h.insert(s["ext"], s["rp"], s["idx"], s["val"])
        base = sorted(zip(*[a.tolist() for a in never.self_join()]))
        off = ix.components_info()
        assert off["on"] == 0 and off["declined"] == _lib.CC_OFF and off["rows"] == 0
        for call in (ix.components, ix.components_dev):
            with pytest.raises(ApssError) as e:
                call()
            assert e.value.code == _lib.E_STATE
        assert sorted(zip(*[a.tolist() for a in ix.self_join()])) == base
        assert ix.stats()["hbm_bytes"] == never.stats()["hbm_bytes"]
        ix.set_components(True)
        assert ix.stats()["hbm_bytes"] == never.stats()["hbm_bytes"]  # (nothing until the structure is used)
        check_labels(ix, np.arange(S1_N, dtype=np.int32), s["ext"], complete=0)
        on_bytes = ix.stats()["hbm_bytes"]
        assert 0 < on_bytes - never.stats()["hbm_bytes"] <= 12 * S1_N + 64
        ix.self_join(fetch=False)
        check_labels(ix, s["labels"], s["ext"], complete=1)
        ix.set_components(False)
        assert ix.stats()["hbm_bytes"] == never.stats()["hbm_bytes"] and ix.components_info()["on"] == 0
        ix.set_components(True)  # made again from nothing: singletons
        check_labels(ix, np.arange(S1_N, dtype=np.int32), s["ext"], complete=0)
        assert ix.stats()["hbm_bytes"] == on_bytes
        with pytest.raises(ApssError) as e:
            ix._chk(ix._L.apss_set_components(ix._h, 2))
        assert e.value.code == _lib.E_INVALID


def test_small_stores_fetch_ranges_and_lazy_labels(shape1):
    s = shape1
    L = _lib.lib()
    with ApssIndex(S1_DIM, S1_THETA, tile_rows=TILE, components=True) as ix:
        info = ix.components_info()  # an empty store
        assert (info["rows"], info["components"], info["largest"], info["complete"], info["label_launches"]) == (0, 0, 0, 1, 0)
        assert ix.components()[0].size == 0 and ix.components_dev().numel() == 0
        ix.insert_and_query(s["ext"][:1], *rows_of(s["rp"], s["idx"], s["val"], 0, 1))  # a store of one row
        one = check_labels(ix, np.zeros(1, np.int32), s["ext"][:1], complete=1)
        assert one["components"] == one["singletons"] == one["largest"] == 1
        ix.clear()  # the setting survives
        info = ix.components_info()
        assert info["on"] == 1 and info["rows"] == 0 and info["complete"] == 1
        ix.insert(s["ext"], s["rp"], s["idx"], s["val"])
        ix.self_join(fetch=False)
        first = ix.components_info()
        assert first["label_launches"] > 0 and first["label_ms"] > 0 and first["hook_ms"] > 0
        second = ix.components_info()  # nothing changed: nothing launched
        assert second["label_launches"] == 0 and second["components"] == first["components"] == 2129
        labels, rep = ix.components(offset=1000, count=500)
        assert np.array_equal(labels, s["labels"][1000:1500]) and np.array_equal(rep, s["ext"][s["labels"][1000:1500]])
        assert ix.components_info()["label_launches"] == 0
        only = np.zeros(7, np.int32)  # either output may be NULL
        assert L.apss_components_fetch(ix._h, 2993, 7, only.ctypes.data_as(ctypes.c_void_p), None) == _lib.OK
        assert np.array_equal(only, s["labels"][2993:])
        reps = np.zeros(7, np.int64)
        assert L.apss_components_fetch(ix._h, 0, 7, None, reps.ctypes.data_as(ctypes.c_void_p)) == _lib.OK
        assert np.array_equal(reps, s["ext"][s["labels"][:7]])
        assert L.apss_components_fetch(ix._h, S1_N, 0, None, None) == _lib.OK
        for offset, count in ((-1, 1), (0, S1_N + 1), (S1_N, 1), (5, -1)):
            assert L.apss_components_fetch(ix._h, offset, count, None, None) == _lib.E_INVALID
        bad = _lib.ComponentsInfo()  # struct_size not set, too small, absurd
        for size in (0, 4, 1 << 20):
            bad.struct_size = size
            assert L.apss_components_get(ix._h, ctypes.byref(bad)) == _lib.E_INVALID
        short = _lib.ComponentsInfo()  # an older caller's shorter struct gets the fields it knows
        short.struct_size = 16
        assert L.apss_components_get(ix._h, ctypes.byref(short)) == _lib.OK
        assert (short.struct_size, short.on, short.complete, short.rows) == (16, 1, 1, 0)


def test_a_term_shard_refuses():
    with pytest.raises(ApssError) as e:
        ApssIndex(S1_DIM, S1_THETA, term_range=(0, S1_DIM // 2), components=True)
    assert e.value.code == _lib.E_UNSUPPORTED and "term shard" in str(e.value)
    with ApssIndex(S1_DIM, S1_THETA, term_range=(0, S1_DIM // 2)) as shard:
        assert shard.components_info()["on"] == 0


def test_the_hook_loop_takes_its_later_trips(shape1, monkeypatch):
    """APSS_DEBUG=cc_grid=1: one workgroup walks the 2,416 pairs in ten trips"""
    s = shape1
    monkeypatch.setenv("APSS_DEBUG", "cc_grid=1")
    with ApssIndex(S1_DIM, S1_THETA, tile_rows=TILE, components=True) as ix:
        ix.insert(s["ext"], s["rp"], s["idx"], s["val"])
        ix.self_join(fetch=False)
        check_labels(ix, s["labels"], s["ext"], complete=1)


# ---- 9. the host mirror
def test_host_mirror_reports_groups():
    subprocess.check_call(["make", "-C", HOST], stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(HOST, "host_components_selftest")], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr[-2000:])
    assert out.returncode == 0 and "host_components_selftest: PASS" in out.stdout
