"""Removal of stored vectors at its edges (csrc/apss_remove.hpp and the removal code of csrc/apss_hip.hip): a ragged store with
an odd row count, external ids over the whole int64 range, the three grid-stride kernels made to take their later trips
(APSS_DEBUG=rm_grid=N), drop lists of every length around a lane's four pairs and a wave's 256, compaction through the
stored-ingest path on every kind of handle, and the path mixes DESIGN.md 5f claims.  The references are the double-precision
oracle with the dead rows' pairs deleted in numpy (tests/remove_ragged.py), a planted join whose answer is known, and a fresh
handle that was only ever given the live rows.  Every oracle-side floor is asserted before the first device call.

Gap of the single-shape suite -> the test that closes it:
  1  k_rm_mark, the unpaired last id (two == false)         test_mark_edges[*]: S = 1501, the first removal is the last row's id
  2  k_rm_mark, ids: range reject, signed sort, search       test_mark_edges[*]: ids < 0, > 2^32, INT64_MIN / MAX, lists wholly
     below / above, every id twice, two live rows under one id
  3  grid-stride loops of k_rm_mark / k_rm_rows / k_rm_drop  test_mark_edges[rm_grid=1], test_compaction_ragged[plain_rm_grid1],
     and `if (total == 0) continue` with a trip behind it   test_drop_list_lengths[rm_grid=1] (m = 1025; 1027 pairs whose first 1024 all go)
  4  k_rm_drop, list lengths: 16-B path and by-element tail  test_drop_list_lengths[*]: m = 1 .. 5, 63 .. 65, 255 .. 257, 1023 .. 1025,
     a list dropped entirely, a list with nothing dropped
  5  k_rm_gather: rows of 0, 1, 63, 64, 65, 129, 200 entries, test_compaction_ragged[plain] (bit for bit against the twin; row
     a dead last row, a compaction that leaves nothing      S - 1 is in D), test_compaction_ragged[nothing_left], [empty_rows_only]
  6  compaction through the stored-ingest path               test_compaction_ragged[prune], [head], [signed]; rows waiting
     outside the index in every configuration (the third insert batch)
  7  path mixes with marks                                   test_paths_with_marks[windowed_self_join], [regrow_no_head],
     [regrow_head64], [virtual_rows], [waiting_rows], [auto_compact_head]"""
import ctypes as C

import numpy as np
import pytest

import remove_ragged as rr
from apss import _lib
from apss.engine import ApssIndex
from helpers import TOL, assert_same_pairs, to_map
from store_view import band_cases, read_store, reference_store
from test_gpu_topk import check_topk

pytestmark = pytest.mark.gpu

S, Q, N, DIM, THETA, TILE = rr.S, rr.Q, rr.N, rr.DIM, rr.THETA, 256
IDS, D, IS_D = rr.IDS, rr.D, rr.IS_D
GRIDS = ["", "rm_grid=1"]
BATCHES = ((0, 700), (700, 1461), (1461, S))  # the last 40 rows wait outside the tile index (kTailMaxBatch = 64)


def handle(monkeypatch, debug="", theta=THETA, dim=DIM, **kw):
    """APSS_DEBUG is read when a handle is created"""
    if debug:
        monkeypatch.setenv("APSS_DEBUG", debug)
    else:
        monkeypatch.delenv("APSS_DEBUG", raising=False)
    ix = ApssIndex(dim, theta, tile_rows=kw.pop("tile_rows", TILE), **kw)
    monkeypatch.delenv("APSS_DEBUG", raising=False)
    return ix


def info_is(ix, dead, removed_total):
    info = ix.removal_info()
    n = int(np.count_nonzero(dead))
    assert (info["rows_removed"], info["rows_live"], info["removed_total"]) == (n, dead.size - n, removed_total), info
    assert ix.size()[0] == dead.size  # physical rows
    return info


def signed_path(name):
    """does apss_stats.probe_kernel name an instantiation for weights of either sign?"""
    args = name[name.index("<") + 1:name.rindex(">")].split(", ")
    if name.startswith("k_probe_coarse<"):
        return args[7] == "true"
    if name.startswith("k_probe_even<"):
        return args[4] == "true"
    return name.startswith("k_probe<") and args[0] == "1"


def sorted_list(got):
    q, c, s = got
    order = np.lexsort((c, q))
    return q[order], c[order], s[order]


# ---- 2. marking
class MarkModel:
    """apss_remove in numpy: the rows of `ext` that are live and listed"""

    def __init__(self, ext):
        self.ext, self.dead, self.total = np.array(ext, np.int64), np.zeros(len(ext), bool), 0

    def remove(self, ids):
        hit = np.isin(self.ext, np.asarray(ids, np.int64)) & ~self.dead
        self.dead |= hit
        self.total += int(hit.sum())
        return int(hit.sum())

    def append(self, ext):
        self.ext = np.concatenate([self.ext, np.asarray(ext, np.int64)])
        self.dead = np.concatenate([self.dead, np.zeros(len(ext), bool)])


@pytest.mark.parametrize("grid", GRIDS)
def test_mark_edges(oracle, monkeypatch, grid):
    import torch
    v = rr.vectors()
    orc = rr.whole_join(oracle, 0.0, False, S)
    rr.class_floors(orc, orc[1] < S, ~IS_D[orc[1]])
    _, want, dropped, _ = rr.split(orc, THETA, orc[1] < S, ~IS_D[orc[1]])
    # the two rows stored (and removed) under one new id at the end are copies of query rows S and S + 1: they and every query
    # row that scores >= theta against one of them lose that pair too
    dropped += 2 + int(((orc[2] >= THETA) & ((orc[1] == S) | (orc[1] == S + 1))).sum())
    stored_min, stored_max = np.sort(IDS[:S])[[1, -2]]  # the stored ids next to the two extremes
    assert IDS[1] == rr.I64_MIN and IDS[2] == rr.I64_MAX and stored_min < 0 and stored_max > 1 << 62
    below = np.array([rr.I64_MIN + 1, -10 ** 12, int(stored_min) - 1], dtype=np.int64)
    above = np.array([int(stored_max) + 1, (1 << 62) + (1 << 40), rr.I64_MAX - 1], dtype=np.int64)
    twice = np.random.default_rng(11).permutation(np.concatenate([IDS[D], IDS[D]]))
    new_id = (1 << 50) + 7
    assert new_id not in rr.ROW_OF
    steps = [[IDS[S - 1]],                                        # the unpaired tail of an odd store
             below, above,                                        # wholly outside the stored range: nothing
             np.concatenate([[rr.I64_MIN], below]),               # ... or exactly the row that carries the extreme
             np.concatenate([above, [rr.I64_MAX]]),
             twice,                                               # every id of D twice, shuffled
             [rr.I64_MIN, rr.I64_MAX]]                            # both extremes, marked already
    want_counts = [1, 0, 0, 1, 1, D.size - 3, 0]
    counts = {}
    for dev in (False, True):
        model = MarkModel(IDS[:S])
        with handle(monkeypatch, grid) as ix:
            ix.insert(IDS[:S], *rr.rows_of(v, 0, S))
            counts[dev] = []
            for ids in steps:
                ids = np.asarray(ids, np.int64)
                n = ix.remove(torch.from_numpy(ids).cuda() if dev else ids)
                assert n == model.remove(ids), (dev, ids[:4], n)
                counts[dev].append(n)
                info_is(ix, model.dead, model.total)
            assert counts[dev] == want_counts and np.array_equal(model.dead, IS_D[:S])
            # two LIVE rows under one id: both are marked, and a query that holds their vectors finds neither
            ix.insert(np.array([new_id, new_id], dtype=np.int64), *rr.rows_of(v, S, S + 2))
            model.append([new_id, new_id])
            assert rr.LEN[S] > 0 and rr.LEN[S + 1] > 0
            found = to_map(*ix.query(IDS[S:S + 2], *rr.rows_of(v, S, S + 2)))
            assert abs(found[(int(IDS[S]), new_id)] - 1.0) <= TOL and abs(found[(int(IDS[S + 1]), new_id)] - 1.0) <= TOL
            n = ix.remove(torch.tensor([new_id], dtype=torch.int64).cuda() if dev else [new_id])
            assert n == model.remove([new_id]) == 2
            info_is(ix, model.dead, model.total)
            got = ix.query(IDS[S:], *rr.rows_of(v, S, N))
            info = ix.removal_info()
        assert new_id not in got[1]
        assert_same_pairs(to_map(*got), rr.by_id(want), THETA)
        assert info["pairs_dropped"] == dropped and info["drop_launches"] == 1
    assert counts[False] == counts[True]


# ---- 3. drop-list lengths on a planted join
P_ROWS, P_NNZ = 1100, 4
P_DIM = P_ROWS * P_NNZ
LENGTHS_M = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025]


def planted():
    """1100 unit rows of 4 private terms each: a copy of row j scores 1 against row j and shares no term with any other"""
    rng = np.random.default_rng(3)
    w = rng.uniform(0.2, 1.0, (P_ROWS, P_NNZ))
    w /= np.sqrt((w * w).sum(axis=1, keepdims=True))
    rp = np.arange(0, P_DIM + 1, P_NNZ, dtype=np.int64)
    return rp, np.arange(P_DIM, dtype=np.int32), w.reshape(-1)


def assert_planted_call(ix, v, rows, dead):
    """a frozen query of copies of the stored `rows` under other ids: exactly the pairs (10^6 + j, j, 1.0) of the live ones"""
    rows = np.asarray(rows, np.int64)
    q, c, s = ix.query(rows + 10 ** 6, *rr.pick(v, rows))
    info = ix.removal_info()
    live = rows[~dead[rows]]
    assert sorted(zip(q.tolist(), c.tolist())) == [(int(j) + 10 ** 6, int(j)) for j in np.sort(live)], (rows.size, len(q))
    assert q.size == live.size == ix.result_count() and (s.size == 0 or np.abs(s - 1.0).max() <= TOL)
    assert info["pairs_dropped"] == rows.size - live.size and info["drop_launches"] == 1, info
    return q, c, s


@pytest.mark.parametrize("grid", GRIDS)
def test_drop_list_lengths(monkeypatch, grid):
    v = planted()
    ids = np.arange(P_ROWS, dtype=np.int64)
    for m in LENGTHS_M:
        dead = np.zeros(P_ROWS, bool)
        dead[::3] = True
        dead[m - 1] = True
        with handle(monkeypatch, grid, dim=P_DIM) as ix:
            ix.insert(ids, *v)
            assert ix.remove(ids[dead]) == int(dead.sum())
            assert_planted_call(ix, v, np.arange(m), dead)
            if m == LENGTHS_M[-1]:
                # (rm_grid=1: the one workgroup's 1024 pairs of the first trip, then one more pair)
                gone = assert_planted_call(ix, v, np.nonzero(dead)[0][:300], dead)  # a list dropped entirely
                assert all(a.size == 0 for a in gone) and all(a.size == 0 for a in ix.fetch())
                assert_planted_call(ix, v, np.nonzero(~dead)[0][:301], dead)          # a list that loses nothing
                assert ix.removal_info()["rows_removed"] == int(dead.sum()) > 0
    # a first trip whose 1024 pairs are ALL dropped, with a kept pair behind it: the wave that meets `total == 0` must go on
    dead = np.zeros(P_ROWS, bool)
    dead[:1024] = True
    with handle(monkeypatch, grid, dim=P_DIM) as ix:
        ix.insert(ids, *v)
        assert ix.remove(ids[dead]) == 1024
        kept = assert_planted_call(ix, v, np.arange(1027), dead)
        assert kept[0].size == 3


# ---- 4. compaction
PRUNE_THR = 0.04


def prune_input():
    """the ragged rows scaled by 0.5 .. 4 (the handle normalises them) and the store float64 says they become"""
    rp, idx, val = rr.vectors()
    scales = np.random.default_rng(17).uniform(0.5, 4.0, N)
    val = (val * np.repeat(scales, rr.LEN)).astype(np.float32).astype(np.float64)
    flags = _lib.FLAG_NORMALIZE | _lib.FLAG_VALUE_PRUNE
    batch = (IDS, rp, idx, val)
    assert band_cases([batch], flags, THETA, PRUNE_THR) == []
    ref = reference_store([batch], DIM, flags, theta=THETA, index_threshold=PRUNE_THR)
    kept = np.diff(ref.rowptr)
    assert 0 < int(kept.sum()) < idx.size and int((kept < rr.LEN).sum()) > 100  # it prunes, and not everything
    return (rp, idx, val), (ref.rowptr, ref.indices, ref.values), flags


def head_of(v):
    """the 64 terms most stored rows hold"""
    rp, idx, _ = v
    return np.argsort(-np.bincount(idx[:rp[S]], minlength=DIM), kind="stable")[:64].astype(np.int32)


def live_rows_of(store, live):
    rows = np.nonzero(live)[0]
    rp, idx, val = rr.pick((store.rowptr, store.indices, store.values), rows)
    return store.ext_ids[rows], rp, idx, val


def insert_stored(ix, ext, rp, idx, val):
    """apss_insert_stored_dev: rows out of a store, not filtered again"""
    import torch
    t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rp, idx, val, ext)]
    ix._chk(ix._L.apss_insert_stored_dev(ix._h, ext.size, idx.size, *(C.c_void_p(x.data_ptr() if x.numel() else 0) for x in t)))
    torch.cuda.synchronize()


def assert_same_store(got, ref):
    assert np.array_equal(got.rowptr, ref.rowptr) and np.array_equal(got.indices, ref.indices)
    assert np.array_equal(got.values.view(np.uint32), ref.values.view(np.uint32)) and np.array_equal(got.ext_ids, ref.ext_ids)


def insert_in_batches(ix, v, ids=IDS):
    for a, b in BATCHES:
        ix.insert(ids[a:b], *rr.rows_of(v, a, b))
    assert ix.stats()["build_ms"] == 0  # the last batch waits outside the index
    assert ix.size()[0] == S


def compaction_of_a_config(oracle, monkeypatch, config):
    kw, v_in, v_orc, head = {}, rr.vectors(), None, None
    if config == "prune":
        v_in, v_orc, flags = prune_input()
        kw = dict(flags=flags, index_threshold=PRUNE_THR)
    if config == "head":
        v_in = rr.vectors(1.0)
        head = head_of(v_in)
    if config == "signed":
        v_in = rr.vectors(0.0, True)
        assert (v_in[2][:v_in[0][S]] < 0).any()
    v_orc = v_orc or v_in
    orc = rr.join_of(oracle, v_orc, THETA, S)
    live_pair = ~IS_D[orc[1]]
    rr.class_floors(orc, np.ones(orc[0].size, bool), live_pair)
    _, want, _, _ = rr.split(orc, THETA, np.ones(orc[0].size, bool), live_pair)

    def make(debug=""):
        ix = handle(monkeypatch, debug, **kw)
        if head is not None:
            ix.set_head_terms(head)
        return ix

    with make("rm_grid=1" if config == "plain_rm_grid1" else "") as ix, make() as twin:
        insert_in_batches(ix, v_in)
        stored = read_store(ix)
        if config == "signed":
            ix.self_join(fetch=False)
            assert signed_path(ix.stats()["probe_kernel"]), ix.stats()["probe_kernel"]
        if config == "prune":
            # a second normalisation or prune would change the bits: the stored rows are no unit rows any more, and ...
            assert stored.indices.size == int(v_orc[0][S]) < int(v_in[0][S])
            row = np.repeat(np.arange(S), np.diff(stored.rowptr))
            sq = np.bincount(row, weights=stored.values.astype(np.float64) ** 2, minlength=S)
            again = (stored.values / np.sqrt(sq[row])).astype(np.float32)
            assert int((again.view(np.uint32) != stored.values.view(np.uint32)).sum()) > 1000 and float(sq[sq > 0].min()) < 0.99
            # ... the rows that were scaled up still hold entries that a prune of the RAW input would not have passed twice
            assert int((again <= np.float32(PRUNE_THR)).sum()) == 0 and int((stored.values <= np.float32(PRUNE_THR)).sum()) == 0
        assert ix.remove(IDS[D]) == D.size
        ix.compact()
        info = ix.removal_info()
        assert (info["rows_removed"], info["rows_live"], info["compactions"], info["compacted_rows"]) == (0, S - D.size, 1, D.size)
        # the twin: only ever given the live rows, as the first handle stored them
        live = live_rows_of(stored, ~IS_D[:S])
        assert np.array_equal(live[0], IDS[:S][~IS_D[:S]]) and int((np.diff(live[1]) == 0).sum()) > 50
        if config == "prune":
            insert_stored(twin, *live)
        else:
            twin.insert(live[0], live[1], live[2], live[3].astype(np.float64))
        got, ref = read_store(ix), read_store(twin)
        assert ref.ext_ids.size == S - D.size and ref.indices.size == live[2].size
        assert_same_store(got, ref)
        assert ix.stats()["tiles"] == twin.stats()["tiles"]
        if head is not None:
            assert np.array_equal(ix.head_terms(), head) and np.array_equal(twin.head_terms(), head)
        if config == "signed":
            ix.self_join(fetch=False)
            assert signed_path(ix.stats()["probe_kernel"]), ix.stats()["probe_kernel"]
        pairs = ix.insert_and_query(IDS[S:], *rr.rows_of(v_in, S, N))
        twin_pairs = twin.insert_and_query(IDS[S:], *rr.rows_of(v_in, S, N))
        st, ts = ix.stats(), twin.stats()
        print(config, st["probe_kernel"], "head", st["head_terms"], st["head_flops"], "downgrades", st["downgrades"], "pairs", len(pairs[0]))
        for key in ("probe_kernel", "head_terms", "symmetric", "downgrades", "tiles", "rows", "nnz"):
            assert st[key] == ts[key], key
        assert_same_pairs(to_map(*pairs), rr.by_id(want), THETA)
        assert_same_pairs(to_map(*twin_pairs), rr.by_id(want), THETA)
        assert ix.removal_info()["drop_launches"] == 0  # nothing is marked any more
        if head is not None:
            assert st["head_terms"] == 64 and st["head_flops"] > 0 and np.array_equal(ix.head_terms(), head)
        if config == "signed":
            assert signed_path(st["probe_kernel"])


def compaction_nothing_left(oracle, monkeypatch, config):
    v = rr.vectors()
    rp, idx, val = rr.rows_of(v, S, N)
    oq, oc, os_ = oracle.selfjoin_pairs(DIM, THETA - rr.LOWER, rp, idx, val)
    assert int((np.abs(os_ - THETA) <= rr.LOWER).sum()) == 0 and oq.size >= 50
    want = {(int(IDS[S + a]), int(IDS[S + b])): float(s) for a, b, s in zip(oq, oc, os_)}
    with handle(monkeypatch) as ix:
        insert_in_batches(ix, v)
        assert ix.remove(np.random.default_rng(2).permutation(IDS[:S])) == S
        ix.compact()
        info = ix.removal_info()
        assert ix.size() == (0, 0) and read_store(ix).ext_ids.size == 0
        assert (info["rows_removed"], info["rows_live"], info["compactions"], info["compacted_rows"]) == (0, 0, 1, S)
        assert all(a.size == 0 for a in ix.query(IDS[S:], rp, idx, val))
        ix.insert(IDS[S:], rp, idx, val)
        assert ix.size() == (Q, idx.size)
        assert_same_pairs(to_map(*ix.self_join()), want, THETA)
        assert ix.removal_info()["drop_launches"] == 0


def compaction_of_empty_rows_only(oracle, monkeypatch, config):
    v = rr.vectors()
    empty = np.nonzero(rr.LEN[:S] == 0)[0]
    assert empty.size == 188 and not IS_D[S - 2]
    with handle(monkeypatch) as ix, handle(monkeypatch) as twin:
        insert_in_batches(ix, v)
        stored = read_store(ix)
        assert ix.remove(IDS[empty]) == empty.size
        ix.compact()
        live = live_rows_of(stored, rr.LEN[:S] > 0)
        twin.insert(live[0], live[1], live[2], live[3].astype(np.float64))
        got = read_store(ix)
        assert_same_store(got, read_store(twin))
        assert np.array_equal(got.indices, stored.indices) and got.ext_ids.size == S - empty.size  # the same content, fewer rows
        info = ix.removal_info()
        assert (info["compactions"], info["compacted_rows"], info["rows_live"]) == (1, empty.size, S - empty.size)


COMPACTIONS = dict(plain=compaction_of_a_config, plain_rm_grid1=compaction_of_a_config, prune=compaction_of_a_config,
                   head=compaction_of_a_config, signed=compaction_of_a_config, nothing_left=compaction_nothing_left,
                   empty_rows_only=compaction_of_empty_rows_only)


@pytest.mark.parametrize("config", list(COMPACTIONS))
def test_compaction_ragged(oracle, monkeypatch, config):
    COMPACTIONS[config](oracle, monkeypatch, config)


# ---- 5. paths with marks
def store_with_marks(ix, v):
    ix.insert(IDS[:S], *rr.rows_of(v, 0, S))
    assert ix.remove(IDS[D]) == D.size


def no_dead_end(got, both=True):
    dead_ids = IDS[:S][IS_D[:S]]
    assert not np.isin(got[1], dead_ids).any()
    if both:
        assert not np.isin(got[0], dead_ids).any()


def windowed_self_join(oracle, monkeypatch):
    k = 3
    v = rr.vectors()
    orc, (live, want, dropped, _) = rr.self_expectation(oracle)
    live_ids = (IDS[live[0]], IDS[live[1]], live[2])
    s_idx = v[1][:v[0][S]]
    df = np.bincount(s_idx, minlength=DIM)
    bound = int(np.minimum(np.bincount(np.repeat(np.arange(S), rr.LEN[:S]), weights=df[s_idx], minlength=S), S).sum())  # (apss_window.hpp's b(q))
    lists = {}
    for window in (0, bound // 5):
        with handle(monkeypatch, top_k=k, top_k_window=window) as ix:
            store_with_marks(ix, v)
            got = ix.self_join()
            wi, ri, st = ix.topk_window_info(), ix.removal_info(), ix.stats()
        print("window", window, wi, ri["drop_launches"], ri["pairs_dropped"], st["symmetric"], len(got[0]))
        check_topk(got, live_ids, k, THETA, IDS[:S])
        no_dead_end(got)
        if window:
            assert wi["windows"] >= 3 and 1 <= ri["drop_launches"] <= wi["windows"]
        else:
            assert wi["windows"] == 0 and ri["drop_launches"] == 1 and ri["pairs_dropped"] == dropped
        lists[window] = got
    for a, b in zip(lists[bound // 5], lists[0]):  # element by element the unwindowed list
        assert np.array_equal(a, b)
    assert len(lists[0][0]) >= 500


def regrow_then_drop(oracle, monkeypatch, head_terms):
    zipf = 1.0 if head_terms > 0 else 0.0
    v = rr.vectors(zipf)
    _, (_, want, dropped, _) = rr.self_expectation(oracle, zipf)
    runs = {}
    for debug in ("", "res_cap=64"):
        with handle(monkeypatch, debug, head_terms=head_terms) as ix:
            store_with_marks(ix, v)
            got = ix.self_join()
            runs[debug] = (sorted_list(got), ix.stats(), ix.removal_info())
        st, ri = runs[debug][1:]
        print(head_terms, debug, st["probe_kernel"], "launches", st["probe_launches"], "head", st["head_terms"], st["head_flops"], ri["pairs_dropped"])
        assert st["symmetric"] == 1
        assert_same_pairs(to_map(*got), rr.by_id(want), THETA)
        no_dead_end(got)
        assert ri["pairs_dropped"] == dropped and ri["drop_launches"] == 1
        if head_terms > 0:
            assert st["head_terms"] == 64 and st["head_flops"] > 0
    (a, sa, ra), (b, sb, rb) = runs[""], runs["res_cap=64"]
    assert sb["probe_launches"] > sa["probe_launches"]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    assert ra["pairs_dropped"] == rb["pairs_dropped"]


def virtual_batch(v):
    """40 query rows: 16 of about 600 terms and 16 of about 1,100 -- a live and a dead stored row of 200 terms at weight 1
    plus one or four more at weight 0.3 (the row then scores 0.69 or 0.65 against each of the first two and 0.2 against
    the others) -- and the first 8 non-empty rows of the Q batch"""
    rp, idx, val = v
    long_rows = np.nonzero(rr.LEN[:S] == 200)[0]
    rng = np.random.default_rng(23)
    alive, gone = long_rows[~IS_D[long_rows]], long_rows[IS_D[long_rows]]
    rows = []
    for j in range(32):
        parts = [(rng.choice(alive), 1.0), (rng.choice(gone), 1.0)] + [(r, 0.3) for r in rng.choice(long_rows, 1 if j < 16 else 4, replace=False)]
        acc = np.zeros(DIM)
        for r, w in parts:
            np.add.at(acc, idx[rp[r]:rp[r + 1]], w * val[rp[r]:rp[r + 1]])
        t = np.nonzero(acc)[0]
        rows.append((t.astype(np.int32), acc[t] / np.sqrt((acc[t] ** 2).sum())))
    for r in np.nonzero(rr.LEN[S:] > 0)[0][:8] + S:
        rows.append((idx[rp[r]:rp[r + 1]], val[rp[r]:rp[r + 1]]))
    q_rp = np.concatenate([[0], np.cumsum([len(t) for t, _ in rows])]).astype(np.int64)
    return q_rp, np.concatenate([t for t, _ in rows]).astype(np.int32), np.concatenate([w for _, w in rows])


def virtual_rows(oracle, monkeypatch):
    v = rr.vectors()
    q_rp, q_idx, q_val = virtual_batch(v)
    q_len = np.diff(q_rp)
    # (two rows of 200 terms that are copies of one another share their terms: some unions of six stay below 1,024)
    assert q_len.size == 40 and int((q_len > 512).sum()) == 32 and int((q_len > 1024).sum()) >= 8 and int(q_len.max()) > 1050
    q_ids = (1 << 45) + np.arange(40, dtype=np.int64)
    all_rp = np.concatenate([v[0][:S + 1], v[0][S] + q_rp[1:]])
    orc = oracle.selfjoin_pairs(DIM, THETA - rr.LOWER, all_rp, np.concatenate([v[1][:v[0][S]], q_idx]),
                                np.concatenate([v[2][:v[0][S]], q_val]), S, S + 40)
    visible = orc[1] < S
    assert int((visible & (np.abs(orc[2] - THETA) <= rr.LOWER)).sum()) == 0
    _, want, dropped, _ = rr.split(orc, THETA, visible, ~IS_D[np.minimum(orc[1], S - 1)])
    is_long = q_len[orc[0] - S] > 512
    long_kept = int((visible & is_long & (orc[2] >= THETA) & ~IS_D[np.minimum(orc[1], S - 1)]).sum())
    long_dropped = int((visible & is_long & (orc[2] >= THETA) & IS_D[np.minimum(orc[1], S - 1)]).sum())
    assert min(long_kept, long_dropped) >= 2 * rr.FLOOR and len(want) >= long_kept and dropped >= long_dropped
    want = {(int(q_ids[a - S]), int(IDS[b])): s for (a, b), s in want.items()}
    with handle(monkeypatch) as ix:
        store_with_marks(ix, v)
        got = ix.query(q_ids, q_rp, q_idx, q_val)
        st, ri = ix.stats(), ix.removal_info()
    print("virtual rows:", st["probe_kernel"], len(got[0]), ri["pairs_dropped"])
    assert_same_pairs(to_map(*got), want, THETA)
    no_dead_end(got, both=False)
    assert ri["pairs_dropped"] == dropped and ri["drop_launches"] == 1


def waiting_rows(oracle, monkeypatch):
    v = rr.vectors()
    indexed = S - 200
    assert IS_D[:indexed].sum() > 400 and IS_D[indexed:S].sum() > 60  # marks among the indexed rows and among the waiting ones
    wants = {frozen: rr.batch_expectation(oracle, frozen=frozen)[1] for frozen in (True, False)}
    lists = {}
    for debug in ("", "no_tail"):
        with handle(monkeypatch, debug) as ix:
            ix.insert(IDS[:indexed], *rr.rows_of(v, 0, indexed))
            for a in range(indexed, S, 40):
                ix.insert(IDS[a:a + 40], *rr.rows_of(v, a, a + 40))
                assert (ix.stats()["build_ms"] == 0) == (debug == "")  # the batch waits outside the index, or extends it at once
            assert ix.remove(IDS[D]) == D.size
            for frozen in (True, False):
                _, want, dropped, _ = wants[frozen]
                got = (ix.query if frozen else ix.insert_and_query)(IDS[S:], *rr.rows_of(v, S, N))
                ri = ix.removal_info()
                assert_same_pairs(to_map(*got), rr.by_id(want), THETA)
                no_dead_end(got, both=False)
                assert ri["pairs_dropped"] == dropped and ri["drop_launches"] == 1, (debug, frozen, ri)
                lists[debug, frozen] = set(zip(got[0].tolist(), got[1].tolist()))
    for frozen in (True, False):
        assert lists["", frozen] == lists["no_tail", frozen]


def auto_compact_head(oracle, monkeypatch):
    B, f = 250, 0.25
    v = rr.vectors(1.0)
    orc = rr.whole_join(oracle, 1.0)
    oq, oc, os_ = orc
    n_batches = N // B
    wants, kept, gone = [], np.zeros(0, np.int64), np.zeros(0, np.int64)
    for i in range(n_batches):
        visible = (oq >= i * B) & (oq < (i + 1) * B) & (oc < (i + 1) * B)
        live = oc >= (i - 3) * B  # batches 0 .. i - 4 were removed
        _, want, _, band = rr.split(orc, THETA, visible, live)
        assert band == 0
        wants.append(rr.by_id(want))
        kept = np.concatenate([kept, oc[visible & live & (os_ >= THETA)]])
        gone = np.concatenate([gone, oc[visible & ~live & (os_ >= THETA)]])
    for n in rr.CLASSES:  # the module's floors, over the whole stream
        assert int((rr.LEN[kept] == n).sum()) >= rr.FLOOR and int((rr.LEN[gone] == n).sum()) >= rr.FLOOR, n
    flops = 0.0
    with handle(monkeypatch, head_terms=64, auto_compact=f) as ix:
        for i in range(n_batches):
            got = ix.insert_and_query(IDS[i * B:(i + 1) * B], *rr.rows_of(v, i * B, (i + 1) * B))
            assert_same_pairs(to_map(*got), wants[i], THETA)
            st, info = ix.stats(), ix.removal_info()
            rows = ix.size()[0]
            assert rows <= 1583 and info["rows_removed"] <= f * (rows - B) + 1e-9, (i, rows, info)
            assert st["head_terms"] == 64, (i, st)
            flops += st["head_flops"]
            if i >= 3:
                assert ix.remove(IDS[(i - 3) * B:(i - 2) * B]) == B
        info = ix.removal_info()
    print("stream with a head:", info)
    assert info["compactions"] >= 1 and info["removed_total"] == (n_batches - 3) * B and flops > 0


PATHS = dict(windowed_self_join=windowed_self_join, regrow_no_head=lambda o, m: regrow_then_drop(o, m, -1),
             regrow_head64=lambda o, m: regrow_then_drop(o, m, 64), virtual_rows=virtual_rows, waiting_rows=waiting_rows,
             auto_compact_head=auto_compact_head)


@pytest.mark.parametrize("case", list(PATHS))
def test_paths_with_marks(oracle, monkeypatch, case):
    PATHS[case](oracle, monkeypatch)
