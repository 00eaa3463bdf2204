"""The adding waves of k_probe_even (csrc/apss_even.hpp) with fewer vector instructions per posting slot: a batch's crossings
found through the MAXIMUM of old + product, idle lanes whose spare word is kept small and non-zero instead of having their
returned value replaced, first touches counted through their complement, and strip entries invalidated by the wave that read
them instead of a range test per window step.  Each shortcut has a corner where it would show as a lost or doubled pair or
as a candidate count that is off: thresholds of a few units (an idle lane's sum passes them), strips that hold descriptors
of an earlier, longer round, tens of thousands of rounds on one spare word, adds that land on a sum which has already
crossed.  Every case checks that k_probe_even ran and compares pairs, scores, posting visits and candidate pairs with the
oracle's."""
import numpy as np
import pytest

from helpers import assert_same_pairs, to_map

pytestmark = pytest.mark.gpu


def _csr(rows):
    rp = np.zeros(len(rows) + 1, np.int64)
    for i, (t, _) in enumerate(rows):
        rp[i + 1] = rp[i] + len(t)
    idx = np.concatenate([np.asarray(t) for t, _ in rows]).astype(np.int32)
    val = np.concatenate([np.asarray(w, np.float64) for _, w in rows])
    return rp, idx, val


def _unit(w):
    w = np.asarray(w, np.float64)
    return w / np.linalg.norm(w)


def _terms(rng, lo, hi, k):
    return np.sort(rng.choice(np.arange(lo, hi), size=k, replace=False)).astype(np.int32)


def _join(oracle, dim, theta, rp, idx, val, band=1e-5, tile_rows=2048):
    """one whole-batch insert_and_query against the oracle: the same pairs (each once), scores to 1e-5, the reference's
    posting visits and the exact number of distinct (q, c != q) pairs sharing a term"""
    from apss.engine import ApssIndex
    n = len(rp) - 1
    want = to_map(*oracle.selfjoin_pairs(dim, theta, rp, idx, val))
    with ApssIndex(dim, theta, head_terms=-1, tile_rows=tile_rows) as ix:
        q, c, s = ix.insert_and_query(np.arange(n, dtype=np.int64), rp, idx, val)
        st = ix.stats()
    got = to_map(q, c, s)
    ref = oracle.selfjoin_sample(1, dim, theta, rp, idx, val, 0, n, 2)
    print("kernel %s | pairs %d (oracle %d) | visits %d (oracle %d) | candidates %d (oracle %d) | survivors %d" % (
        st["probe_kernel"], len(q), len(want), st["posting_visits"], ref["visits"], st["candidate_pairs"], ref["cand_pairs"],
        st["filter_survivors"]))
    assert st["probe_kernel"].startswith("k_probe_even<") and st["thin_launches"] > 0, st["probe_kernel"]
    assert len(got) == len(q), "a pair reported twice"
    assert_same_pairs(got, want, theta, band=band, tol=1e-5)
    assert st["posting_visits"] == ref["visits"]
    assert st["candidate_pairs"] == ref["cand_pairs"]
    return want, st


@pytest.fixture(scope="module")
def sparse_rows():
    """2,048 rows of one to three terms over 512: nearly every slot of a window is an idle lane's"""
    rng = np.random.default_rng(811)
    rows = []
    for _ in range(2048):
        k = int(rng.integers(1, 4))
        rows.append((_terms(rng, 0, 512, k), _unit(10.0 ** rng.uniform(-3, 0, size=k))))
    return _csr(rows)


@pytest.mark.parametrize("units", [1, 2, 3, 13])
def test_thresholds_of_a_few_units(oracle, sparse_rows, units):
    """unit rows take 2^15 units per 1.0; the coarse threshold is floor(theta 2^15 (1 - 2^-11 - 1e-6)) - 2 units.  At a few
    units the sum of an idle lane (its spare word's count + 1) passes the threshold, so every batch goes through the exact
    test: no crossing may be reported for an idle lane, none lost, and the idle lanes count as no first touch"""
    rp, idx, val = sparse_rows
    theta = (units + 2 + 0.002) / 32768.0 / (1.0 - 2.0 ** -11 - 1e-6)
    want, st = _join(oracle, 512, theta, rp, idx, val, band=1e-6)
    assert len(want) > 5000 and st["filter_survivors"] >= len(want)


@pytest.fixture(scope="module")
def alternating_rows():
    """rows of 128 terms alternate with rows of one term: the strip a one-term round reads was filled by a 128-term round
    three rounds earlier.  A twelfth of the long rows are noisy copies of another, the one-term rows share 300 terms"""
    rng = np.random.default_rng(812)
    dim, n = 16384, 2048
    rows = []
    for i in range(n):
        if i % 2 == 0:
            if i > 100 and rng.random() < 1.0 / 12:
                t, w = rows[2 * int(rng.integers(0, i // 2))]
                rows.append((t, _unit(w * (1.0 + 0.05 * rng.standard_normal(w.size)))))
            else:
                rows.append((_terms(rng, 0, dim, 128), _unit(np.abs(rng.standard_normal(128)) + 0.1)))
        else:
            rows.append((_terms(rng, 0, 300, 1), np.ones(1)))
    return (dim,) + _csr(rows)


@pytest.mark.parametrize("chunks", [2048, 1024, 683, 1])
def test_stale_strip_slots_are_not_loaded(oracle, monkeypatch, alternating_rows, chunks):
    """chunks of one, two and three queries with a short last chunk, and one workgroup for the whole batch: a descriptor left
    in a strip and loaded again would show as extra visits of its postings -- extra first touches, and sums that cross"""
    monkeypatch.setenv("APSS_DEBUG", "chunks=%d" % chunks)
    dim, rp, idx, val = alternating_rows
    # (filter tiles are twice tile_rows: one 2048-row tile, eight postings per term -- where a plain handle's rounds fit the
    # six adding waves' windows; at 4096 rows the library keeps k_probe_coarse)
    want, _ = _join(oracle, dim, 0.6, rp, idx, val, tile_rows=1024)
    assert len(want) > 1000


def test_spare_words_are_reset_every_round(oracle, monkeypatch):
    """one workgroup, 8,192 rounds of two terms each on one tile: ~28 idle adds per lane number and round would take a spare
    word past 2^16 -- its low half back to zero, an idle lane counted as a first touch -- were it not set to 1 every round"""
    monkeypatch.setenv("APSS_DEBUG", "chunks=1")
    rng = np.random.default_rng(813)
    rows = [(_terms(rng, 0, 4096, 2), _unit(np.abs(rng.standard_normal(2)) + 0.1)) for _ in range(8192)]
    rp, idx, val = _csr(rows)
    want, st = _join(oracle, 4096, 0.8, rp, idx, val, tile_rows=8192)
    assert len(want) > 100 and st["tiles"] == 1


def test_repeated_touches_and_adds_after_the_crossing(oracle):
    """64 groups of 8 identical rows of 40 terms among 2,000 random rows: every pair of a group crosses half-way through the
    row and is added to 20 more times, often twice within one batch: each pair once, each (q, c) one first touch"""
    rng = np.random.default_rng(814)
    dim = 8000
    rows = [(_terms(rng, 0, dim, 40), _unit(np.abs(rng.standard_normal(40)) + 0.1)) for _ in range(2000)]
    for _ in range(64):
        t, w = _terms(rng, 0, dim, 40), _unit(np.abs(rng.standard_normal(40)) + 0.1)
        for _ in range(8):
            rows.insert(int(rng.integers(0, len(rows) + 1)), (t, w))
    rp, idx, val = _csr(rows)
    want, _ = _join(oracle, dim, 0.5, rp, idx, val)
    assert len(want) >= 64 * 8 * 7


@pytest.mark.parametrize("debug,acc8", [("", "true>"), ("no_acc8", "false>")])
def test_the_1024_thread_kernels(oracle, monkeypatch, debug, acc8):
    """a sparse regime (four postings per term and 32768 rows): 131072-row tiles with 8-bit accumulators, four to a word, and
    65536-row tiles with 16-bit ones addressed by slot -- the other forms of the address, the shift and the extracted half"""
    monkeypatch.setenv("APSS_DEBUG", debug)
    from apss import synth
    n, dim, nnz, theta = 4000, 65536, 8, 0.7
    rp, idx, val = synth.make_vectors(n, dim, nnz, 0.0, seed=815, dup_frac=0.2)
    want, st = _join(oracle, dim, theta, rp, idx, val, tile_rows=0)
    assert st["probe_kernel"].startswith("k_probe_even<1024, ") and st["probe_kernel"].endswith(acc8), st["probe_kernel"]
    assert len(want) > 300


def _restrict(rp, idx, val, lo, hi):
    """the batch with only its terms in [lo, hi): what one term shard indexes"""
    keep = (idx >= lo) & (idx < hi)
    row = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    rp2 = np.zeros(len(rp), np.int64)
    np.cumsum(np.bincount(row[keep], minlength=len(rp) - 1), out=rp2[1:])
    return rp2, idx[keep], val[keep]


def _shard_join(oracle, dim, theta, rp, idx, val, world, tile_rows):
    import torch
    from apss.dist import HipShardEngine, join_shards_local, term_ranges
    n = len(rp) - 1
    want = to_map(*oracle.selfjoin_pairs(dim, theta, rp, idx, val))
    ranges = term_ranges(np.bincount(idx, minlength=dim), world)
    engines = [HipShardEngine(dim, theta, tr, torch.device("cuda", 0), tile_rows=tile_rows) for tr in ranges]
    for e in engines:
        e.load(rp, idx, val)
    q, c, s, _ = join_shards_local(engines, n, theta)
    assert len(to_map(q, c, s)) == len(q), "a pair reported twice"
    assert_same_pairs(to_map(q, c, s), want, theta)
    refs = [oracle.selfjoin_sample(1, dim, theta, *_restrict(rp, idx, val, lo, hi), 0, n, 2) for lo, hi in ranges]
    for e, ref in zip(engines, refs):
        print("kernel %s | rows per round %d | visits %d (oracle %d) | candidates %d (oracle, one row per round: %d)" % (
            e.stats["probe_kernel"], e.stats["queries_per_round"], e.stats["posting_visits"], ref["visits"],
            e.stats["candidate_pairs"], ref["cand_pairs"]))
        assert e.stats["probe_kernel"].startswith("k_probe_even") and e.stats["thin_launches"] > 0, e.stats["probe_kernel"]
        assert e.stats["posting_visits"] == ref["visits"]
    return want, engines, refs


def test_stale_strip_slots_under_the_shard_rule(oracle, monkeypatch, alternating_rows):
    """the alternating rows cut into four term ranges: the shard-rule instantiations skip the window steps behind a wave's
    last chunk, so the slots tested are counted per round from the steps taken"""
    monkeypatch.setenv("APSS_DEBUG", "chunks=683,merge=0")  # (one row per round: the merged instantiations have a case of their own)
    dim, rp, idx, val = alternating_rows
    want, engines, refs = _shard_join(oracle, dim, 0.6, rp, idx, val, 4, 1024)
    assert len(want) > 1000
    for e, ref in zip(engines, refs):
        assert e.stats["probe_kernel"].startswith("k_probe_even<") and e.stats["queries_per_round"] == 1
        assert e.stats["candidate_pairs"] == ref["cand_pairs"]


@pytest.mark.parametrize("debug,tile_rows,acc8,merged", [("merge=0", 1024, False, False), ("", 1024, False, True),
                                                         ("merge=0", 0, True, False), ("", 0, True, True)])
def test_merged_and_8_bit_instantiations(oracle, monkeypatch, debug, tile_rows, acc8, merged):
    """term shards of 64-term rows, as tests/test_gpu_merged_rounds.py makes the library merge: one row per round and two, with
    16-bit accumulators over 1024-row tiles and with 8-bit ones over one 65536-row tile.  One row per round: the candidate
    count is the oracle's for the shard's terms.  Two rows per round share their accumulators: a round's first touches are
    the candidates EITHER row touches, so the count lies between half the oracle's and the oracle's"""
    monkeypatch.setenv("APSS_DEBUG", debug)
    from apss import synth
    n, dim, nnz, theta, world = 4096, 60_000, 64, 0.7, 4
    rp, idx, val = synth.make_vectors(n, dim, nnz, 0.0, seed=816, dup_frac=0.05)
    idx, val = idx.reshape(n, nnz).copy(), val.reshape(n, nnz).copy()
    rng = np.random.default_rng(817)
    for a in rng.choice(n - 1, size=n // 40, replace=False):  # near-duplicates of the NEXT row: inside a round of two, or across two
        idx[a + 1], val[a + 1] = idx[a], _unit(val[a] * rng.uniform(0.95, 1.05, size=nnz))
    idx, val = idx.reshape(-1), val.reshape(-1)
    want, engines, refs = _shard_join(oracle, dim, theta, rp, idx, val, world, tile_rows)
    assert len(want) > 150
    for e, ref in zip(engines, refs):
        name = e.stats["probe_kernel"]
        assert name.startswith("k_probe_even_merged<") == merged and name.endswith("true>") == acc8, name
        if merged:
            assert e.stats["queries_per_round"] == 2
            assert ref["cand_pairs"] // 2 <= e.stats["candidate_pairs"] <= ref["cand_pairs"]
        else:
            assert e.stats["candidate_pairs"] == ref["cand_pairs"]
