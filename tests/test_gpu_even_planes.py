"""k_probe_planes (csrc/apss_even.hpp, TWO): the plain 512-thread thin-round filter with two planes of 8-bit sums and ONE
barrier per round -- round v adds into plane v mod 2 and clears round v - 1 on the other plane, from the posting registers
that still hold it, directly ahead of its own adds.  What can go wrong is a clear that is missing, late, or on the wrong plane
(a sum that starts above zero: a false pair, and a first touch that is not counted), a plane that is not zero when the next
item of a persistent workgroup starts, and barriers that do not pair between the staging and the adding waves.

Every case runs twice, with APSS_DEBUG=planes (the library itself takes the kernel for query chunks of 256 rounds or more; the
token takes it for any) and with APSS_DEBUG=no_planes (k_probe_even's 16-bit sums), and checks both
against the oracle: the same pairs (each once), scores to 1e-5, the reference's posting visits and the exact number of distinct
(q, c != q) pairs that share a term; the kernel's name is asserted in both runs."""
import math
import re

import numpy as np
import pytest

from helpers import assert_same_pairs, to_map

pytestmark = pytest.mark.gpu

DIM = 2000
TILE = 1024        # tile_rows of every handle here
FTILE = 2 * TILE   # ... whose filter tiles are two of them
PLANES = r"k_probe_even<512, (\d), 128, false, false, true, planes>$"
PLAIN = r"k_probe_even<512, (\d), 128, false, false, false>$"


def _unit(w):
    w = np.asarray(w, np.float64)
    return w / np.linalg.norm(w)


def _csr(rows):
    rp = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(t) for t, _ in rows], out=rp[1:])
    idx = np.concatenate([np.asarray(t) for t, _ in rows]).astype(np.int32)
    val = np.concatenate([np.asarray(w, np.float64) for _, w in rows])
    return rp, idx, val


def _row(rng, lo=0, hi=DIM):
    k = int(rng.integers(16, 25))
    t = np.sort(rng.choice(np.arange(lo, hi), size=k, replace=False)).astype(np.int32)
    return t, _unit(np.abs(rng.standard_normal(k)) + 0.1)


def _noisy(rng, row):
    t, w = row
    return t, _unit(w * (1.0 + 0.05 * rng.standard_normal(w.size)))


def _random_rows(rng, n, dup):
    rows = []
    for i in range(n):
        rows.append(_noisy(rng, rows[int(rng.integers(0, i))]) if i > 20 and rng.random() < dup else _row(rng))
    return rows


def _reference(oracle, theta, rp, idx, val, dim=DIM):
    n = len(rp) - 1
    return (to_map(*oracle.selfjoin_pairs(dim, theta, rp, idx, val)), oracle.selfjoin_sample(1, dim, theta, rp, idx, val, 0, n, 2))


def _run(monkeypatch, debug, theta, rp, idx, val, flags=0, dim=DIM):
    from apss.engine import ApssIndex
    monkeypatch.setenv("APSS_DEBUG", debug)
    n = len(rp) - 1
    with ApssIndex(dim, theta, head_terms=-1, tile_rows=TILE, flags=flags) as ix:
        q, c, s = ix.insert_and_query(np.arange(n, dtype=np.int64), rp, idx, val)
        st = ix.stats()
    o = np.lexsort((c, q))
    return (q[o], c[o], s[o]), st


def _both(monkeypatch, reference, theta, rp, idx, val, debug="", flags=0, name=True, dim=DIM):
    """the two-plane kernel and its no_planes twin against the reference; returns the two stats"""
    want, ref = reference
    out = []
    for twin in (False, True):
        pairs, st = _run(monkeypatch, ",".join(x for x in (debug, "no_planes" if twin else "planes") if x), theta, rp, idx, val, flags, dim)
        print("%s | pairs %d (oracle %d) | visits %d (oracle %d) | candidates %d (oracle %d) | survivors %d | downgrades %d" % (
            st["probe_kernel"], len(pairs[0]), len(want), st["posting_visits"], ref["visits"], st["candidate_pairs"],
            ref["cand_pairs"], st["filter_survivors"], st["downgrades"]))
        if name:
            assert re.match(PLAIN if twin else PLANES, st["probe_kernel"]), st["probe_kernel"]
            assert st["thin_launches"] > 0 and st["downgrades"] == 0 and st["filter_tile_rows"] == FTILE
        got = to_map(*pairs)
        assert len(got) == len(pairs[0]), "a pair reported twice"
        assert_same_pairs(got, want, theta)
        assert st["posting_visits"] == ref["visits"]
        assert st["candidate_pairs"] == ref["cand_pairs"]
        out.append((pairs, st))
    for a, b in zip(out[0][0], out[1][0]):
        assert a.tobytes() == b.tobytes()
    if name:  # the same window, the same work list
        assert re.match(PLANES, out[0][1]["probe_kernel"]).group(1) == re.match(PLAIN, out[1][1]["probe_kernel"]).group(1)
        assert out[0][1]["query_chunk"] == out[1][1]["query_chunk"]
    return out[0][1], out[1][1]


# ---- 1. chunk shapes: items of one, two and three rounds, a short last chunk, one- and two-row batches

@pytest.mark.parametrize("n,chunks,q_chunk", [(2047, 2047, 1), (2047, 1024, 2), (2048, 683, 3), (1000, 334, 3), (777, 1, 777), (2, 2, 1), (1, 1, 1)])
def test_chunk_shapes_pin_the_barrier_pairing(oracle, monkeypatch, n, chunks, q_chunk):
    """the staging and the adding waves run different loops around the same ONE barrier per round; the adding waves' loop is
    unrolled by two (the plane is a constant of each half) and leaves after an odd last round, and the last round's clear comes
    behind the loop, from whichever register set holds it.  Chunks of one query, of two, of three (odd and even item lengths),
    a short last chunk (2047 = 1023 x 2 + 1, 2048 = 682 x 3 + 2, 1000 = 333 x 3 + 1), one chunk of everything, tiny batches"""
    from apss import _lib
    rp, idx, val = _csr(_random_rows(np.random.default_rng(7100 + n + chunks), max(n, 2), 0.2))
    rp, idx, val = rp[:n + 1], idx[:rp[n]], val[:rp[n]]
    theta = 0.6
    planes, plain = _both(monkeypatch, _reference(oracle, theta, rp, idx, val), theta, rp, idx, val, debug="chunks=%d" % chunks,
                          flags=_lib.FLAG_NO_SYMMETRY, name=n > 100)
    if n > 100:
        assert planes["query_chunk"] == q_chunk and planes["symmetric"] == 0
        assert planes["result_pairs"] > 20


# ---- 2. the same candidates in consecutive rounds and in rounds two apart

@pytest.fixture(scope="module")
def block_rows():
    """groups of seven stored neighbours A A B A B B B (A, B two unrelated rows): rounds v and v + 1 meet the same candidates
    (they share a plane only if a clear was missed), rounds v and v + 2 meet them on the SAME plane with one clear between"""
    rng = np.random.default_rng(7201)
    rows = []
    while len(rows) < 3000:
        a, b = _row(rng), _row(rng)
        rows += [a, a, b, a, b, b, b]
    return _csr(rows)


@pytest.fixture(scope="module")
def block_reference(oracle, block_rows):
    return _reference(oracle, 0.7, *block_rows)


@pytest.mark.parametrize("debug", ["", "chunks=3", "chunks=1000"])
def test_same_candidates_in_neighbouring_rounds(monkeypatch, block_rows, block_reference, debug):
    planes, _ = _both(monkeypatch, block_reference, 0.7, *block_rows, debug=debug)
    assert planes["result_pairs"] >= (len(block_rows[0]) - 1) // 7 * 18  # (6 ordered pairs among the three copies of A, 12 among B's four)


# ---- 3. a rare round between ordinary ones

HEAVY = DIM - 1
POPULAR = (DIM - 41, DIM - 1)  # 40 terms that every "wide" row takes 24 of


@pytest.fixture(scope="module")
def rare_rows():
    """two filter tiles of 2,048 rows.  HEAVY's segment in the first is a long one (300 rows: more than 256 postings, swept by
    the whole workgroup); in the second tile every ninth row holds it, between two near-copies of itself that do not:
    ordinary, rare, ordinary on the same candidates.  Every third of a tile's first 600 rows (those triples apart) is a
    `wide` row, 24 of 40 popular terms whose segments run to eight chunks each: more chunks than the register windows hold
    (whole-plane clear without a sweep)"""
    rng = np.random.default_rng(7301)
    rows = _random_rows(rng, 2 * FTILE, 0.1)
    rows = [(t[t < POPULAR[0]], w[t < POPULAR[0]]) for t, w in rows]
    rows = [(t, _unit(w)) for t, w in rows]
    with_heavy = lambda r: (np.append(r[0], HEAVY).astype(np.int32), _unit(np.append(r[1], 0.3)))
    for i in rng.choice(FTILE, 300, replace=False):
        rows[i] = with_heavy(rows[i])
    first = FTILE + 6
    for i in range(first, 2 * FTILE - 8, 9):
        rows[i - 1] = _noisy(rng, rows[i])
        rows[i + 1] = _noisy(rng, rows[i])
        rows[i] = with_heavy(rows[i])
    for i in range(3, 2 * FTILE, 3):
        if i % FTILE < 600 and HEAVY not in rows[i][0] and not (i >= first - 1 and (i - first + 1) % 9 < 3):
            t = np.sort(rng.choice(np.arange(*POPULAR), size=24, replace=False)).astype(np.int32)
            rows[i] = (t, _unit(np.abs(rng.standard_normal(24)) + 0.1))
    return _csr(rows)


@pytest.fixture(scope="module")
def rare_reference(oracle, rare_rows):
    return _reference(oracle, 0.6, *rare_rows)


@pytest.mark.parametrize("debug", ["", "chunks=8"])
def test_a_rare_round_between_ordinary_ones(monkeypatch, rare_rows, rare_reference, debug):
    """a rare round's whole-plane clear happens one round late, at the top of the next round, which is adding to the other plane"""
    rp, idx, val = rare_rows
    row = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    holders = row[idx == HEAVY]
    assert (holders < FTILE).sum() > 256 and 100 < (holders >= FTILE).sum() <= 256
    from apss import _lib
    _both(monkeypatch, rare_reference, 0.6, rp, idx, val, debug=debug, flags=_lib.FLAG_NO_SYMMETRY)


# ---- 4. consecutive items in one workgroup

@pytest.mark.parametrize("data,debug", [("block", "chunks=41,persist_fine=16,persist_wgs=1"), ("block", "chunks=600,persist_wgs=1"),
                                        ("rare", "chunks=32,persist_fine=32,persist_wgs=1"), ("rare", "chunks=586,persist_wgs=2")])
def test_consecutive_items_in_one_workgroup(monkeypatch, request, data, debug):
    """one persistent workgroup takes every item: an item finds the planes as the last one left them -- both zero, whichever
    plane its last round used (items of odd and of even length, items that end with a rare round)"""
    from apss import _lib
    rows = request.getfixturevalue(data + "_rows")
    theta = 0.7 if data == "block" else 0.6
    _both(monkeypatch, request.getfixturevalue(data + "_reference"), theta, *rows, debug=debug,
          flags=_lib.FLAG_NO_SYMMETRY if data == "rare" else 0)


# ---- 5. the threshold at its minimum

def test_threshold_at_the_minimum(oracle, monkeypatch):
    """rows of norm 2: |q||c| = 4 leaves room for 2^5 units per 1.0 in a byte (4 x 64 = 256 does not fit), and theta is chosen so
    that the threshold is 14 units, the least the library takes byte sums for (12 after the coarse slack of 2).  An idle
    lane's spare sum is of that size: every batch goes through the exact test"""
    rp, idx, val = _csr(_random_rows(np.random.default_rng(7501), 3000, 0.15))
    val = val * 2.0
    shrink = 1.0 - 2.0 ** -11 - 1e-6
    theta = 14.3 / 32.0 / shrink
    assert math.floor(theta * 32.0 * shrink) == 14 and math.floor(theta * 64.0 * shrink) > 14
    planes, _ = _both(monkeypatch, _reference(oracle, theta, rp, idx, val), theta, rp, idx, val)
    assert planes["result_pairs"] > 500


# ---- 6. the latch

def test_unselective_byte_sums_latch_back_without_a_rebuild(oracle, monkeypatch):
    """eight interleaved groups of rows (a group's shared terms: 256 postings per filter tile, no long segment); a group's rows
    share 16 terms that carry 0.76 of every row's squared norm in equal parts, the rest lies on four terms of the row's own.
    Two rows of a group score 0.76 < theta = 0.8, but in byte sums every shared term is floor(128 x 0.76 / 16) + 1 = 7 units and
    16 x 7 = 112 passes the threshold of 100: all 6,144^2 / 8 = 4.7M pairs inside the groups survive the 8-bit filter, more
    than the guard's 4M.  The handle must answer through the 16-bit kernel, say so in
    `downgrades`, and build no index for it (build_ms is written by an index build only)"""
    from apss import _lib
    from apss.engine import ApssIndex
    rng = np.random.default_rng(7601)
    n, groups, theta = 6144, 8, 0.8
    rows = []
    for i in range(n):
        if i >= 64 and rng.random() < 0.05:  # a near-copy of an earlier row of the group: the pairs to report
            t, w = rows[i - groups * int(rng.integers(1, 16))]
            rows.append((t, _unit(w * (1.0 + 0.02 * rng.standard_normal(w.size)))))
            continue
        g = i % groups
        own = rng.choice(np.arange(16 * groups, DIM), size=4, replace=False)
        t = np.concatenate([np.arange(16 * g, 16 * g + 16), own]).astype(np.int32)
        w = np.concatenate([np.full(16, math.sqrt(0.76 / 16)), np.full(4, math.sqrt(0.24 / 4))])
        o = np.argsort(t)
        rows.append((t[o], w[o]))
    rp, idx, val = _csr(rows)
    want = to_map(*oracle.selfjoin_pairs(DIM, theta, rp, idx, val))
    assert 100 < len(want) < 100000
    monkeypatch.setenv("APSS_DEBUG", "no_tail,planes")
    with ApssIndex(DIM, theta, head_terms=-1, tile_rows=TILE) as ix:
        ix.insert(np.arange(n, dtype=np.int64), rp, idx, val)
        before = ix.stats()
        q, c, s = ix.self_join()
        st = ix.stats()
        q2, c2, s2 = ix.self_join()  # latched: straight to the 16-bit kernel
        st2 = ix.stats()
    print(st["probe_kernel"], "survivors", st["filter_survivors"], "pairs", len(q), "downgrades", st["downgrades"], "build_ms", before["build_ms"], st["build_ms"])
    assert before["downgrades"] == 0 and before["build_ms"] > 0
    assert st["downgrades"] & _lib.DOWNGRADE_ACC8 and re.match(PLAIN, st["probe_kernel"]), (st["downgrades"], st["probe_kernel"])
    assert st["build_ms"] == before["build_ms"] == st2["build_ms"] and st["tiles"] == before["tiles"]
    got = to_map(q, c, s)
    assert len(got) == len(q)
    assert_same_pairs(got, want, theta)
    assert_same_pairs(to_map(q2, c2, s2), want, theta)
    assert st2["probe_kernel"] == st["probe_kernel"] and st["filter_survivors"] < 4000000


# ---- the library's own choice

@pytest.mark.parametrize("chunks,planes", [(8, True), (41, False)])
def test_default_choice_by_chunk_length(monkeypatch, block_rows, block_reference, chunks, planes):
    """without a token the two-plane kernel takes query chunks of 256 rounds or more (3,003 rows in 8 chunks: 376 rounds) and
    leaves shorter ones (41 chunks: 74 rounds) to the 16-bit kernel"""
    want, ref = block_reference
    pairs, st = _run(monkeypatch, "chunks=%d" % chunks, 0.7, *block_rows)
    assert re.match(PLANES if planes else PLAIN, st["probe_kernel"]), st["probe_kernel"]
    assert (st["query_chunk"] >= 256) == planes and st["downgrades"] == 0
    assert_same_pairs(to_map(*pairs), want, 0.7)
    assert st["posting_visits"] == ref["visits"] and st["candidate_pairs"] == ref["cand_pairs"]
