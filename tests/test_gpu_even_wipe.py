"""k_probe_planes<5> and <6> (csrc/apss_even.hpp, WIPE): windows of five and six steps keep their two planes of 8-bit sums
32,768 bytes apart and clear the idle plane WHOLE, by ds_write_addtid_b32 stores of zeros dealt over all eight waves, where the
narrower windows clear posting by posting.  What can go wrong: a wipe that is missing, on the wrong plane, short of the tile's
last rows, or not landed before the barrier (a sum that starts above zero: a false pair, and a first touch that is not
counted); a plane that is not zero when the next item of a persistent workgroup starts; a store that runs into the live plane.

The existing two-plane tests use rows of 16 to 24 terms and never reach five steps.  Here every row has exactly 100 terms
(the flagship's), tile_rows = 1024 (filter tiles of 2,048 rows), three filter tiles, and the dimension puts 25 to 30 postings
into a (tile, term) segment: dim 8000 takes the five-step window, dim 6800 the six-step one (plan_filter(): 105 chunks-per-term
x terms over 48 slots per step) -- asserted through the kernel's name.  One case has filter tiles of 32,768 rows, the only
size at which every store of a wipe is issued.

Every case runs twice, with APSS_DEBUG=planes and with APSS_DEBUG=no_planes (k_probe_even's 16-bit sums), and checks both against
the oracle: the same pairs (each once), scores to 1e-5, the reference's posting visits and the exact number of distinct
(q, c != q) pairs that share a term; the two runs' outputs are byte-identical."""
import re

import numpy as np
import pytest

from helpers import assert_same_pairs, to_map

pytestmark = pytest.mark.gpu

NNZ = 100
TILE = 1024        # tile_rows of every handle here
FTILE = 2 * TILE   # ... whose filter tiles are two of them
N = 3 * FTILE
DIMS = {5: 8000, 6: 6800}  # window steps -> dimension
PLANES = r"k_probe_even<512, (\d), 128, false, false, true, planes>$"
PLAIN = r"k_probe_even<512, (\d), 128, false, false, false>$"
N_POPULAR = 40  # the terms below HEAVY that only `wide` rows hold


def _unit(w):
    w = np.asarray(w, np.float64)
    return w / np.linalg.norm(w)


def _csr(rows):
    assert all(len(t) == NNZ and len(set(t.tolist())) == NNZ for t, _ in rows)
    rp = np.arange(len(rows) + 1, dtype=np.int64) * NNZ
    idx = np.concatenate([np.asarray(t) for t, _ in rows]).astype(np.int32)
    val = np.concatenate([np.asarray(w, np.float64) for _, w in rows])
    return rp, idx, val


def _row(rng, hi):
    t = np.sort(rng.choice(hi, size=NNZ, replace=False)).astype(np.int32)
    return t, _unit(np.abs(rng.standard_normal(NNZ)) + 0.1)


def _noisy(rng, row):
    t, w = row
    return t, _unit(w * (1.0 + 0.05 * rng.standard_normal(w.size)))


def _reference(oracle, dim, theta, rp, idx, val):
    n = len(rp) - 1
    return (to_map(*oracle.selfjoin_pairs(dim, theta, rp, idx, val)), oracle.selfjoin_sample(1, dim, theta, rp, idx, val, 0, n, 2))


def _run(monkeypatch, debug, dim, theta, rp, idx, val, flags, tile=TILE):
    from apss.engine import ApssIndex
    monkeypatch.setenv("APSS_DEBUG", debug)
    n = len(rp) - 1
    with ApssIndex(dim, theta, head_terms=-1, tile_rows=tile, flags=flags) as ix:
        q, c, s = ix.insert_and_query(np.arange(n, dtype=np.int64), rp, idx, val)
        st = ix.stats()
    o = np.lexsort((c, q))
    return (q[o], c[o], s[o]), st


def _both(monkeypatch, u, reference, theta, rp, idx, val, debug="", flags=0, ftile=FTILE, dim=None, tile=TILE):
    """the two-plane kernel of `u` steps and its no_planes twin against the reference; returns the two stats"""
    want, ref = reference
    out = []
    for twin in (False, True):
        pairs, st = _run(monkeypatch, ",".join(x for x in (debug, "no_planes" if twin else "planes") if x), dim or DIMS[u], theta, rp,
                         idx, val, flags, tile)
        print("%s | pairs %d (oracle %d) | visits %d (oracle %d) | candidates %d (oracle %d) | survivors %d | downgrades %d | chunk %d" % (
            st["probe_kernel"], len(pairs[0]), len(want), st["posting_visits"], ref["visits"], st["candidate_pairs"],
            ref["cand_pairs"], st["filter_survivors"], st["downgrades"], st["query_chunk"]))
        m = re.match(PLAIN if twin else PLANES, st["probe_kernel"])
        assert m and int(m.group(1)) == u, st["probe_kernel"]
        assert st["thin_launches"] > 0 and st["downgrades"] == 0 and st["filter_tile_rows"] == ftile
        got = to_map(*pairs)
        assert len(got) == len(pairs[0]), "a pair reported twice"
        assert_same_pairs(got, want, theta)
        assert st["posting_visits"] == ref["visits"]
        assert st["candidate_pairs"] == ref["cand_pairs"]
        out.append((pairs, st))
    for a, b in zip(out[0][0], out[1][0]):
        assert a.tobytes() == b.tobytes()
    assert out[0][1]["query_chunk"] == out[1][1]["query_chunk"]  # the same work list
    return out[0][1], out[1][1]


# ---- data: one set per window, each with its reference, computed once

def _block_rows(u, n=N, dim=None):
    """groups of seven stored neighbours A A B A B B B (A, B two unrelated rows): rounds v and v + 1 meet the same candidates
    (they share a plane only if a wipe was missed), rounds v and v + 2 meet them on the SAME plane with one wipe between"""
    rng = np.random.default_rng(8100 + u)
    rows = []
    while len(rows) < n:
        a, b = _row(rng, dim or DIMS[u]), _row(rng, dim or DIMS[u])
        rows += [a, a, b, a, b, b, b]
    return rows[:n]


def _rare_rows(u):
    """three filter tiles.  HEAVY's segment in the first is a long one (300 rows: more than 256 postings, swept by the whole
    workgroup); in the second tile every ninth row holds it, between two near-copies of itself that do not: ordinary, rare,
    ordinary on the same candidates.  Every third of a tile's first 600 rows (those triples apart) is a `wide` row, 12 or 24 of
    its terms among 40 popular ones whose segments run to six chunks: 24 of them make a round of more chunks than the strips
    hold (flagged at staging and swept straight from the index, whatever the window), 12 a round of about 260 -- more than the
    five-step window's 240 and less than the strips' 288 (chunks past the window, read from the strip)"""
    dim = DIMS[u]
    heavy, popular = dim - 1, (dim - 1 - N_POPULAR, dim - 1)
    rng = np.random.default_rng(8300 + u)
    rows = []
    for i in range(N):
        rows.append(_noisy(rng, rows[int(rng.integers(0, i))]) if i > 20 and rng.random() < 0.1 else _row(rng, popular[0]))

    def with_heavy(r):  # (in place of the row's last term: 100 terms stay 100)
        return np.append(r[0][:-1], heavy).astype(np.int32), r[1]

    for i in rng.choice(FTILE, 300, replace=False):
        rows[i] = with_heavy(rows[i])
    first = FTILE + 6
    near = set()
    for i in range(first, 2 * FTILE - 8, 9):
        rows[i - 1] = _noisy(rng, rows[i])
        rows[i + 1] = _noisy(rng, rows[i])
        rows[i] = with_heavy(rows[i])
        near.update((i - 1, i, i + 1))
    k = 0
    for i in range(3, N, 3):
        if i % FTILE < 600 and heavy not in rows[i][0] and i not in near:
            npop = 12 if k % 2 else 24
            k += 1
            t = np.concatenate([rng.choice(popular[0], size=NNZ - npop, replace=False), rng.choice(np.arange(*popular), size=npop, replace=False)])
            rows[i] = (np.sort(t).astype(np.int32), _unit(np.abs(rng.standard_normal(NNZ)) + 0.1))
    return rows


THETA = {"block": 0.7, "rare": 0.6, "short": 0.7, "big": 0.7}
BIG_TILE = 16384                           # tile_rows of the one case with full planes: filter tiles of 32,768 rows
BIG_DIMS = {5: 128000, 6: 108800}          # ... and the dimensions that put DIMS' postings into their segments
BIG_N = 2 * BIG_TILE + 777
_cache = {}


def _data(oracle, kind, u):
    """(rowptr, indices, values), reference -- shared by every test that uses the set, never changed"""
    if (kind, u) not in _cache:
        dim = DIMS[u]
        if kind == "short":  # the block rows with a last tile of 777 rows
            rows = _block_rows(u)[:2 * FTILE + 777]
        elif kind == "big":
            dim = BIG_DIMS[u]
            rows = _block_rows(u, BIG_N, dim)
        else:
            rows = _block_rows(u) if kind == "block" else _rare_rows(u)
        csr = _csr(rows)
        _cache[(kind, u)] = (csr, _reference(oracle, dim, THETA[kind], *csr))
    return _cache[(kind, u)]


# ---- 1. the same candidates in rounds v, v + 1 and v + 2

@pytest.mark.parametrize("u", [5, 6])
def test_same_candidates_in_neighbouring_rounds(oracle, monkeypatch, u):
    csr, ref = _data(oracle, "block", u)
    planes, _ = _both(monkeypatch, u, ref, THETA["block"], *csr)
    assert planes["result_pairs"] >= (N - 6) // 7 * 18  # (6 ordered pairs among the three copies of A, 12 among B's four)


# ---- 2. a rare round between ordinary ones, plain and as an item's last round

@pytest.mark.parametrize("u", [5, 6])
@pytest.mark.parametrize("debug", ["", "chunks=%d" % N, "chunks=%d" % (N // 2)])
def test_a_rare_round_between_ordinary_ones(oracle, monkeypatch, u, debug):
    """a rare round (a long segment swept by the workgroup, chunks past the register window, a round swept straight from the
    index) needs no clear of its own: its plane is wiped in the next round like any other.  With chunks of one round every rare
    round is its item's last, and the wipe behind the item's last barrier takes it; with chunks of two it is the last of every
    other item"""
    from apss import _lib
    csr, ref = _data(oracle, "rare", u)
    rp, idx, val = csr
    row = np.repeat(np.arange(rp.size - 1), NNZ)
    holders = row[idx == DIMS[u] - 1]
    assert (holders < FTILE).sum() > 256 and 100 < ((holders >= FTILE) & (holders < 2 * FTILE)).sum() <= 256
    planes, _ = _both(monkeypatch, u, ref, THETA["rare"], rp, idx, val, debug=debug, flags=_lib.FLAG_NO_SYMMETRY)
    if debug:
        assert planes["query_chunk"] == N // int(debug.split("=")[1])


@pytest.mark.parametrize("u", [5, 6])
def test_the_rare_set_takes_every_rare_path(oracle, monkeypatch, capfd, u):
    """what makes a round rare is decided by the window (U), the adding waves (A) and the strips (48 slots per adding wave) --
    the planner's choice, not the data's.  APSS_DEBUG=diag has plan_filter() say what it chose; with those figures the set's
    rounds are counted here as the staging waves count them (a segment of up to 256 postings: ceil(len / 16) chunks; a longer
    one: a long segment, no chunks).  A planner that chose otherwise turns the rare cases above into ordinary ones: this fails"""
    from apss import _lib
    (rp, idx, val), _ = _data(oracle, "rare", u)
    capfd.readouterr()
    _, st = _run(monkeypatch, "diag,planes", DIMS[u], THETA["rare"], rp, idx, val, _lib.FLAG_NO_SYMMETRY)
    said = re.findall(r"\[apss diag\] even\? merge 1 block 512 u \d+ \| F (\d+) G \d+ A (\d+) chunks [\d.]+ ue (\d+) fits 1", capfd.readouterr().err)
    assert said and re.match(PLANES, st["probe_kernel"]), st["probe_kernel"]
    stagers, adders, steps = (int(x) for x in said[-1])
    assert steps == u and stagers + adders == 8
    window, strips = adders * 8 * u, adders * 48
    tile_of = np.repeat(np.arange(N) // FTILE, NNZ)
    seg = np.zeros((3, DIMS[u]), np.int64)
    np.add.at(seg, (tile_of, idx), 1)
    chunks = np.where(seg > 256, 0, (seg + 15) // 16)
    tot = chunks[:, idx].reshape(3, N, NNZ).sum(axis=2)          # [tile, query]: chunks of the round
    longs = (seg > 256)[:, idx].reshape(3, N, NNZ).sum(axis=2)   # ... and its long segments
    past, swept, long_rounds = (tot > window) & (tot <= strips), tot > strips, (longs > 0) & (tot <= strips)
    print("U %d F %d A %d: %d rounds, %d past the window, %d swept from the index, %d with a long segment" % (
        u, stagers, adders, tot.size, past.sum(), swept.sum(), long_rounds.sum()))
    assert swept.sum() > 100 and long_rounds.sum() > 100
    assert past.sum() > (100 if window < strips else -1)  # (six steps x 8 = the strip's 48 slots: nothing lies between)
    ordinary = (tot <= window) & (longs == 0)
    assert ordinary.sum() > 0.8 * tot.size
    # ... and between ordinary ones: a rare round of either kind with an ordinary round before and behind it, in every tile it occurs in
    rare = ~ordinary
    assert (rare[:, 1:-1] & ordinary[:, :-2] & ordinary[:, 2:]).sum() > 100


# ---- 3. consecutive items in one workgroup, items of odd and of even length

@pytest.mark.parametrize("u", [5, 6])
@pytest.mark.parametrize("kind,debug,symmetric,q_chunk", [("block", "chunks=41,persist_fine=16,persist_wgs=1", True, 256),
                                                          ("block", "chunks=43,persist_wgs=1", False, 143),
                                                          ("block", "chunks=2048,persist_wgs=1", False, 3),
                                                          ("rare", "chunks=192,persist_fine=32,persist_wgs=1", False, 32),
                                                          ("rare", "chunks=43,persist_wgs=1", False, 143)])
def test_consecutive_items_in_one_workgroup(oracle, monkeypatch, u, kind, debug, symmetric, q_chunk):
    """one persistent workgroup takes every item: an item finds the planes as the last one left them -- both zero, whichever
    plane its last round used, and the wipe behind an item's last barrier takes plane 0 after an odd number of rounds, plane 1
    after an even one.  The symmetric join rounds its chunks up to a power of two (41 chunks asked: 256 rounds, cut fine at
    the end into pieces of 16): even items only.  Without symmetry 6,144 rows in 43 chunks are items of 143 rounds (the last:
    138) and, cut fine at the end, shorter ones; in 2,048 chunks items of 3; in 192 chunks items of 32, those that end with a
    rare round among them"""
    from apss import _lib
    csr, ref = _data(oracle, kind, u)
    planes, _ = _both(monkeypatch, u, ref, THETA[kind], *csr, debug=debug, flags=0 if symmetric else _lib.FLAG_NO_SYMMETRY)
    assert planes["query_chunk"] == q_chunk and (planes["symmetric"] != 0) == symmetric


# ---- 4. a short last tile, and tiles that are no multiple of a store

@pytest.mark.parametrize("u", [5, 6])
def test_a_last_tile_of_777_rows(oracle, monkeypatch, u):
    csr, ref = _data(oracle, "short", u)
    _both(monkeypatch, u, ref, THETA["short"], *csr)


@pytest.mark.parametrize("u", [5, 6])
def test_tiles_that_are_no_multiple_of_256_rows(oracle, monkeypatch, u):
    """a handle's filter tiles are all of one size, the last one merely holds fewer rows; cx_tile=2112 makes that size 8.25
    stores of 256 bytes: the wipe rounds up to nine, the ninth runs 192 bytes past the tile inside the plane's 32,768"""
    csr, ref = _data(oracle, "block", u)
    _both(monkeypatch, u, ref, THETA["block"], *csr, debug="cx_tile=2112", ftile=2112)


@pytest.mark.parametrize("u", [5, 6])
def test_full_planes_every_store_of_the_wipe(oracle, monkeypatch, u):
    """filter tiles of 32,768 rows (tile_rows = 16,384; two of them and a third of 777 rows): 128 stores per wipe, all sixteen of
    every wave and all four statements with their immediates up to 30,720 -- the small tiles above end inside the first
    statement's first store.  Near-copies lie all over the tile, so a quarter of a plane that is not wiped shows as false pairs
    and uncounted first touches among its rows"""
    csr, ref = _data(oracle, "big", u)
    planes, _ = _both(monkeypatch, u, ref, THETA["big"], *csr, ftile=2 * BIG_TILE, dim=BIG_DIMS[u], tile=BIG_TILE)
    assert planes["result_pairs"] >= (BIG_N - 6) // 7 * 18


# ---- 5. chunks of one, two and three rounds

@pytest.mark.parametrize("u", [5, 6])
@pytest.mark.parametrize("q_chunk", [1, 2, 3])
def test_chunks_of_one_two_and_three_rounds(oracle, monkeypatch, u, q_chunk):
    """the adding waves' loop is unrolled by two (the plane is a constant of each half) and leaves after an odd last round; the
    wipe behind the loop takes whichever plane the last round used"""
    from apss import _lib
    csr, ref = _data(oracle, "block", u)
    planes, _ = _both(monkeypatch, u, ref, THETA["block"], *csr, debug="chunks=%d" % (N // q_chunk), flags=_lib.FLAG_NO_SYMMETRY)
    assert planes["query_chunk"] == q_chunk and planes["symmetric"] == 0
