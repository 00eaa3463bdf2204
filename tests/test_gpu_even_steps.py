"""k_probe_even deals a round's chunks in whole window steps (csrc/apss_even.hpp): chunk j goes to step j div 8A, and inside
the step to adding wave (j mod 8A) div 8, lane group j mod 8; an adding wave works out from the round's total alone how many
chunks and steps are its own, and skips the steps behind its last chunk.  A mistake there loses or doubles whole chunks for
particular totals only -- around a multiple of 8 (the last wave of a step), of 8A (the last step) and of 8AU (the window).

The batches are built so that the total of every round of interest is known on the host: two filter tiles of 2,048 rows; the
first holds 2,048 filler rows, the second the DESIGN rows, each followed by a row whose terms the first tile does not hold.
A term of a design row has 16 m postings in the first tile (m chunks), or one posting, or none, and one posting in the second
tile (the row's own).  A design row meets the first tile in a round of its own (two rows per round: with the row behind it,
which adds no chunks), so that round's total is the sum of its terms' chunks.  Every row has one more term at or above D0, in
segments of 16 postings: the second term range of the sharded cases.

The totals are computed here from the batch itself (document frequencies per tile) and checked against the cases above for
the A and U of the launch -- U from `probe_kernel`, A from the staging waves that plan_filter's diagnostic line states --
before any result is looked at.  Then: pairs and scores against the oracle, posting visits and candidate pairs exact (merged
rounds too: the union of a round's rows per tile, computed here), the thin-round kernel ran, and the query chunks had the
size the case asks for (`query_chunk`)."""
import re

import numpy as np
import pytest

from helpers import assert_same_pairs, to_map

pytestmark = pytest.mark.gpu

FTR = 2048            # rows of a filter tile at tile_rows = 1024
D0, DIM = 65536, 131072
THETA = 0.6
DEBUG = "flat_group=0"  # one staging lane per term: a staging wave takes 64 terms of the round's row


def _adding_waves(longest_row):
    """adding waves of a 512-thread launch whose longest staged row has that many terms, one staging lane per term"""
    return 8 - max(1, -(-longest_row // 64))


def _cases(A, U):
    """round totals that a launch with A adding waves and windows of U steps has to meet"""
    return {0, 1, 7, 8, 9, 8 * A - 1, 8 * A, 8 * A + 1, 8 * A * U - 1, 8 * A * U + 1}


def _parts(total, kmax, rng):
    """`total` chunks as at most kmax terms of 1 .. 16 chunks each: mostly one to three, now and then more (a staging lane
    writes a term's first three chunks without a loop)"""
    parts, left = [], total
    while left > 0:
        room = kmax - len(parts)
        m = int(rng.integers(4, 17)) if rng.random() < 0.02 else int(rng.integers(1, 4))
        m = min(16, left, max(-(-left // room), m))
        parts.append(m)
        left -= m
    assert len(parts) <= kmax and sum(parts) == total
    return parts


def _design(kmax, waves, single_totals, seed):
    """kmax: design terms per row at the most; waves: {adding waves: window steps} to have every case for.  single_totals:
    totals also built from terms of ONE posting in the first tile (rows of that many terms).  Returns the batch and, per design row, (row, total)."""
    rng = np.random.default_rng(seed)
    wanted = set()
    for A, steps in waves.items():
        for U in steps:
            wanted |= {t for t in _cases(A, U) if t <= 16 * kmax}
    next_term = [0]

    def new_terms(k):
        t = np.arange(next_term[0], next_term[0] + k, dtype=np.int32)
        next_term[0] += k
        return t

    need = []      # (term, postings in the first tile)
    second = []    # rows of the second tile: term arrays
    design = []    # (row, total)

    def add_design_row(terms, total):
        if terms.size < 8:
            terms = np.concatenate([terms, new_terms(8 - terms.size)])  # (terms the first tile does not hold)
        design.append((FTR + len(second), total))
        second.append(terms)
        second.append(new_terms(8))

    for total in sorted(wanted):
        parts = _parts(total, kmax, rng)
        terms = new_terms(len(parts))
        need += [(int(t), 16 * m) for t, m in zip(terms, parts)]
        add_design_row(terms, total)
    for total in single_totals:
        terms = new_terms(total)
        need += [(int(t), 1) for t in terms]
        add_design_row(terms, total)
    # the first tile: the postings dealt out to its rows in turn (a term's rows are distinct: no term needs more than FTR)
    first = [[] for _ in range(FTR)]
    at = 0
    for t, k in need:
        for i in range(k):
            first[(at + i) % FTR].append(t)
        at += k
    assert max(len(r) for r in first) < 64
    rows = []
    for i, r in enumerate(first):
        rows.append(np.array(sorted(r) + [D0 + i // 16], np.int32))
    for j, t in enumerate(second):
        rows.append(np.concatenate([np.sort(t), [D0 + FTR // 16 + j]]).astype(np.int32))
    assert next_term[0] <= D0
    rp = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([r.size for r in rows], out=rp[1:])
    idx = np.concatenate(rows)
    val = np.concatenate([w / np.linalg.norm(w) for w in (np.abs(rng.standard_normal(r.size)) + 0.1 for r in rows)])
    return rp, idx, val, design


def _tile_totals(rp, idx, lo, hi, tile):
    """per row: the chunks of its terms in [lo, hi) among the postings of that tile's rows; also checks the design: every
    document frequency inside the tile is a multiple of 16, or 1"""
    n = len(rp) - 1
    row = np.repeat(np.arange(n), np.diff(rp))
    keep = (idx >= lo) & (idx < hi)
    in_tile = keep & (row // FTR == tile)
    df = np.bincount(idx[in_tile], minlength=DIM)
    assert np.all((df % 16 == 0) | (df == 1)), "a design term's document frequency is neither a multiple of 16 nor 1"
    return np.bincount(row[keep], weights=-(-df[idx[keep]] // 16), minlength=n).astype(np.int64)


def _check_cases(rp, idx, lo, hi, kernel, rows_per_round):
    """the rounds of the second tile's rows against the first tile: their totals cover the cases for this launch's A and U"""
    n = len(rp) - 1
    U = int(re.match(r"k_probe_even(?:_merged<|<512, )(\d+)", kernel).group(1))
    keep = (idx >= lo) & (idx < hi)
    longest = int(np.bincount(np.repeat(np.arange(n), np.diff(rp))[keep], minlength=n).max())
    A = _adding_waves(min(longest * rows_per_round, int(keep.sum())))
    tot = _tile_totals(rp, idx, lo, hi, 0)
    _tile_totals(rp, idx, lo, hi, 1)
    second = tot[FTR:]
    if second.size % rows_per_round:
        second = np.concatenate([second, np.zeros(rows_per_round - second.size % rows_per_round, np.int64)])
    rounds = set(int(t) for t in second.reshape(-1, rows_per_round).sum(axis=1))
    print("kernel %s: A = %d, U = %d, %d rows per round, round totals %s" % (kernel, A, U, rows_per_round, sorted(rounds)))
    missing = _cases(A, U) - rounds
    assert not missing, "no round of %s chunks for A = %d, U = %d" % (sorted(missing), A, U)
    return A, U


@pytest.fixture(scope="module")
def batches(oracle):
    """'short': rows of at most 64 terms (one staging wave, A = 7); 'long': rows of up to 128 terms (two staging waves, A = 6).
    With each: the oracle's pairs and its counts for the whole batch and for the two term ranges"""
    out = {}
    # (two rows of 'short' in one round are a row of up to 128 terms: A = 6 there)
    for name, kmax, waves, singles, seed in (("short", 63, {7: (2, 3, 4), 6: (3, 4, 5)}, (9, 47, 48, 49, 55), 901),
                                             ("long", 120, {6: (2, 3, 4)}, (9, 47, 48, 49, 95, 96, 97, 127), 902)):
        rp, idx, val, design = _design(kmax, waves, singles, seed)
        n = len(rp) - 1
        assert n <= 4096
        want = to_map(*oracle.selfjoin_pairs(DIM, THETA, rp, idx, val))
        assert len(want) > 1000
        refs = {(lo, hi): oracle.selfjoin_sample(1, DIM, THETA, *_restrict(rp, idx, val, lo, hi), 0, n, 2)
                for lo, hi in ((0, DIM), (0, D0), (D0, DIM))}
        out[name] = (rp, idx, val, want, refs)
    return out


def _restrict(rp, idx, val, lo, hi):
    """the batch with only its terms in [lo, hi): what one term shard indexes"""
    keep = (idx >= lo) & (idx < hi)
    row = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    rp2 = np.zeros(len(rp), np.int64)
    np.cumsum(np.bincount(row[keep], minlength=len(rp) - 1), out=rp2[1:])
    return rp2, idx[keep], None if val is None else val[keep]


def _chunks(n, q_chunk, sym=True):
    """APSS_DEBUG for query chunks of q_chunk rows: `chunks=N` asks for N chunks and the library takes ceil(n / N) rows each; a
    symmetric join rounds that up to a power of two, so any other size runs without the symmetry"""
    want = -(-n // q_chunk)
    assert -(-n // want) == q_chunk
    return ",chunks=%d" % want + ("" if sym and q_chunk & (q_chunk - 1) == 0 else ",no_sym")


def _staging_waves(err, rows_per_round):
    """the staging waves F of the launch as plan_filter's diagnostic line states them (APSS_DEBUG=diag, on stderr): the line
    of the number of rows per round that was taken"""
    f = set(int(m.group(2)) for m in re.finditer(r"\[apss diag\] even\? merge (\d+) .*\| F (\d+) G", err)
            if int(m.group(1)) == rows_per_round)
    assert len(f) == 1, err
    return f.pop()


def _merged_candidates(rp, idx, lo, hi, rows_per_round, q_chunk, symmetric):
    """first touches of a launch with M rows per round and query chunks of q_chunk rows, less a row's touch of its own slot.
    A workgroup (query chunk, candidate tile) whose tile holds rows of the chunk runs the chunk's rows one per round: per row,
    the tile's rows sharing a term with it.  Any other counts, per round, the candidates that ANY of the round's rows
    touches.  A symmetric join runs the tiles up to the chunk's own and counts those below it twice"""
    import scipy.sparse as sp
    n, M = len(rp) - 1, rows_per_round
    rp2, idx2, _ = _restrict(rp, idx, None, lo, hi)
    X = sp.csr_matrix((np.ones(idx2.size), idx2, rp2), shape=(n, DIM))
    rounds = sp.csr_matrix((np.ones(n), (np.arange(n) // M, np.arange(n))), shape=(-(-n // M), n)) @ X
    n_tiles = -(-n // FTR)
    total = -int((np.diff(rp2) > 0).sum())
    for t in range(n_tiles):
        Xt = X[t * FTR:min((t + 1) * FTR, n)].T.tocsr()
        per_row = np.diff(((X @ Xt) > 0).tocsr().indptr)      # candidates of every row in tile t
        per_round = np.diff(((rounds @ Xt) > 0).tocsr().indptr)  # ... of every round
        for r0 in range(0, n, q_chunk):
            r1 = min(r0 + q_chunk, n)
            own_lo, own_hi = r0 // FTR, (r1 - 1) // FTR
            if symmetric and t > own_lo:
                continue
            if own_lo <= t <= own_hi:
                total += int(per_row[r0:r1].sum())
            else:
                assert r0 % M == 0
                total += (2 if symmetric else 1) * int(per_round[r0 // M:-(-r1 // M)].sum())
    return total


@pytest.mark.parametrize("q_chunk", [0, 1, 2, 3])
@pytest.mark.parametrize("name,A", [("short", 7), ("long", 6)])
def test_plain_handle(batches, monkeypatch, capfd, name, A, q_chunk):
    """one handle over all terms; query chunks as the library cuts them, and chunks of one, two and three queries: the adding
    waves' loop is unrolled by two and leaves after an odd last round (three: without the symmetry, which wants a power of
    two; neither batch's rows are a multiple of three, so the last chunk is short)"""
    from apss.engine import ApssIndex
    rp, idx, val, want, refs = batches[name]
    n = len(rp) - 1
    assert n % 3
    monkeypatch.setenv("APSS_DEBUG", DEBUG + ",diag" + (_chunks(n, q_chunk) if q_chunk else ""))
    with ApssIndex(DIM, THETA, head_terms=-1, tile_rows=FTR // 2) as ix:
        q, c, s = ix.insert_and_query(np.arange(n, dtype=np.int64), rp, idx, val)
        st = ix.stats()
    assert st["probe_kernel"].startswith("k_probe_even<512, ") and st["thin_launches"] > 0, st["probe_kernel"]
    assert st["filter_tile_rows"] == FTR and st["tiles"] == 2 and st["queries_per_round"] == 1
    if q_chunk:
        assert st["query_chunk"] == q_chunk and st["symmetric"] == (q_chunk != 3)
    assert _check_cases(rp, idx, 0, DIM, st["probe_kernel"], 1)[0] == A == 8 - _staging_waves(capfd.readouterr().err, 1)
    got = to_map(q, c, s)
    assert len(got) == len(q), "a pair reported twice"
    assert_same_pairs(got, want, THETA)
    assert st["posting_visits"] == refs[(0, DIM)]["visits"]
    assert st["candidate_pairs"] == refs[(0, DIM)]["cand_pairs"]


@pytest.mark.parametrize("name,merged,A,q_chunk", [("short", False, 7, 4), ("long", False, 6, 4), ("short", True, 6, 2),
                                                   ("short", True, 6, 4), ("short", True, 6, 6)])
def test_two_term_shards(batches, monkeypatch, capfd, name, merged, A, q_chunk):
    """the term ranges [0, D0) and [D0, DIM) as two shards (shard rule: every window step may be skipped); on the short rows also
    with two rows per round, which the first range's launch has to report, in chunks of one, two and three rounds (three:
    without the symmetry)"""
    import torch
    from apss.dist import HipShardEngine, join_shards_local
    rp, idx, val, want, refs = batches[name]
    n = len(rp) - 1
    ranges = ((0, D0), (D0, DIM))
    engines = []
    for tr, diag in zip(ranges, (",diag", "")):  # (APSS_DEBUG is read when a handle is created: the first range's plan is printed)
        monkeypatch.setenv("APSS_DEBUG", DEBUG + diag + _chunks(n, q_chunk) + ("" if merged else ",merge=0"))
        engines.append(HipShardEngine(DIM, THETA, tr, torch.device("cuda", 0), tile_rows=FTR // 2))
    for e in engines:
        e.load(rp, idx, val)
    q, c, s, _ = join_shards_local(engines, n, THETA)
    st = engines[0].stats
    assert st["probe_kernel"].startswith("k_probe_even") and st["thin_launches"] > 0, st["probe_kernel"]
    assert st["filter_tile_rows"] == FTR and st["tiles"] == 2
    assert st["query_chunk"] == q_chunk and st["symmetric"] == (q_chunk != 6)
    assert (st["queries_per_round"] == 2 and "merged" in st["probe_kernel"]) if merged else st["queries_per_round"] == 1, st["probe_kernel"]
    M = st["queries_per_round"]
    assert _check_cases(rp, idx, 0, D0, st["probe_kernel"], M)[0] == A == 8 - _staging_waves(capfd.readouterr().err, M)
    got = to_map(q, c, s)
    assert len(got) == len(q), "a pair reported twice"
    assert_same_pairs(got, want, THETA)
    for e, tr in zip(engines, ranges):
        assert e.stats["posting_visits"] == refs[tr]["visits"], tr
        if e.stats["queries_per_round"] == 1:
            assert e.stats["candidate_pairs"] == refs[tr]["cand_pairs"], tr
        else:  # (two rows share their accumulators: a round's first touches are the candidates either row touches)
            assert e.stats["candidate_pairs"] == _merged_candidates(rp, idx, *tr, e.stats["queries_per_round"], q_chunk, e.stats["symmetric"] == 1), tr
