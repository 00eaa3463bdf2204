"""The ragged shape of the removal edge tests (tests/test_gpu_remove_edges.py) and its oracle lists, computed once per process.

S = 1501 stored rows (odd) and Q = 333 query rows in dim 4096.  Row i has LENGTHS[i % 8] = 0, 1, 2, 63, 64, 65, 129 or 200
terms: an empty row, rows at both sides of k_rm_gather's 64-lane stride, rows of three and four trips.  From row 64 on a
non-empty row is, with probability 1/2, a copy of an earlier row of its own length class with 5 % multiplicative noise on the
weights (U(0.95, 1.05)); otherwise fresh: terms uniform (or Zipf(1.0)) without replacement, weights |N(0, 1)| + 0.1.  Every row
has unit norm.  The dead set D = rows 0 .. 69, every third row below S, and row S - 1 (the last one): 547 rows.

External ids follow a table, never the row number: row r carries -(r + 1), r, 2^40 + r or 2^62 + r for r % 4 = 0, 1, 2, 3,
and rows 1 and 2 carry INT64_MIN and INT64_MAX (include/apss.h puts no limit on an external id).  Expectations are the oracle's
row-number lists translated through the table.

An expectation is always the oracle's list for the whole history with every pair that touches a dead row deleted in numpy
(remove_shape.split).  The floors every test stands on, asserted on the oracle side before any device call: an empty band
(no visible pair within LOWER of theta) and, per non-empty length class of the CANDIDATE row, at least 15 kept and 15 dropped
pairs (class_floors)."""
import functools

import numpy as np

from remove_shape import LOWER, split  # noqa: F401  (split: the one way an expectation is made)

S, Q, DIM = 1501, 333, 4096
N = S + Q
THETA = 0.5
SEED = 5
LENGTHS = (0, 1, 2, 63, 64, 65, 129, 200)
CLASSES = tuple(n for n in LENGTHS if n)
FLOOR = 15
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max

LEN = np.array([LENGTHS[i % 8] for i in range(N)], dtype=np.int64)
D = np.unique(np.concatenate([np.arange(70), np.arange(0, S, 3), [S - 1]])).astype(np.int64)
IS_D = np.zeros(N, bool)
IS_D[D] = True
assert D.size == 547 and S % 2 == 1 and IS_D[S - 1]


def _ids():
    r = np.arange(N, dtype=np.int64)
    ids = np.select([r % 4 == 0, r % 4 == 1, r % 4 == 2], [-(r + 1), r, (1 << 40) + r], (1 << 62) + r).astype(np.int64)
    ids[1], ids[2] = I64_MIN, I64_MAX
    assert np.unique(ids).size == N
    return ids


IDS = _ids()
ROW_OF = {int(v): i for i, v in enumerate(IDS)}


@functools.lru_cache(maxsize=None)
def vectors(zipf=0.0, signed=False):
    """CSR (rowptr, indices, values float64) of the N unit rows.  signed: every fifth non-empty row carries its entries on the
    terms divisible by 7 negated (about a seventh of a row's mass: a copy and its source still score well above theta)"""
    rng = np.random.default_rng(SEED)
    p = None
    if zipf > 0:
        p = 1.0 / np.arange(1, DIM + 1, dtype=np.float64) ** zipf
        p = (p / p.sum())[np.argsort(rng.permutation(DIM))]
    terms, weights = [], []
    for i in range(N):
        n = int(LEN[i])
        if n == 0:
            t, w = np.zeros(0, np.int32), np.zeros(0)
        elif i >= 64 and rng.random() < 0.5:
            src = i - 8 * int(rng.integers(1, i // 8 + 1))
            t, w = terms[src], weights[src] * rng.uniform(0.95, 1.05, n)
        else:
            t = np.sort(rng.choice(DIM, n, replace=False, p=p)).astype(np.int32)
            w = np.abs(rng.standard_normal(n)) + 0.1
        terms.append(t)
        weights.append(w / np.sqrt((w * w).sum()) if n else w)
    if signed:
        for k, i in enumerate(np.nonzero(LEN)[0]):
            if k % 5 == 0:
                weights[i] = np.where(terms[i] % 7 == 0, -weights[i], weights[i])
    rp = np.concatenate([[0], np.cumsum(LEN)]).astype(np.int64)
    return rp, np.concatenate(terms).astype(np.int32), np.concatenate(weights).astype(np.float64)


def rows_of(v, a, b):
    rp, idx, val = v
    return rp[a:b + 1] - rp[a], idx[rp[a]:rp[b]], val[rp[a]:rp[b]]


def pick(v, rows):
    """the CSR of the given rows of v, in that order"""
    rp, idx, val = v
    rows = np.asarray(rows, np.int64)
    out = np.concatenate([[0], np.cumsum(rp[rows + 1] - rp[rows])]).astype(np.int64)
    sel = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
    return out, idx[sel], val[sel]


def join_of(oracle, v, theta=THETA, q_begin=0):
    """(q, c, score) of every pair >= theta - LOWER with q >= q_begin, by row number, sorted by (q, c)"""
    rp, idx, val = v
    return oracle.selfjoin_pairs(DIM, theta - LOWER, rp, idx, val, q_begin, rp.size - 1)


@functools.lru_cache(maxsize=None)
def whole_join(oracle, zipf=0.0, signed=False, q_begin=0):
    return join_of(oracle, vectors(zipf, signed), THETA, q_begin)


def class_floors(orc, visible, live, theta=THETA, lengths=LEN):
    """asserts the module's floors on the pairs `visible` of the oracle's list: nothing within LOWER of theta, and per
    non-empty length class of the candidate row at least FLOOR kept and FLOOR dropped pairs.  Returns {class: (kept, dropped)}"""
    oq, oc, os_ = orc
    assert int((visible & (np.abs(os_ - theta) <= LOWER)).sum()) == 0, "a pair inside the band: change the seed"
    over = visible & (os_ >= theta)
    out = {}
    for n in CLASSES:
        of_class = over & (lengths[oc] == n)
        out[n] = (int((of_class & live).sum()), int((of_class & ~live).sum()))
        assert min(out[n]) >= FLOOR, (n, out[n])
    return out


def by_id(want, ids=IDS):
    """a {(q row, c row): score} map translated through the id table"""
    return {(int(ids[a]), int(ids[b])): s for (a, b), s in want.items()}


def batch_expectation(oracle, zipf=0.0, signed=False, frozen=False, dead=IS_D):
    """the S rows stored, `dead` marked, then the Q rows as a query-insert (or as a frozen query: the batch does not see
    itself).  Returns (the oracle's triples, split(...)) with the floors asserted"""
    orc = whole_join(oracle, zipf, signed, S)
    visible = orc[1] < S if frozen else np.ones(orc[0].size, bool)
    live = ~dead[orc[1]]
    class_floors(orc, visible, live)
    return orc, split(orc, THETA, visible, live)


def self_expectation(oracle, zipf=0.0, signed=False, dead=IS_D, rows=S):
    """self-join of the first `rows` rows with `dead` marked: a pair goes when either end is dead"""
    orc = whole_join(oracle, zipf, signed)
    visible = (orc[0] < rows) & (orc[1] < rows)
    live = ~dead[orc[0]] & ~dead[orc[1]]
    class_floors(orc, visible, live)
    return orc, split(orc, THETA, visible, live)
