"""The one shape of the removal tests (tests/test_gpu_remove.py) and its oracle lists, computed once per process.

3000 unit rows of 30 terms in dim 2000, ids = row numbers, tile_rows = 512: the first 2000 rows fill four tiles.  The removed set
R = rows 0 .. 511 (a wholly dead tile), every 7th row from 512 below 2000, and row 1999: 726 rows.  An expectation is always the
oracle's list for the whole history with every pair that touches a removed row deleted in numpy."""
import functools

import numpy as np

from apss import synth

N, DIM, NNZ, TILE = 3000, 2000, 30, 512
STORED = 2000           # rows inserted before the removal
LOWER = 2e-5            # the oracle runs this much below the device's threshold, so that it knows the pairs just below it
IDS = np.arange(N, dtype=np.int64)
R = np.unique(np.concatenate([np.arange(0, 512), np.arange(512, STORED, 7), [1999]])).astype(np.int64)
IS_R = np.zeros(N, bool)
IS_R[R] = True
assert R.size == 726


@functools.lru_cache(maxsize=None)
def vectors(zipf=0.0):
    return synth.make_vectors(N, DIM, NNZ, zipf, seed=8, dup_frac=0.1)


def rows_of(v, a, b):
    rp, idx, val = v
    return rp[a:b + 1] - rp[a], idx[rp[a]:rp[b]], val[rp[a]:rp[b]]


@functools.lru_cache(maxsize=None)
def whole_join(oracle, theta, zipf=0.0, q_begin=0):
    """(q, c, score) of every pair >= theta - LOWER with q >= q_begin, by row number, sorted by (q, c)"""
    rp, idx, val = vectors(zipf)
    return oracle.selfjoin_pairs(DIM, theta - LOWER, rp, idx, val, q_begin, N)


def split(orc, theta, visible, live):
    """visible / live: masks over orc's pairs -- what the call can see at all, and which of those touch no removed row.
    Returns (the live triples incl. the band below theta, map of the live pairs >= theta, removed pairs >= theta, removed
    pairs inside |score - theta| <= LOWER)"""
    oq, oc, os_ = orc
    over = os_ >= theta
    keep, gone = visible & live, visible & ~live
    want = {(int(a), int(b)): float(s) for a, b, s in zip(oq[keep & over], oc[keep & over], os_[keep & over])}
    dropped = int((gone & over).sum())
    band = int((gone & (np.abs(os_ - theta) <= LOWER)).sum())
    return (oq[keep], oc[keep], os_[keep]), want, dropped, band
