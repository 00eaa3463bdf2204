"""Inputs shared by the tests of the index build (test_gpu_build_runs.py, test_gpu_index_contents.py)."""
import numpy as np

from apss import synth


def corner_vectors(dim, seed, n_base=1400, nnz=20, range_terms=16384):
    """uniform rows with 5 % duplicates + the corners of the cut computation, each twice (a pair to report): rows whose
    entries all lie in the first / in the last term range, rows of 1 entry and of 2,247, a row with entries in the first and the
    last range only (every range between: empty runs), empty rows; shuffled, unit norm"""
    rng = np.random.default_rng(seed)
    rp, idx, val = synth.make_vectors(n_base, dim, nnz, 0.0, seed=seed, dup_frac=0.05)
    rows = [(idx[rp[i]:rp[i + 1]].astype(np.int32), val[rp[i]:rp[i + 1]].astype(np.float64)) for i in range(n_base)]
    last_lo = (dim - 1) // range_terms * range_terms
    first_hi = min(range_terms, dim)

    def row(terms):
        t = np.unique(np.asarray(terms, np.int64)).astype(np.int32)
        v = np.abs(rng.standard_normal(t.size)) + 0.1
        return t, v / np.sqrt((v * v).sum())

    special = [
        row(rng.choice(first_hi, size=min(30, first_hi), replace=False)),              # all in the first range
        row(last_lo + rng.choice(dim - last_lo, size=min(30, dim - last_lo), replace=False)),  # all in the last (short) range
        row([int(rng.integers(0, dim))]),                                              # one entry
        row([dim - 1]),                                                                # ... the very last term
        row([0]),                                                                      # ... the very first
        row(rng.choice(dim, size=min(2247, dim), replace=False)),                      # far longer than a lane group
        row(np.concatenate([rng.choice(first_hi, 5, replace=False), [dim - 1, dim - 2]])),  # first + last range only
    ]
    empty = (np.zeros(0, np.int32), np.zeros(0))
    rows += special + special + [empty] * 7
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    rp = np.concatenate([[0], np.cumsum([r[0].size for r in rows])]).astype(np.int64)
    return rp, np.concatenate([r[0] for r in rows]).astype(np.int32), np.concatenate([r[1] for r in rows])


def _rows_of(rp, idx, val):
    return [(np.asarray(idx[rp[i]:rp[i + 1]], np.int32), np.asarray(val[rp[i]:rp[i + 1]], np.float64)) for i in range(len(rp) - 1)]


def _csr_of(rows):
    rp = np.concatenate([[0], np.cumsum([r[0].size for r in rows])]).astype(np.int64)
    return rp, np.concatenate([r[0] for r in rows]).astype(np.int32), np.concatenate([r[1] for r in rows]).astype(np.float64)


def plant_term(rows, term, holders, rel_weight=0.15):
    """`rows` (list of (terms, values), changed in place) with `term` held by exactly the rows `holders` (a set of row numbers)
    among those it is asked about: taken out of every other row, put into the holders at rel_weight times the row's largest
    weight, holders renormalised to unit norm"""
    for r, (t, v) in enumerate(rows):
        has = t.size and (t == term).any()
        if r in holders and not has:
            k = int(np.searchsorted(t, term))
            w = rel_weight * float(np.abs(v).max()) if v.size else 1.0
            t, v = np.insert(t, k, term).astype(np.int32), np.insert(v, k, w)
            rows[r] = (t, v / np.sqrt((v * v).sum()))
        elif r not in holders and has:
            keep = t != term
            rows[r] = (t[keep], v[keep])


def index_inputs(dim, seed, cb, align, range_terms=16384, counts=None, n_fill=704):
    """the corner vectors + n_fill short uniform rows (1,421 + 704 = 2,125 rows: no multiple of a tile, so the tiles are cut
    inside the data and the last one is partial) in which ONE common term (dim // 2 + 3) is held by a chosen number of each
    tile's rows: tile after tile align - 1, align, align + 1 and 300 (more than the 256 postings the probe sweeps as a long
    segment; a tile of fewer rows: all of them), then over again -- the lengths around the aligned unit and the long segment,
    by construction.  counts: {tile: rows} overrides.  Returns (rowptr, indices, values, common term)."""
    from apss import synth
    rp, idx, val = corner_vectors(dim, seed, range_terms=range_terms)
    rows = _rows_of(rp, idx, val)
    frp, fidx, fval = synth.make_vectors(n_fill, dim, 8, 0.0, seed=seed + 1, dup_frac=0.0)
    rows += _rows_of(frp, fidx, fval)
    n = len(rows)
    common = dim // 2 + 3
    pattern = (align - 1, align, align + 1, 300)
    holders = set()
    for tile in range(-(-n // cb)):
        want = (counts or {}).get(tile, pattern[tile % 4])
        nonempty = [r for r in range(tile * cb, min(n, (tile + 1) * cb)) if rows[r][0].size]
        holders.update(nonempty[:want])
    plant_term(rows, common, holders)
    return _csr_of(rows) + (common,)


def two_long_segments(n, dim, nnz, seed, terms=(5, 9)):
    """n uniform rows (5 % duplicates) that ALL hold the given common terms, at a small weight: (tile, term) segments of as many
    postings as the tile has rows, next to each other in one sub-range of the run-reading build"""
    from apss import synth
    rp, idx, val = synth.make_vectors(n, dim, nnz, 0.0, seed=seed, dup_frac=0.05)
    keep = ~np.isin(idx, terms)
    row = np.repeat(np.arange(n), np.diff(rp))[keep]
    idx, val = idx[keep], val[keep].astype(np.float64)
    k = len(terms)
    t2 = np.concatenate([idx, np.tile(np.asarray(terms, idx.dtype), n)])
    v2 = np.concatenate([val, np.full(n * k, 0.05)])
    r2 = np.concatenate([row, np.repeat(np.arange(n), k)])
    o = np.lexsort((t2, r2))
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(r2, minlength=n))]).astype(np.int64)
    return rp2, t2[o].astype(np.int32), v2[o]
