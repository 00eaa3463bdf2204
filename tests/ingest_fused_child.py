"""Child process of test_gpu_ingest_fused.py: runs every scenario of that file once, with the one-pass ingest of plain batches
(k_ingest_plain) or with APSS_DEBUG=no_fused_ingest (k_ingest_count + k_ingest_write, k_row_cuts, k_df_sample), and pickles
what the library left: the store read back, the sorted result pairs, the stats that do not measure time, the `[apss diag]`
lines of each scenario, and the error of every rejected batch.

    python ingest_fused_child.py fused|unfused OUT.pkl

The inputs are built here from fixed seeds (scenario_inputs), so that the test process restates them for its references."""
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "all-pairs-similarity_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

DIM = 40_000  # three ranges of 16,384 terms, the last one 7,232 terms wide
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 64, 65, 100)
EDGE_TERMS = (0, 16383, 16384, 32767, 32768, DIM - 1)
RUNS = "build_lds,build_runs,build_trace"
TIMING = ("probe_ms", "build_ms", "rescore_ms", "head_ms", "hbm_bytes")
BAD_KINDS = ("not_increasing", "term_eq_dim", "term_minus_one", "nan", "inf", "rowptr_decreasing", "rowptr_end_past_nnz",
             "rowptr_first_not_zero")


def _unit_f32(v):
    """unit norm, then rounded to fp32: the device's narrowing of the doubles is exact"""
    return (v / np.sqrt((v * v).sum())).astype(np.float32).astype(np.float64)


def _rows_to_csr(rows):
    rp = np.concatenate([[0], np.cumsum([r[0].size for r in rows])]).astype(np.int64)
    idx = np.concatenate([r[0] for r in rows] + [np.zeros(0, np.int32)]).astype(np.int32)
    val = np.concatenate([r[1] for r in rows] + [np.zeros(0)]).astype(np.float64)
    return rp, idx, val


def shape_rows(seed, per_length=14):
    """rows of every length of LENGTHS, each row twice (a pair to report), with the terms at the range edges planted in some
    of them; a row inside one range, a row with an entry in every range; shuffled"""
    rng = np.random.default_rng(seed)
    rows = []

    def row(terms):
        t = np.unique(np.asarray(terms, np.int64)).astype(np.int32)
        v = rng.uniform(0.1, 1.0, t.size)
        return (t, _unit_f32(v) if t.size else np.zeros(0))

    for n in LENGTHS:
        for i in range(per_length):
            terms = rng.choice(DIM, n, replace=False) if n else np.zeros(0, np.int64)
            if n and i % 3 == 0:  # plant edge terms (as many as fit), keeping the length
                k = min(n, len(EDGE_TERMS))
                terms = np.concatenate([rng.choice(EDGE_TERMS, k, replace=False), terms])
                terms = np.unique(terms)
                while terms.size > n:
                    drop = [j for j in range(terms.size) if int(terms[j]) not in EDGE_TERMS]
                    terms = np.delete(terms, drop[0] if drop else 0)
                while terms.size < n:
                    terms = np.unique(np.concatenate([terms, rng.choice(DIM, 1)]))
            rows.append(row(terms))
    rows.append(row(16384 + rng.choice(16384, 40, replace=False)))              # entirely inside the middle range
    rows.append(row(np.array(EDGE_TERMS)))                                      # an entry at every edge: every range
    rows.append(row(np.concatenate([rng.choice(16384, 3, replace=False), 32768 + rng.choice(DIM - 32768, 3, replace=False)])))  # first + last range only
    rows = rows + rows
    order = rng.permutation(len(rows))
    return [rows[i] for i in order]


def scenario_inputs():
    """name -> CSR (rowptr, indices, values) of every scenario, from fixed seeds"""
    from apss import synth
    out = {}
    out["shapes"] = _rows_to_csr(shape_rows(11))
    out["runs"] = _rows_to_csr(shape_rows(12, per_length=60))  # ~1,300 rows: six tiles of 256
    rp, idx, val = synth.make_vectors(300, DIM, 24, 0.0, seed=13, dup_frac=0.1)
    out["valid"] = (rp, idx, val.astype(np.float32).astype(np.float64))
    _, zi, zv = synth.make_vectors_zipf_dev(3000, DIM, 50, 1.0, 14, "cpu", dup_frac=0.1)
    zi, zv = zi.numpy().astype(np.int32), zv.numpy().astype(np.float32).astype(np.float64)
    out["zipf"] = (np.arange(3001, dtype=np.int64) * 50, zi.reshape(-1), zv.reshape(-1))
    return out


def bad_batch(kind, rp, idx, val, row=7):
    """the valid batch with one defect in `row` (or in its rowptr): (rowptr, indices, values float32)"""
    rp, idx, val = rp.copy(), idx.copy(), val.astype(np.float32)
    b, e = int(rp[row]), int(rp[row + 1])
    assert e - b >= 3
    if kind == "not_increasing":
        idx[b + 2] = idx[b + 1]
    elif kind == "term_eq_dim":
        idx[e - 1] = DIM
    elif kind == "term_minus_one":
        idx[b] = -1
    elif kind == "nan":
        val[b + 1] = np.nan
    elif kind == "inf":
        val[b + 1] = np.inf
    elif kind == "rowptr_decreasing":
        rp[row + 1] = rp[row] - 1
    elif kind == "rowptr_end_past_nnz":
        rp[-1] += 5
    elif kind == "rowptr_first_not_zero":
        rp[0] = 1
    else:
        raise ValueError(kind)
    return rp, idx, val


class Diag:
    """the process's stderr goes to a file; lines() returns the `[apss` lines written since the last call"""

    def __init__(self, path):
        self.f = open(path, "w+b")
        os.dup2(self.f.fileno(), 2)
        self.pos = 0

    def lines(self):
        self.f.seek(self.pos)
        data = self.f.read()
        self.pos += len(data)
        return [ln for ln in data.decode(errors="replace").splitlines() if ln.startswith("[apss")]


def main():
    mode, out_path = sys.argv[1], sys.argv[2]
    base = "diag" + ("" if mode == "fused" else ",no_fused_ingest")
    diag = Diag(out_path + ".stderr")
    import torch
    from apss import _lib, engine
    from store_view import read_store
    _lib.lib()
    inputs = scenario_inputs()
    res = {}

    def debug(extra=""):
        os.environ["APSS_DEBUG"] = base + ("," + extra if extra else "")

    def pairs(qcs):
        q, c, s = qcs
        o = np.lexsort((c, q))
        return q[o], c[o], s[o]

    def stats(ix):
        return {k: v for k, v in ix.stats().items() if k not in TIMING}

    def store(ix):
        st = read_store(ix)
        return (st.rowptr, st.indices, st.values, st.ext_ids)

    def dev(rp, idx, val, ids):
        t = lambda a, dt: torch.tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")  # noqa: E731
        return t(ids, torch.int64), t(rp, torch.int64), t(idx, torch.int32), t(val, torch.float32)

    # 1. row shapes: one batch, the handle's own choices
    rp, idx, val = inputs["shapes"]
    n = rp.size - 1
    debug()
    diag.lines()
    with engine.ApssIndex(DIM, 0.5) as ix:
        p = pairs(ix.insert_and_query(np.arange(n) + 500, rp, idx, val))
        res["shapes"] = dict(pairs=p, stats=stats(ix), store=store(ix), diag=diag.lines())

    # 2. run-form build forced: one batch; two batches, the second starting inside a tile
    rp, idx, val = inputs["runs"]
    n = rp.size - 1
    debug(RUNS)
    with engine.ApssIndex(DIM, 0.5, tile_rows=256) as ix:
        p = pairs(ix.insert_and_query(np.arange(n), rp, idx, val))
        res["runs_one"] = dict(pairs=p, stats=stats(ix), store=store(ix), diag=diag.lines())
    m = 2 * 256 + 188
    with engine.ApssIndex(DIM, 0.5, tile_rows=256) as ix:
        got = []
        for b0, b1 in ((0, m), (m, n)):
            sl = slice(rp[b0], rp[b1])
            got.append(pairs(ix.insert_and_query(np.arange(b0, b1), rp[b0:b1 + 1] - rp[b0], idx[sl], val[sl])))
        whole = pairs(ix.self_join())
        res["runs_two"] = dict(batches=got, pairs=whole, stats=stats(ix), store=store(ix), diag=diag.lines())

    # 3. rejected batches: the defect sits in a row the df sample takes (stride 1: every row) of a handle whose head policy is
    # live and whose build reads runs; then a valid batch; and a handle that only ever saw the valid batch
    rp, idx, val = inputs["valid"]
    n = rp.size - 1
    ids = np.arange(n) + 9000
    debug(RUNS)
    for kind in BAD_KINDS + ("clean",):
        with engine.ApssIndex(DIM, 0.5, tile_rows=256, head_terms=64) as ix:
            err = None
            if kind != "clean":
                brp, bidx, bval = bad_batch(kind, rp, idx, val)
                try:
                    ix.insert_dev(*dev(brp, bidx, bval, ids))
                except engine.ApssError as e:
                    err = (e.code, str(e))
                size_after = ix.size()
            else:
                size_after = (0, 0)
            p = pairs(ix.insert_and_query(ids, rp, idx, val))
            res["bad_" + kind] = dict(err=err, size_after=size_after, pairs=p, stats=stats(ix), store=store(ix), head=np.array(ix.head_terms()),
                                      diag=diag.lines())

    # 4. head policy on a Zipf(1) batch: the df sample decides the block's terms
    rp, idx, val = inputs["zipf"]
    n = rp.size - 1
    debug()
    with engine.ApssIndex(DIM, 0.6, head_terms=64) as ix:
        p = pairs(ix.insert_and_query(np.arange(n), rp, idx, val))
        res["zipf"] = dict(pairs=p, stats=stats(ix), head=np.array(ix.head_terms()), diag=diag.lines())

    # 5. other paths: a negative weight after a block was chosen; a query-only batch; handles whose ingest transforms
    half = n // 2
    sl0, sl1 = slice(rp[0], rp[half]), slice(rp[half], rp[n])
    neg = val[sl1].copy()
    neg[5] = -neg[5]
    with engine.ApssIndex(DIM, 0.6, head_terms=64) as ix:
        ix.insert(np.arange(half), rp[:half + 1], idx[sl0], val[sl0])
        before = stats(ix)
        p = pairs(ix.insert_and_query(np.arange(half, n), rp[half:] - rp[half], idx[sl1], neg))
        res["negative"] = dict(pairs=p, before=before, stats=stats(ix), diag=diag.lines())
    rp, idx, val = inputs["shapes"]
    n = rp.size - 1
    with engine.ApssIndex(DIM, 0.5) as ix:
        ix.insert(np.arange(n), rp, idx, val)
        p = pairs(ix.query(np.arange(200) + n, rp[:201], idx[:rp[200]], val[:rp[200]]))
        res["query_only"] = dict(pairs=p, stats=stats(ix), size=ix.size(), diag=diag.lines())
    # ... a good query, then a defective and far larger query-only batch (its staging outgrows the buffers the first one's
    # results point into), then the result calls, then the good query again
    zrp, zidx, zval = inputs["zipf"]
    with engine.ApssIndex(DIM, 0.5) as ix:
        ix.insert(np.arange(n), rp, idx, val)
        good = (np.arange(200) + n, rp[:201], idx[:rp[200]], val[:rp[200]])
        first = pairs(ix.query(*good))
        brp, bidx, bval = bad_batch("not_increasing", zrp, zidx, zval)
        err = after = None
        try:
            ix.query_dev(*dev(brp, bidx, bval, np.arange(zrp.size - 1) + 70000))
        except engine.ApssError as e:
            err = (e.code, str(e))
        try:
            after = ("pairs", pairs(ix.fetch()))
        except engine.ApssError as e:
            after = ("error", e.code)
        again = pairs(ix.query(*good))
        res["query_rejected"] = dict(first=first, err=err, after=after, again=again, size=ix.size(), diag=diag.lines())
    # ... the run-reading build by the library's own decision (nothing forced): 24 coarse tiles of 128 rows x 3 ranges, 50 entries per row
    debug("build_trace")
    with engine.ApssIndex(DIM, 0.6, tile_rows=64, head_terms=-1) as ix:
        p = pairs(ix.insert_and_query(np.arange(zrp.size - 1), zrp, zidx, zval))
        res["default_runs"] = dict(pairs=p, stats=stats(ix), diag=diag.lines())
    debug()
    with engine.ApssIndex(DIM, 0.5, flags=_lib.FLAG_NORMALIZE) as ix:
        p = pairs(ix.insert_and_query(np.arange(n), rp, idx, val))
        res["normalize"] = dict(pairs=p, diag=diag.lines())
    with engine.ApssIndex(DIM, 0.5, term_range=(10_000, 30_000)) as ix:
        ix.insert(np.arange(n), rp, idx, val)
        res["shard"] = dict(size=ix.size(), diag=diag.lines())

    with open(out_path, "wb") as f:
        pickle.dump(res, f)


if __name__ == "__main__":
    main()
