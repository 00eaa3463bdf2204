"""Child process of test_gpu_persist.py: runs every scenario of that file once, with the persistent launch of the thin-round
filter (k_probe_even over a work list, csrc/apss_worklist.hpp) or with APSS_DEBUG=no_persist (one workgroup per (tile, chunk)
cell), and pickles what the library left: the sorted result pairs, the stats that do not measure time and the `[apss diag]`
lines of each scenario.

    python persist_child.py persist|grid OUT.pkl

APSS_DEBUG is read when a handle is created, so every scenario sets it first.  The inputs are built here from fixed seeds
(scenario_inputs), so that the test process restates them for its references."""
import os
import pickle
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "all-pairs-similarity_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

TIMING = ("probe_ms", "build_ms", "rescore_ms", "head_ms", "hbm_bytes")
THETA = 0.5
DIM_A, DIM_L, DIM_M = 8000, 16384, 60_000
HEAVY = DIM_A - 1   # the rare-round batch's term with more than 256 postings in the first tile
QUERY_ID0 = 100_000  # ids of an outside query batch


def _unit(w):
    w = np.asarray(w, np.float64)
    return w / np.linalg.norm(w)


def _csr(rows):
    rp = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(t) for t, _ in rows], out=rp[1:])
    idx = np.concatenate([np.asarray(t) for t, _ in rows]).astype(np.int32)
    val = np.concatenate([np.asarray(w, np.float64) for _, w in rows])
    return rp, idx, val


def _terms(rng, lo, hi, k):
    return np.sort(rng.choice(np.arange(lo, hi), size=k, replace=False)).astype(np.int32)


def _random_rows(rng, n, dim, k, dup):
    """rows of k terms; a fraction `dup` of them noisy copies of an earlier row (the pairs to report)"""
    rows = []
    for i in range(n):
        if i > 20 and rng.random() < dup:
            t, w = rows[int(rng.integers(0, i))]
            rows.append((t, _unit(w * (1.0 + 0.05 * rng.standard_normal(w.size)))))
        else:
            rows.append((_terms(rng, 0, dim, k), _unit(np.abs(rng.standard_normal(k)) + 0.1)))
    return rows


def scenario_inputs():
    """name -> (dim, rowptr, indices, values), from fixed seeds"""
    out = {}
    # 2,600 rows of 40 terms: at tile_rows = 256 five filter tiles of 512 rows and a sixth of 40
    out["many"] = (DIM_A,) + _csr(_random_rows(np.random.default_rng(921), 2600, DIM_A, 40, 0.1))
    out["few"] = (DIM_A,) + _csr(_random_rows(np.random.default_rng(922), 300, DIM_A, 40, 0.3))
    # rare rounds: two filter tiles of 512 rows; HEAVY is in 300 rows of the first tile (a long segment there: every round
    # that holds it is swept by the whole workgroup and ends with a whole-tile clear) and, in the second, in the LAST row of
    # every 64 -- the last round of a chunk of 64 and of any piece of it
    rng = np.random.default_rng(923)
    rows = _random_rows(rng, 1024, HEAVY, 8, 0.15)
    heavy = set(int(i) for i in rng.choice(512, 300, replace=False)) | set(range(575, 1024, 64))
    rows = [(np.append(t, HEAVY).astype(np.int32), _unit(np.append(w, 0.3))) if i in heavy else (t, w) for i, (t, w) in enumerate(rows)]
    out["rare"] = (DIM_A,) + _csr(rows)
    # stale strips: the last four rows of every 64 have 128 terms, the others one term out of 300: an item's last rounds fill
    # the strips, the next item's first rounds must not find them
    rng = np.random.default_rng(924)
    rows = []
    for i in range(2048):
        if i % 64 >= 60:
            if i > 200 and rng.random() < 0.3:
                t, w = rows[64 * int(rng.integers(0, i // 64)) + 60 + int(rng.integers(0, 4))]
                rows.append((t, _unit(w * (1.0 + 0.05 * rng.standard_normal(w.size)))))
            else:
                rows.append((_terms(rng, 0, DIM_L, 128), _unit(np.abs(rng.standard_normal(128)) + 0.1)))
        else:
            rows.append((_terms(rng, 0, 300, 1), np.ones(1)))
    out["stale"] = (DIM_L,) + _csr(rows)
    # term shards of 64-term rows, as tests/test_gpu_even_lean.py makes the library merge two rows per round
    from apss import synth
    n, nnz = 4096, 64
    rp, idx, val = synth.make_vectors(n, DIM_M, nnz, 0.0, seed=925, dup_frac=0.05)
    idx, val = idx.reshape(n, nnz).copy(), val.reshape(n, nnz).copy()
    rng = np.random.default_rng(926)
    for a in rng.choice(n - 1, size=n // 40, replace=False):
        idx[a + 1], val[a + 1] = idx[a], _unit(val[a] * rng.uniform(0.95, 1.05, size=nnz))
    out["shards"] = (DIM_M, rp, idx.reshape(-1), val.reshape(-1))
    return out


def head(rp, idx, val, m):
    """the first m rows as a batch of their own"""
    return rp[:m + 1], idx[:rp[m]], val[:rp[m]]


# (name, input, what runs, APSS_DEBUG of the scenario).  `join`: insert-and-query into an empty handle; `nosym`: the same on a handle
# with APSS_FLAG_NO_SYMMETRY; `outside`: the batch is stored, then its first 777 rows asked as an outside batch; `cache`: stored,
# then outside batches of 500 and of 777 rows on the same handle; `shards`: four term shards of one GPU
SCENARIOS = (
    # more items than workgroups: 126 cells of 64 rounds over six tiles, pieces of 16 rounds
    ("many_wgs1", "many", "join", "chunks=41,persist_fine=16,persist_wgs=1"),
    ("many_wgs3", "many", "join", "chunks=41,persist_fine=16,persist_wgs=3"),
    ("many_default", "many", "join", "chunks=41,persist_fine=16"),
    # the symmetric join's list, nothing cut: the diag line's item count has a closed form
    ("many_uncut", "many", "join", "chunks=41"),
    # fewer items than workgroups
    ("one_item", "few", "join", "chunks=1,persist_fine=512"),
    ("two_items", "few", "join", "chunks=2,persist_fine=512"),
    # not symmetric: chunks of 7 rounds (the last one of 3) in pieces of 1, of 2 (the last one of 1) and of 4 and 3
    ("nosym_fine1", "many", "nosym", "chunks=372,persist_fine=1,persist_wgs=5"),
    ("nosym_fine2", "many", "nosym", "chunks=372,persist_fine=2,persist_wgs=5"),
    ("nosym_fine4", "many", "nosym", "chunks=372,persist_fine=4"),
    ("outside_fine1", "many", "outside", "chunks=111,persist_fine=1,persist_wgs=2"),
    ("outside_fine2", "many", "outside", "chunks=111,persist_fine=2"),
    # rare rounds as the last round of an item, the next item on the other tile
    ("rare_wgs1", "rare", "nosym", "chunks=16,persist_wgs=1"),
    ("rare_fine32", "rare", "nosym", "chunks=16,persist_fine=32,persist_wgs=1"),
    ("rare_default", "rare", "nosym", "chunks=16,persist_fine=32"),
    # long rounds at the end of an item, short ones at the start of the next
    ("stale_wgs1", "stale", "join", "chunks=32,persist_wgs=1"),
    ("stale_fine16", "stale", "join", "chunks=32,persist_fine=16,persist_wgs=2"),
    # merged rounds of a term shard, diagonal (own_tile) items among merged ones in one workgroup; the shard rule unmerged
    ("shards_merged_wgs1", "shards", "shards", "chunks=16,persist_fine=32,persist_wgs=1"),
    ("shards_merged", "shards", "shards", "chunks=16,persist_fine=32"),
    ("shards_unmerged", "shards", "shards", "merge=0,chunks=16,persist_fine=32,persist_wgs=3"),
    # the candidate list overflows and the probe runs again: the work counter starts from zero
    ("regrow", "many", "join", "chunks=41,persist_fine=16,persist_wgs=3,res_cap=64"),
    # two batch sizes on one handle: the cached list is rebuilt
    ("cache", "many", "cache", "chunks=50,persist_fine=4,persist_wgs=2"),
)


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
    base = "diag" + ("" if mode == "persist" else ",no_persist")
    diag = Diag(out_path + ".stderr")
    import torch
    from apss import _lib, engine
    from apss.dist import HipShardEngine, join_shards_local, term_ranges
    _lib.lib()
    inputs = scenario_inputs()
    res = {}

    def pairs(qcs):
        q, c, s = (np.asarray(x) for x in qcs[:3])
        o = np.lexsort((c, q))
        return q[o], c[o], s[o]

    def stats(st):
        return {k: v for k, v in st.items() if k not in TIMING}

    for name, key, kind, debug in SCENARIOS:
        os.environ["APSS_DEBUG"] = base + "," + debug
        dim, rp, idx, val = inputs[key]
        n = rp.size - 1
        ids = np.arange(n, dtype=np.int64)
        tile_rows = 1024 if key in ("stale", "shards") else 256
        diag.lines()
        if kind in ("join", "nosym"):
            with engine.ApssIndex(dim, THETA, head_terms=-1, tile_rows=tile_rows, flags=_lib.FLAG_NO_SYMMETRY if kind == "nosym" else 0) as ix:
                p = pairs(ix.insert_and_query(ids, rp, idx, val))
                res[name] = dict(pairs=p, stats=stats(ix.stats()), diag=diag.lines())
        elif kind in ("outside", "cache"):
            with engine.ApssIndex(dim, THETA, head_terms=-1, tile_rows=tile_rows) as ix:
                ix.insert(ids, rp, idx, val)
                calls = []
                for m in ((777,) if kind == "outside" else (500, 777)):
                    p = pairs(ix.query(np.arange(m, dtype=np.int64) + QUERY_ID0, *head(rp, idx, val, m)))
                    calls.append(dict(pairs=p, stats=stats(ix.stats()), diag=diag.lines()))
                res[name] = calls[0] if kind == "outside" else dict(calls=calls)
        else:
            ranges = term_ranges(np.bincount(idx, minlength=dim), 4)
            engines = [HipShardEngine(dim, 0.7, tr, torch.device("cuda", 0), tile_rows=tile_rows) for tr in ranges]
            for e in engines:
                e.load(rp, idx, val)
            p = pairs(join_shards_local(engines, n, 0.7))
            res[name] = dict(pairs=p, stats=[stats(e.stats) for e in engines], diag=diag.lines())
            del engines

    with open(out_path, "wb") as f:
        pickle.dump(res, f)


if __name__ == "__main__":
    main()
