"""The global top-K (apss_set_top_pairs) timed on one GPU: select_ms (HIP events) and the call's wall time, beside the
per-query pass on the same list (apss_topk_info.select_ms at top_k = 8) and what a caller did before: fetch() the whole list and
np.lexsort it on the host.  One JSON line per (shape, K) on stdout; profiles/top_pairs.md quotes them.
  python profiles/top_pairs.py [a] [z] [c3]     shape A | the 2.7 M-pair theta = 0 list | a C3 slice of 200k rows"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "all-pairs-similarity_amd")):
    sys.path.insert(0, p)
from apss import synth  # noqa: E402
from apss.engine import ApssIndex  # noqa: E402



def med(xs):
    return float(np.median(xs))


def run(name, dim, theta, rp, idx, val, Ks, tile_rows=0, reps=7):
    n = len(rp) - 1
    ids = np.arange(n, dtype=np.int64)
    with ApssIndex(dim, theta, tile_rows=tile_rows) as ix:
        ix.insert(ids, rp, idx, val)
        for _ in range(2):
            pairs = ix.self_join(fetch=False)
        wall0 = []
        for _ in range(reps):
            t = time.perf_counter()
            ix.self_join(fetch=False)
            wall0.append((time.perf_counter() - t) * 1e3)
        # what a caller does today: fetch the whole list, sort it on the host, cut
        host = []
        for _ in range(3):
            t = time.perf_counter()
            q, c, s = ix.fetch()
            order = np.lexsort((c, q, -s.astype(np.float64)))[:max(Ks)]
            host.append((time.perf_counter() - t) * 1e3)
        # the per-query pass on the same list
        ix.set_top_k(8)
        pq = []
        for _ in range(reps + 2):
            ix.self_join(fetch=False)
            pq.append(ix.topk_info()["select_ms"])
        ix.set_top_k(0)
        for K in Ks:
            ix.set_top_pairs(K)
            sel, wall, launches = [], [], 0
            for r in range(reps + 2):
                t = time.perf_counter()
                ix.self_join(fetch=False)
                w = (time.perf_counter() - t) * 1e3
                info = ix.top_pairs_info()
                if r >= 2:
                    sel.append(info["select_ms"])
                    wall.append(w)
                launches = info["launches"]
            t = time.perf_counter()
            ix.fetch()
            fetch_k = (time.perf_counter() - t) * 1e3
            rec = dict(shape=name, pairs=pairs, K=K, select_ms=med(sel), select_ms_min=min(sel), call_wall_ms=med(wall), call_wall_ms_K0=med(wall0),
                       stage_wall_ms=med(wall) - med(wall0), fetch_K_ms=fetch_k, launches=launches, above=info["above"], tied=info["tied"],
                       per_query_top8_select_ms=med(pq[2:]), fetch_and_lexsort_ms=med(host))
            print(json.dumps(rec), flush=True)
        ix.set_top_pairs(0)


which = sys.argv[1:] or ["a", "z", "c3"]
if "a" in which:
    rp, idx, val = synth.make_vectors(1500, 300, 12, 1.0, seed=21, dup_frac=0.1)
    run("shape A (1500 rows, theta 0.45)", 300, 0.45, rp, idx, val, [1000], tile_rows=512)
if "z" in which:
    rp, idx, val = synth.make_vectors(2000, 64, 8, 0.0, seed=5, dup_frac=0.1)
    run("theta 0 (2000 rows, dim 64)", 64, 0.0, rp, idx, val, [10, 100000])
if "c3" in which:
    c = synth.CONFIGS["c3"]
    rp, idx, val = synth.make_vectors(200000, c["dim"], c["nnz"], c["zipf_s"], c["seed"])
    run("C3 slice (200k rows, theta 0.8)", c["dim"], c["theta"], rp, idx, val, [1000], reps=3)
