"""apss_query_stored on one MI355X against the parent's way to ask the same question: apss_query_dev of the same rows handed in as
a device batch (default store: C3, the metric's config -- 1M rows of 100 terms, theta 0.8).

    python profiles/query_stored.py [--workload c3] [--rows N] [--reps 20] [--warmup 3] [--out profiles/query_stored.jsonl]

For 1, 1024 and 16384 random stored ids: the median over `reps` calls (after `warmup`) of
  wall_ms     time.perf_counter around the call (it synchronises the handle's stream before it returns)
  event_ms    HIP events on the default stream around the call (the handle's own stream is a blocking stream: it orders itself
              with the default stream, so the two events bracket the handle's device work and the host's waits in between)
for query_stored (ids on the device) and for query_dev (the rows cut out of the batch on the device beforehand, untimed), and the
library's own device times of the stored query: select_ms (sort, k_qs_select, scans, k_qs_ids), gather_ms (k_qs_slots, k_qs_gather)
and the probe's (probe_ms + rescore_ms).  One JSON line per measurement; profiles/query_stored.md is written by hand from them."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "all-pairs-similarity_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3")
    ap.add_argument("--rows", type=int, default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from apss import synth
    from apss.engine import ApssIndex
    cfg = dict(synth.CONFIGS[a.workload])
    if a.rows:
        cfg["n"] = a.rows
    n, dim, theta = cfg["n"], cfg["dim"], cfg["theta"]
    dev = torch.device("cuda", 0)
    t0 = time.time()
    rp, idx, val = synth.make_vectors(n, dim, cfg["nnz"], cfg["zipf_s"], cfg["seed"])
    d_rp = torch.from_numpy(rp).to(dev)
    d_idx = torch.from_numpy(idx).to(dev)
    d_val = torch.from_numpy(val.astype(np.float32)).to(dev)
    d_ids = torch.arange(n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    out = open(a.out, "a") if a.out else None

    def emit(**kw):
        line = json.dumps(dict(workload=a.workload, n=n, dim=dim, theta=theta, **kw))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    emit(what="setup", gen_s=round(time.time() - t0, 1))
    rng = np.random.Generator(np.random.PCG64(5))
    ix = ApssIndex(dim, theta, capacity_rows=n, capacity_nnz=d_idx.numel())
    ix.insert_dev(d_ids, d_rp, d_idx, d_val)

    def timed(call):
        wall, event, extra = [], [], []
        for i in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t = time.perf_counter()
            x = call()
            w = (time.perf_counter() - t) * 1e3
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                wall.append(w)
                event.append(e0.elapsed_time(e1))
                extra.append(x)
        return float(np.median(wall)), float(np.median(event)), extra

    for count in (1, 1024, 16384):
        if count > n:
            continue
        rows = np.sort(rng.choice(n, size=count, replace=False)).astype(np.int64)
        ids = torch.from_numpy(rows).to(dev)
        # the same rows as a device batch (rows are the ids in this store), cut out beforehand
        lens = (d_rp[1:] - d_rp[:-1])[ids]
        b_rp = torch.zeros(count + 1, dtype=torch.int64, device=dev)
        b_rp[1:] = torch.cumsum(lens, 0)
        ent = torch.repeat_interleave(d_rp[:-1][ids] - b_rp[:-1], lens) + torch.arange(int(b_rp[-1]), device=dev)
        b_idx, b_val, b_ids = d_idx[ent].contiguous(), d_val[ent].contiguous(), d_ids[ids].contiguous()
        torch.cuda.synchronize()

        def stored():
            r = ix.query_stored(ids, fetch=False)
            qi, st = ix.stored_query_info(), ix.stats()
            return r, qi["select_ms"], qi["gather_ms"], st["probe_ms"] + st["rescore_ms"], st["probe_kernel"]

        def handed_in():
            r = ix.query_dev(b_ids, b_rp, b_idx, b_val)
            st = ix.stats()
            return r, st["probe_ms"] + st["rescore_ms"], st["probe_kernel"]

        w, e, x = timed(stored)
        assert all(v[0][0] == count for v in x)
        emit(what="query_stored", ids=count, wall_ms=w, event_ms=e, pairs=x[0][0][1], select_ms=float(np.median([v[1] for v in x])),
             gather_ms=float(np.median([v[2] for v in x])), probe_ms=float(np.median([v[3] for v in x])), probe_kernel=x[0][4])
        w2, e2, y = timed(handed_in)
        assert y[0][0] == x[0][0][1]
        emit(what="query_dev", ids=count, wall_ms=w2, event_ms=e2, pairs=y[0][0], probe_ms=float(np.median([v[1] for v in y])),
             probe_kernel=y[0][2])
    ix.close()


if __name__ == "__main__":
    main()
