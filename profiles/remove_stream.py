"""Removal on one MI355X: what marking, dropping and compacting cost on a workload's store (default: C3, the metric's config).

    python profiles/remove_stream.py [--workload c3] [--rows N] [--reps 3] [--out profiles/remove_runs.jsonl]

One JSON line per measurement (device times are the library's own HIP events, apss_removal_info / apss_stats):
  mark      apss_remove_dev of 1, 1024 and 100k ids drawn from the stored ones: mark_ms (sort of the list + k_rm_mark)
  drop      a self-join with 10 % of the rows marked: drop_ms (k_rm_drop) beside probe_ms + rescore_ms, pairs before / after
  compact   apss_compact of that store: compact_ms, wall, against the only alternative a caller has without it --
            apss_clear + apss_insert_dev of the live rows (gathered on the device with torch beforehand, not timed)
profiles/remove.md is written by hand from these lines."""
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
    ap.add_argument("--reps", type=int, default=3)
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
    rng = np.random.Generator(np.random.PCG64(3))
    ix = ApssIndex(dim, theta, capacity_rows=n, capacity_nnz=d_idx.numel())
    ix.insert_dev(d_ids, d_rp, d_idx, d_val)
    base = ix.self_join(fetch=False)
    st = ix.stats()
    emit(what="self_join_nothing_marked", pairs=base, probe_ms=st["probe_ms"], rescore_ms=st["rescore_ms"],
         drop_launches=ix.removal_info()["drop_launches"])

    # ---- mark: every repetition on a fresh store, ids drawn from the stored ones
    for count in (1, 1024, 100000):
        if count > n:
            continue
        ms = []
        for _ in range(a.reps):
            ix.clear()
            ix.insert_dev(d_ids, d_rp, d_idx, d_val)
            ids = torch.from_numpy(rng.choice(n, size=count, replace=False).astype(np.int64)).to(dev)
            assert ix.remove(ids) == count
            ms.append(ix.removal_info()["mark_ms"])
        emit(what="mark", ids=count, mark_ms=ms)

    # ---- drop: 10 % of the rows marked
    ix.clear()
    ix.insert_dev(d_ids, d_rp, d_idx, d_val)
    gone = torch.from_numpy(np.sort(rng.choice(n, size=n // 10, replace=False)).astype(np.int64)).to(dev)
    assert ix.remove(gone) == n // 10
    for _ in range(a.reps):
        kept = ix.self_join(fetch=False)
        st, ri = ix.stats(), ix.removal_info()
        emit(what="drop", marked=n // 10, pairs_before=kept + ri["pairs_dropped"], pairs_after=kept, pairs_nothing_marked=base,
             drop_ms=ri["drop_ms"], probe_ms=st["probe_ms"], rescore_ms=st["rescore_ms"], drop_launches=ri["drop_launches"])

    # ---- compact against clear + insert_dev of the live rows
    live = torch.ones(n, dtype=torch.bool, device=dev)
    live[gone] = False
    rows = live.nonzero().flatten()
    lens = (d_rp[1:] - d_rp[:-1])[rows]
    l_rp = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=dev)
    l_rp[1:] = torch.cumsum(lens, 0)
    ent = torch.repeat_interleave(d_rp[:-1][rows] - l_rp[:-1], lens) + torch.arange(int(l_rp[-1]), device=dev)
    l_idx, l_val, l_ids = d_idx[ent].contiguous(), d_val[ent].contiguous(), d_ids[rows].contiguous()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        ix.clear()
        ix.insert_dev(d_ids, d_rp, d_idx, d_val)
        assert ix.remove(gone) == n // 10
        t0 = time.perf_counter()
        ix.compact()
        wall = (time.perf_counter() - t0) * 1e3
        ri, st = ix.removal_info(), ix.stats()
        assert ix.size()[0] == rows.numel()
        emit(what="compact", compact_ms=ri["compact_ms"], wall_ms=wall, build_ms=st["build_ms"], live_rows=int(rows.numel()),
             hbm_bytes=st["hbm_bytes"])
        t0 = time.perf_counter()
        ix.clear()
        ix.insert_dev(l_ids, l_rp, l_idx, l_val)
        wall = (time.perf_counter() - t0) * 1e3
        emit(what="clear_and_insert_live", wall_ms=wall, build_ms=ix.stats()["build_ms"], hbm_bytes=ix.stats()["hbm_bytes"])
    after = ix.self_join(fetch=False)
    emit(what="self_join_after_compaction", pairs=after, probe_ms=ix.stats()["probe_ms"])
    ix.close()


if __name__ == "__main__":
    main()
