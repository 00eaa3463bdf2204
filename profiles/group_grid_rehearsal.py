"""Rehearsal of the T x D grids of apss_group on ONE GPU: BASELINE.json configs[3] (C3) through ApssGroup
with all eight members on device 0, for the grids 8x1, 4x2, 2x4, 1x8 in one session.  A step is what `bench.py --engine group
--share-device` times: apss_group_clear + apss_group_insert_and_query_dev on a batch resident in HBM.  The 8x1 row is the
layout apss_group_create offers (T x 1).  With every member on one device a step's time is roughly the SUM of the cells' work:
this ranks the layouts' total device work, it is not a scaling figure.

    python profiles/group_grid_rehearsal.py [--config c3] [--steps 7] [--warmup 2] [--grids 8x1,4x2,2x4,1x8] [--out FILE]

Writes profiles/group_grid_rehearsal.json (per grid: median step ms of the timed steps, own / outside phase and exchange wall
times, device posting visits, result count) and asserts that every grid reports the same number of pairs."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "all-pairs-similarity_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--grids", default="8x1,4x2,2x4,1x8")
    ap.add_argument("--head-terms", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_grid_rehearsal.json"))
    a = ap.parse_args()
    import torch
    from apss import synth
    from apss.engine import ApssGroup
    cfg, rp, idx, val = synth.make_config(a.config)
    n = cfg["n"]
    dev = torch.device("cuda", 0)
    d0 = (torch.arange(n, dtype=torch.int64, device=dev), torch.from_numpy(rp).to(dev), torch.from_numpy(idx).to(dev),
          torch.from_numpy(val.astype(np.float32)).to(dev))
    torch.cuda.synchronize()
    rows = []
    for spec in a.grids.split(","):
        T, D = (int(x) for x in spec.split("x"))
        with ApssGroup(cfg["dim"], cfg["theta"], [0] * (T * D), head_terms=a.head_terms, row_ranges=D) as g:
            per_member = [d0] * (T * D)

            def step():
                g.clear()
                return g.insert_and_query_dev(per_member)

            for _ in range(max(1, a.warmup)):  # (the first call decides the layout)
                step()
            ms, per, grids = [], [], []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                n_pairs = step()  # (returns when every member has finished: nothing is in flight)
                ms.append((time.perf_counter() - t0) * 1e3)
                per.append(g.stats())
                grids.append(g.grid())
            med = lambda xs: float(np.median(xs))  # noqa: E731
            st, gr = per[-1], grids[-1]
            rows.append({
                "grid": "%dx%d" % (T, D), "term_ranges": T, "row_ranges": D, "step_ms": med(ms), "step_ms_all": [round(x, 3) for x in ms],
                "own_ms_max": med([x["own_ms_max"] for x in grids]), "outside_ms_max": med([x["outside_ms_max"] for x in grids]),
                "exchange_ms": med([x["exchange_ms"] for x in per]), "member_ms_max": med([x["member_ms_max"] for x in per]),
                "build_ms_max": med([x["build_ms_max"] for x in per]), "probe_ms_max": med([x["probe_ms_max"] for x in per]),
                "posting_visits": st["posting_visits"], "device_posting_visits": st["device_posting_visits"],
                "candidates_sum": st["candidates_sum"], "union_pairs": st["union_pairs"], "result_pairs": int(n_pairs),
                "head_terms": st["head_terms"], "symmetric_ranges": gr["symmetric_ranges"], "mirrored_pairs": gr["mirrored_pairs"],
                "outside_rows_max": gr["outside_rows_max"], "rows_in_range": gr["rows_in_range"], "term_cuts": st["term_cuts"]})
            print(json.dumps(rows[-1]), flush=True)
    counts = {r["result_pairs"] for r in rows}
    assert len(counts) == 1, "the grids disagree on the number of pairs: %s" % {r["grid"]: r["result_pairs"] for r in rows}
    out = {"what": "apss_group grids, every member on GPU 0 (rehearsal: a step is roughly the sum of the cells' work, not a scaling figure)",
           "config": a.config, "n": n, "dim": cfg["dim"], "theta": cfg["theta"], "steps": a.steps, "warmup": a.warmup,
           "step": "apss_group_clear + apss_group_insert_and_query_dev, batch resident in HBM; step_ms = median of the timed steps",
           "device": torch.cuda.get_device_name(0), "grids": rows}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
