"""Per-query top-k (apss_set_top_k): device time of the pass beside the join it follows, per call.

Shapes: the reference's server template at similarityThreshold = 0 (N = 60,000, dim 1024, nnz 40: profiles/r04_theta0.json) and
BASELINE config 2's shape at theta = 0.5, both with k = 10.  Each shape: one handle, a warm-up self-join per setting (sizes the
buffers), then `--reps` self-joins alternating k = 0 and k = 10.  Times are HIP events inside the library (apss_stats.probe_ms /
rescore_ms, apss_topk_info.select_ms).  Beside them the floors the pass cannot beat: one read of the list (12 B x
pairs_over_theta) at the 6.29 TB/s copy peak, and the bytes this design moves --
  count    4 B per pair (query row)
  scatter  12 B read + 8 B written per pair
  select   a segment of <= 1024 pairs: 8 B read + an 8-B external id gathered per pair; a longer one: 4 B per pair and digit pass
           (four score digits at most, fewer when a digit already separates the k-th pair from the next) + 4 B for the collect
  output   12 B per kept pair
-- computed from the shapes (every segment taken as long when the mean segment is above 1024, four digit passes: an upper
estimate for data without ties at the cut).
Usage: python profiles/topk_select.py [--reps 3] [--shape template|c2|all] > profiles/topk_select.json

--window-pairs P [P ...] (apss_set_top_k_window, DESIGN.md 5e "Windows") measures the windowed call instead: on each chosen shape,
k = --k, `--reps` self-joins alternating the unwindowed setting (0) and every P, each setting on a handle of its own (a handle's
reservations only grow: `hbm_bytes` of a shared one would be the unwindowed list's) after one warm-up call.  Per call: wall time
of the call (it returns after the stream is synchronised), probe_ms, rescore_ms, select_ms, plan_ms, windows, the planning
figures and hbm_bytes.  `--shape c3zero` is C3's store (N = 1M, dim 100k, nnz 100) at theta = 0: the unwindowed setting is left
out there (its list does not fit the device) and one call per P is made, without a warm-up.
  python profiles/topk_select.py --shape template --window-pairs 67108864 268435456 > profiles/topk_window_template.json
  python profiles/topk_select.py --shape c3zero --window-pairs 1073741824 > profiles/topk_window_c3zero.json

--tile-cut (apss_set_top_k_tile_cut, DESIGN.md 5e "Cut inside the probe") measures the cut inside the theta <= 0 probe kernel: on
each chosen shape, k = --k, one handle with the setting off and one with it on (a handle's reservations only grow), a warm-up
self-join each, then `--reps` self-joins alternating the two.  Per call: probe_ms, select_ms, their sum, pairs_emitted,
pairs_over_theta, hbm_bytes, the probe's instantiation and why the cut did not apply (C2's shape at theta = 0.5: the declined
path, which must not move).  A library without the setting (an older commit the script is pointed at) is measured with the off
handle alone.  profiles/topk_tile_cut.md says what to run beside it.
  python profiles/topk_select.py --tile-cut --reps 5 > profiles/topk_tile_cut.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "all-pairs-similarity_amd"))
from apss import synth  # noqa: E402
from apss.engine import ApssIndex  # noqa: E402

COPY_PEAK = 6.29e12  # B/s, plain device copy on the MI355X
SHAPES = {"template": ("template_dim1024_theta0", 60_000, 1024, 40, 0.0, 0.0), "c2": ("c2_shape_theta0.5", 30_000, 10_000, 50, 1.0, 0.5)}


def design_bytes(pairs, kept, nq, passes=4):
    mean = pairs / max(nq, 1)
    select = pairs * (4 * (passes + 1)) if mean > 1024 else pairs * 16
    return pairs * 4 + pairs * 20 + select + kept * 12


C3_ZERO = ("c3_store_theta0", 1_000_000, 100_000, 100, 0.0, 0.0)


def windowed_call(ix):
    t0 = time.perf_counter()
    ix.self_join(fetch=False)
    wall = (time.perf_counter() - t0) * 1e3
    st, ti, tw = ix.stats(), ix.topk_info(), ix.topk_window_info()
    call = {"wall_ms": wall, "probe_ms": st["probe_ms"], "rescore_ms": st["rescore_ms"], "select_ms": ti["select_ms"],
            "hbm_bytes": st["hbm_bytes"], "pairs_over_theta": ti["pairs_over_theta"], "kept": ti["kept"]}
    call.update({k: v for k, v in tw.items() if k != "struct_size"})
    return call


def windows_main(a):
    out = {}
    shapes = dict(SHAPES, c3zero=C3_ZERO)
    for key, (name, n, dim, nnz, zipf, theta) in shapes.items():
        if a.shape != key and not (a.shape == "all" and key != "c3zero"):
            continue
        once = key == "c3zero"
        rp, idx, val = synth.make_vectors(n, dim, nnz, zipf, seed=11)
        row = {"n": n, "dim": dim, "nnz": nnz, "zipf_s": zipf, "theta": theta, "k": a.k, "calls": []}
        settings = list(a.window_pairs) if once else [0] + list(a.window_pairs)
        handles = []
        try:
            for pairs in settings:
                ix = ApssIndex(dim, theta, top_k=a.k, top_k_window=pairs)
                handles.append(ix)
                ix.insert(np.arange(n), rp, idx, val)
                if not once:
                    ix.self_join(fetch=False)  # warm-up: sizes this setting's buffers
            for rep in range(1 if once else a.reps):
                for pairs, ix in zip(settings, handles):
                    row["calls"].append(windowed_call(ix))
        finally:
            for ix in handles:
                ix.close()
        out[name] = row
    print(json.dumps(out, indent=1))


def tile_cut_main(a):
    have = hasattr(ApssIndex, "set_top_k_tile_cut")
    out = {"library_has_tile_cut": have}
    for key, (name, n, dim, nnz, zipf, theta) in SHAPES.items():
        if a.shape not in ("all", key):
            continue
        rp, idx, val = synth.make_vectors(n, dim, nnz, zipf, seed=11)
        row = {"n": n, "dim": dim, "nnz": nnz, "zipf_s": zipf, "theta": theta, "k": a.k, "calls": []}
        handles = []
        try:
            for on in ([False, True] if have else [False]):
                ix = ApssIndex(dim, theta, top_k=a.k)
                handles.append((on, ix))
                if on:
                    ix.set_top_k_tile_cut(True)
                ix.insert(np.arange(n), rp, idx, val)
                ix.self_join(fetch=False)  # warm-up: sizes this setting's buffers
            for rep in range(a.reps):
                for on, ix in handles:
                    ix.self_join(fetch=False)
                    st, ti = ix.stats(), ix.topk_info()
                    call = {"tile_cut": on, "probe_ms": st["probe_ms"], "select_ms": ti["select_ms"],
                            "probe_plus_select_ms": st["probe_ms"] + ti["select_ms"], "rescore_ms": st["rescore_ms"],
                            "pairs_over_theta": ti["pairs_over_theta"], "kept": ti["kept"], "hbm_bytes": st["hbm_bytes"],
                            "probe_kernel": st["probe_kernel"]}
                    if have:
                        ci = ix.topk_tile_cut_info()
                        call.update(applied=ci["applied"], declined=ci["declined"], pairs_emitted=ci["pairs_emitted"],
                                    rounds_cut=ci["rounds_cut"],
                                    emitted_share=ci["pairs_emitted"] / max(ti["pairs_over_theta"], 1))
                    row["calls"].append(call)
        finally:
            for _, ix in handles:
                ix.close()
        out[name] = row
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--shape", default="all")
    ap.add_argument("--window-pairs", type=int, nargs="+", default=None,
                    help="measure apss_set_top_k_window at these budgets against the unwindowed call (see the module docstring)")
    ap.add_argument("--tile-cut", action="store_true",
                    help="measure apss_set_top_k_tile_cut off against on, a handle each (see the module docstring)")
    a = ap.parse_args()
    if a.window_pairs:
        return windows_main(a)
    if a.tile_cut:
        return tile_cut_main(a)
    out = {}
    for key, (name, n, dim, nnz, zipf, theta) in SHAPES.items():
        if a.shape not in ("all", key):
            continue
        rp, idx, val = synth.make_vectors(n, dim, nnz, zipf, seed=11)
        row = {"n": n, "dim": dim, "nnz": nnz, "zipf_s": zipf, "theta": theta, "k": a.k, "calls": []}
        with ApssIndex(dim, theta) as ix:
            ix.insert(np.arange(n), rp, idx, val)
            ix.self_join(fetch=False)  # warm-up, k = 0
            row["hbm_bytes_k0"] = ix.stats()["hbm_bytes"]
            ix.set_top_k(a.k)
            ix.self_join(fetch=False)  # warm-up, k > 0: sizes the pass's buffers
            row["hbm_bytes_k"] = ix.stats()["hbm_bytes"]
            for rep in range(a.reps):
                for k in (0, a.k):
                    ix.set_top_k(k)
                    ix.self_join(fetch=False)
                    st, ti = ix.stats(), ix.topk_info()
                    call = {"k": k, "probe_ms": st["probe_ms"], "rescore_ms": st["rescore_ms"], "select_ms": ti["select_ms"],
                            "pairs_over_theta": ti["pairs_over_theta"], "kept": ti["kept"], "queries_cut": ti["queries_cut"],
                            "longest_segment": ti["longest_segment"], "select_launches": ti["select_launches"]}
                    if k:
                        call["floor_read_list_ms"] = 12.0 * ti["pairs_over_theta"] / COPY_PEAK * 1e3
                        moved = design_bytes(ti["pairs_over_theta"], ti["kept"], n)
                        call["design_bytes"] = moved
                        call["floor_design_bytes_ms"] = moved / COPY_PEAK * 1e3
                    row["calls"].append(call)
        out[name] = row
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
