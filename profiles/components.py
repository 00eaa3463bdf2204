"""The components stage (apss_set_components) timed on one GPU.  One JSON line per measurement on stdout;
profiles/components.md quotes them.
  python profiles/components.py join      C3 (N = 1M) self-join with the setting on: hook_ms, label_ms, wall, against the path it
                                          replaces (fetch the whole list, scipy connected_components on the host); labels compared
  python profiles/components.py stream    bench_stream.py's shape: 1M vectors in 1,024-row insert_and_query calls, off against on
  python profiles/components.py stream-short [on]   the first 64 such calls alone (the run a kernel trace is taken of)
  python profiles/components.py path | star         the adversarial shapes at 1M rows through apss_self_join
  python profiles/components.py repair    the stream case's store (1M rows) with planted duplicate clusters, 1,000 ids removed in
                                          batches of 100 with apss_set_components_repair on: wall of every remove, rows_rejoined,
                                          detach_ms, rejoin_ms; then compact() with the forest carried
  python profiles/components.py rejoin    the route without the repair, which every commit since apss_set_components has: the same
                                          removes, each followed by the apss_self_join that makes the structure complete again;
                                          then compact()"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "all-pairs-similarity_amd")):
    sys.path.insert(0, p)
from apss import _lib, synth  # noqa: E402
from apss.engine import ApssIndex  # noqa: E402


def med(xs):
    return float(np.median(xs))


def c3():
    c = synth.CONFIGS["c3"]
    rp, idx, val = synth.make_vectors(c["n"], c["dim"], c["nnz"], c["zipf_s"], c["seed"])
    return c, rp, idx, val


def join():
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    c, rp, idx, val = c3()
    n = c["n"]
    ids = np.arange(n, dtype=np.int64)
    with ApssIndex(c["dim"], c["theta"]) as ix:
        ix.insert(ids, rp, idx, val)
        walls = {}
        for on in (False, True):
            ix.set_components(on)
            w, hook, label, read = [], [], [], []
            for r in range(6):
                t = time.perf_counter()
                pairs = ix.self_join(fetch=False)
                w.append((time.perf_counter() - t) * 1e3)
                if on:
                    t = time.perf_counter()
                    info = ix.components_info()
                    read.append((time.perf_counter() - t) * 1e3)
                    hook.append(info["hook_ms"])
                    label.append(info["label_ms"])
            walls[on] = med(w[2:])
        t = time.perf_counter()
        labels, _ = ix.components()
        fetch_labels = (time.perf_counter() - t) * 1e3
        # the path this replaces
        t = time.perf_counter()
        q, cc, _ = ix.fetch()
        t_fetch = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        g = sp.coo_matrix((np.ones(len(q), np.int8), (q, cc)), shape=(n, n)).tocsr()
        _, comp = connected_components(g, directed=False)
        first = np.full(comp.max() + 1, n, np.int64)
        np.minimum.at(first, comp, np.arange(n))
        host_labels = first[comp].astype(np.int32)
        t_host = (time.perf_counter() - t) * 1e3
        print(json.dumps(dict(what="C3 self-join, N=1M", pairs=int(pairs), call_wall_ms_off=walls[False], call_wall_ms_on=walls[True],
                              hook_ms=med(hook[2:]), label_ms=med(label[2:]), info_read_wall_ms=med(read[2:]), fetch_labels_ms=fetch_labels,
                              components=info["components"], largest=info["largest"], unions_total=info["unions_total"],
                              host_fetch_list_ms=t_fetch, host_scipy_ms=t_host, labels_identical=bool(np.array_equal(labels, host_labels)))), flush=True)


def stream(calls=None, settings=(False, True)):
    import torch
    c, rp, idx, val = c3()
    n, nnz, B = c["n"], c["nnz"], 1024
    dev = torch.device("cuda:0")
    d_idx, d_val = torch.from_numpy(idx).to(dev), torch.from_numpy(val.astype(np.float32)).to(dev)
    d_ids = torch.arange(n, dtype=torch.int64, device=dev)
    d_rp = torch.arange(0, (B + 1) * nnz, nnz, dtype=torch.int64, device=dev)
    for on in settings:
        with ApssIndex(c["dim"], c["theta"], capacity_rows=n, capacity_nnz=idx.size, components=on) as ix:
            dts = []
            for b0 in range(0, n, B)[:calls]:
                b1 = min(n, b0 + B)
                sl = slice(b0 * nnz, b1 * nnz)
                torch.cuda.synchronize()
                t = time.perf_counter()
                ix.insert_and_query_dev(d_ids[b0:b1], d_rp[:b1 - b0 + 1], d_idx[sl], d_val[sl])
                dts.append((time.perf_counter() - t) * 1e3)
            rec = dict(what="stream of 1024-row insert_and_query calls", components=on, calls=len(dts), mean_call_ms=float(np.mean(dts)),
                       median_call_ms=med(dts), total_s=float(np.sum(dts)) / 1e3)
            if on:
                t = time.perf_counter()
                info = ix.components_info()
                rec.update(info_read_wall_ms=(time.perf_counter() - t) * 1e3, label_ms=info["label_ms"], n_components=info["components"],
                           largest=info["largest"], complete=info["complete"])
            print(json.dumps(rec), flush=True)


def adversarial(which):
    n = 1_000_000
    if which == "path":  # row i: terms {i, i + 1}, slots in reverse order of i
        order = np.arange(n, dtype=np.int64)[::-1]
        rp = 2 * np.arange(n + 1, dtype=np.int64)
        idx = np.stack([order, order + 1], axis=1).astype(np.int32).ravel()
        val = np.full(2 * n, 1.0 / np.sqrt(2.0))
        dim, theta, flags = n + 1, 0.4, 0
    else:  # a hub of 512 terms at 1/sqrt(512) in slot n / 2; every leaf: one hub term at 0.04 and a private term -- hub . leaf =
        # 1.77e-3, leaf . leaf = 1.6e-3, theta between them: every edge touches the hub
        hub, a = n // 2, 0.04
        lens = np.full(n, 2, np.int64)
        lens[hub] = 512
        rp = np.concatenate([[0], np.cumsum(lens)])
        idx, val = np.empty(rp[-1], np.int32), np.empty(rp[-1])
        leaf = np.delete(np.arange(n), hub)
        idx[rp[leaf]] = leaf % 512
        idx[rp[leaf] + 1] = 512 + leaf
        val[rp[leaf]] = a
        val[rp[leaf] + 1] = np.sqrt(1 - a * a)
        idx[rp[hub]:rp[hub + 1]] = np.arange(512)
        val[rp[hub]:rp[hub + 1]] = 1.0 / np.sqrt(512.0)
        dim, theta, flags = 512 + n, 1.7e-3, _lib.FLAG_EXACT_ACCUM
    with ApssIndex(dim, theta, flags=flags, components=True) as ix:
        ix.insert(np.arange(n, dtype=np.int64), rp, idx, val)
        for r in range(3):
            t = time.perf_counter()
            pairs = ix.self_join(fetch=False)
            wall = (time.perf_counter() - t) * 1e3
            info = ix.components_info()
            print(json.dumps(dict(what=which + " of 1M rows", run=r, pairs=int(pairs), call_wall_ms=wall, hook_ms=info["hook_ms"], label_ms=info["label_ms"],
                                  components=info["components"], largest=info["largest"], unions_total=info["unions_total"])), flush=True)
        labels, _ = ix.components()
        print(json.dumps(dict(what=which + " of 1M rows", labels_all_zero=bool((labels == 0).all()))), flush=True)


def removal(repair_on):
    c = synth.CONFIGS["c3"]
    n, dup = c["n"], 0.2
    rp, idx, val = synth.make_vectors(n, c["dim"], c["nnz"], c["zipf_s"], c["seed"], dup_frac=dup)
    ids = np.arange(n, dtype=np.int64)
    gone = np.random.default_rng(1).permutation(n)[:1000].astype(np.int64)
    kw = dict(components_repair=n) if repair_on else {}
    with ApssIndex(c["dim"], c["theta"], components=True, **kw) as ix:
        ix.insert(ids, rp, idx, val)
        ix.self_join(fetch=False)
        start = ix.components_info()
        print(json.dumps(dict(what="store", rows=n, dup_frac=dup, components=start["components"], largest=start["largest"],
                              complete=start["complete"])), flush=True)
        for b in range(0, 1000, 100):
            t = time.perf_counter()
            marked = ix.remove(gone[b:b + 100])
            remove_ms = (time.perf_counter() - t) * 1e3
            rec = dict(what="remove of 100 ids", repair=repair_on, batch=b // 100, rows_marked=int(marked), remove_wall_ms=remove_ms)
            if repair_on:
                ri = ix.components_repair_info()
                rec.update(declined=ri["declined"], components_touched=ri["components_touched"], rows_rejoined=ri["rows_rejoined"],
                           pairs_rejoined=ri["pairs_rejoined"], detach_ms=ri["detach_ms"], rejoin_ms=ri["rejoin_ms"], launches=ri["launches"])
            else:
                t = time.perf_counter()
                ix.self_join(fetch=False)
                rec.update(self_join_wall_ms=(time.perf_counter() - t) * 1e3)
                rec.update(route_wall_ms=remove_ms + rec["self_join_wall_ms"])
            info = ix.components_info()
            rec.update(complete=info["complete"], components=info["components"])
            print(json.dumps(rec), flush=True)
        t = time.perf_counter()
        ix.compact()
        rec = dict(what="compact", repair=repair_on, compact_wall_ms=(time.perf_counter() - t) * 1e3, compact_ms=ix.removal_info()["compact_ms"])
        info = ix.components_info()
        rec.update(complete=info["complete"], components=info["components"], rows=info["rows"])
        if repair_on:
            rec.update(remap_ms=ix.components_repair_info()["remap_ms"])
        print(json.dumps(rec), flush=True)


which = sys.argv[1] if len(sys.argv) > 1 else "join"
if which == "join":
    join()
elif which == "stream":
    stream()
elif which == "stream-short":
    stream(calls=64, settings=(len(sys.argv) > 2 and sys.argv[2] == "on",))
elif which in ("repair", "rejoin"):
    removal(which == "repair")
else:
    adversarial(which)
