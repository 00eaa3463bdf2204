"""GPU tests of the one-pass ingest of plain batches (k_ingest_plain, apss_kernels.hpp): validate, store, per-row range cuts and
the df sample in one kernel, against the kernels it stands in for (APSS_DEBUG=no_fused_ingest: k_ingest_count + k_ingest_write,
k_row_cuts, k_df_sample), against the float64 restatement of ingest (store_view.py) and against the CPU oracle.

Every scenario runs twice, each time in a fresh child process (ingest_fused_child.py): one child per mode runs them all and
pickles what the library left; the tests below compare the two pickles with each other and with the references.  Shapes are
small: dim 40,000 (three ranges of 16,384 terms), 300 to 3,000 rows."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

import ingest_fused_child as child
from apss import synth
from helpers import assert_same_pairs, to_map
from store_view import Store, assert_store_equal, reference_store

pytestmark = pytest.mark.gpu

DIM = child.DIM


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{"fused": ..., "unfused": ...}: the pickled results of one child process per mode"""
    out = {}
    d = tmp_path_factory.mktemp("ingest_fused")
    for mode in ("fused", "unfused"):
        path = str(d / (mode + ".pkl"))
        env = dict(os.environ)
        env.pop("APSS_DEBUG", None)
        r = subprocess.run([sys.executable, child.__file__, mode, path], env=env, capture_output=True, text=True, timeout=300)
        err = open(path + ".stderr", errors="replace").read()[-3000:] if os.path.exists(path + ".stderr") else ""
        assert r.returncode == 0, (mode, r.returncode, r.stdout[-2000:], r.stderr[-2000:], err)
        with open(path, "rb") as f:
            out[mode] = pickle.load(f)
    return out


@pytest.fixture(scope="module")
def inputs():
    return child.scenario_inputs()


def _diag(res, prefix):
    return [ln for ln in res["diag"] if ln.startswith("[apss diag] " + prefix)]


def _same_pairs(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)


def _same_store(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)


def _assert_mode_lines(runs, key, store_rows=None):
    """the fused child ingested `key`'s store batches with k_ingest_plain, the other child with the two-pass kernels"""
    f, u = _diag(runs["fused"][key], "ingest"), _diag(runs["unfused"][key], "ingest")
    assert f and all("ingest fused:" in ln for ln in f), f
    assert u and all("ingest unfused:" in ln and "(no_fused_ingest)" in ln for ln in u), u
    assert len(f) == len(u)
    if store_rows is not None:
        assert any(" %d store rows" % store_rows in ln for ln in f), f


def test_row_shapes_store_and_join(runs, inputs, oracle):
    """row lengths 0 .. 100 around the 16-lane stride, terms on both sides of every range boundary: the store is the same bits
    as the two-pass ingest's and as the float64 restatement; the join, its work counters and every stat that is not a time
    are identical (the longest row picks the probe kernel, the largest norm scales its accumulators, the non-empty count
    enters candidate_pairs); the pairs are the oracle's"""
    rp, idx, val = inputs["shapes"]
    n = rp.size - 1
    lens = set(np.diff(rp).tolist())
    assert set(child.LENGTHS) <= lens
    for t in child.EDGE_TERMS:
        assert (idx == t).sum() >= 2
    f, u = runs["fused"]["shapes"], runs["unfused"]["shapes"]
    _assert_mode_lines(runs, "shapes", n)
    _same_store(f["store"], u["store"])
    want = reference_store([(np.arange(n) + 500, rp, idx, val)], DIM)
    assert_store_equal(Store(*f["store"], None), want)
    assert f["stats"] == u["stats"], {k: (f["stats"][k], u["stats"][k]) for k in f["stats"] if f["stats"][k] != u["stats"][k]}
    assert f["stats"]["rows"] == n and f["stats"]["nnz"] == idx.size
    assert f["stats"]["posting_visits"] == int(synth.workload_counts(DIM, rp, idx)[1])
    _same_pairs(f["pairs"], u["pairs"])
    oq, oc, os_ = oracle.selfjoin_pairs(DIM, 0.5, rp, idx, val)
    ref = to_map(oq + 500, oc + 500, os_)
    assert len(ref) > 100
    assert_same_pairs(to_map(*f["pairs"]), ref, 0.5)


def test_run_form_build_takes_the_cuts_of_the_ingest(runs, inputs, oracle):
    """the run-reading build forced (as test_gpu_build_runs.py forces it): the build reuses the cuts k_ingest_plain left -- for
    one batch, and for a second batch that starts inside a tile (its cuts extend the table; the tiles beyond the appended-to
    one are built from them) -- and computes its own under no_fused_ingest; pairs and counts are the oracle's"""
    rp, idx, val = inputs["runs"]
    n = rp.size - 1
    whole = to_map(*oracle.selfjoin_pairs(DIM, 0.5, rp, idx, val))
    assert len(whole) > 300
    visits = int(synth.workload_counts(DIM, rp, idx)[1])
    for key in ("runs_one", "runs_two"):
        f, u = runs["fused"][key], runs["unfused"][key]
        _assert_mode_lines(runs, key)
        builds = [ln for ln in f["diag"] if ln.startswith("[apss] build ")]
        assert builds and all(": runs, 3 ranges of 16384 terms" in ln for ln in builds), builds
        cuts_f, cuts_u = _diag(f, "build"), _diag(u, "build")
        assert cuts_f and len(cuts_f) == len(builds) and all(ln.endswith("cuts reused") for ln in cuts_f), cuts_f
        assert cuts_u and all(ln.endswith("cuts computed") for ln in cuts_u), cuts_u
        _same_store(f["store"], u["store"])
        assert f["stats"] == u["stats"]
        _same_pairs(f["pairs"], u["pairs"])
        assert_same_pairs(to_map(*f["pairs"]), whole, 0.5)
        assert f["stats"]["posting_visits"] == visits and f["stats"]["rows"] == n and f["stats"]["nnz"] == idx.size
    f, u = runs["fused"]["runs_two"], runs["unfused"]["runs_two"]
    ing = _diag(f, "ingest")
    assert "cuts written" in ing[0] and "cuts appended" in ing[1] and " at 700," in ing[1], ing
    # the tiles beyond the one the second batch starts in (appended to): a build that starts behind the first batch's rows
    starts = [int(re.search(r"rows \[(\d+),", ln).group(1)) for ln in _diag(f, "build")]
    assert any(r0 > 700 and r0 % 256 == 0 for r0 in starts), f["diag"]
    w = oracle.Worker(DIM, 0.5)
    m = 2 * 256 + 188
    for (b0, b1), got_f, got_u in zip(((0, m), (m, n)), f["batches"], u["batches"]):
        sl = slice(rp[b0], rp[b1])
        want = to_map(*w.index_data(np.arange(b0, b1), rp[b0:b1 + 1] - rp[b0], idx[sl], val[sl]))
        _same_pairs(got_f, got_u)
        assert_same_pairs(to_map(*got_f), want, 0.5)


MESSAGES = {"nan": "non-finite value in a vector", "inf": "non-finite value in a vector"}


@pytest.mark.parametrize("kind", child.BAD_KINDS)
def test_rejected_batch_leaves_no_trace(runs, inputs, oracle, kind):
    """a defective first batch -- the defect in a row the df sample takes, on a handle that also writes cuts -- is refused with
    the code and message of the two-pass ingest, commits nothing, and the valid batch after it gives the store, the block and
    the join of a handle that never saw it"""
    from apss import _lib
    rp, idx, val = inputs["valid"]
    n = rp.size - 1
    f, u, clean = runs["fused"]["bad_" + kind], runs["unfused"]["bad_" + kind], runs["fused"]["bad_clean"]
    ing = _diag(f, "ingest")
    assert len(ing) == 2 and all("ingest fused:" in ln and "df sample taken" in ln and "cuts written" in ln for ln in ing), ing
    assert f["err"] is not None and f["err"] == u["err"]
    assert f["err"][0] == _lib.E_INVALID and MESSAGES.get(kind, "malformed vector: indices must be strictly increasing and in [0, dim)") in f["err"][1]
    assert f["size_after"] == u["size_after"] == (0, 0)
    for other in (u, clean, runs["unfused"]["bad_clean"]):
        _same_store(f["store"], other["store"])
        _same_pairs(f["pairs"], other["pairs"])
        assert f["stats"] == other["stats"]
        assert np.array_equal(f["head"], other["head"])
    assert_store_equal(Store(*f["store"], None), reference_store([(np.arange(n) + 9000, rp, idx, val)], DIM))
    oq, oc, os_ = oracle.selfjoin_pairs(DIM, 0.5, rp, idx, val)
    assert_same_pairs(to_map(*f["pairs"]), to_map(oq + 9000, oc + 9000, os_), 0.5)


def test_head_policy_chooses_the_same_terms(runs, inputs, oracle):
    """a live head policy on a Zipf(1) batch: the sample delivered by the ingest is the sample k_df_sample takes -- same block
    terms in the same order, same survivors of the dense filter, same pairs"""
    rp, idx, val = inputs["zipf"]
    f, u = runs["fused"]["zipf"], runs["unfused"]["zipf"]
    assert any("df sample taken" in ln for ln in _diag(f, "ingest"))
    assert [ln for ln in _diag(f, "head policy") if ln.endswith("reused")] and not [ln for ln in _diag(f, "head policy") if ln.endswith("computed")]
    assert [ln for ln in _diag(u, "head policy") if ln.endswith("computed")] and not [ln for ln in _diag(u, "head policy") if ln.endswith("reused")]
    assert f["head"].size == 64 and np.array_equal(f["head"], u["head"])
    df = np.bincount(idx, minlength=DIM)
    assert set(f["head"].tolist()) <= set(np.argsort(-df, kind="stable")[:80].tolist())  # (ties at the 64th place aside: the most frequent terms)
    for key in ("head_terms", "head_survivors", "head_pairs", "posting_visits", "candidate_pairs", "filter_survivors"):
        assert f["stats"][key] == u["stats"][key], key
    assert f["stats"]["head_terms"] == 64
    _same_pairs(f["pairs"], u["pairs"])
    assert_same_pairs(to_map(*f["pairs"]), to_map(*oracle.selfjoin_pairs(DIM, 0.6, rp, idx, val)), 0.6)


def test_other_paths_unchanged(runs):
    """a negative weight takes the downgrade it took; a query-only batch gives the same answers; handles whose ingest
    transforms (normalise, a term shard) keep the two-pass kernels"""
    from apss import _lib
    f, u = runs["fused"]["negative"], runs["unfused"]["negative"]
    assert f["before"] == u["before"] and f["before"]["head_terms"] == 64 and f["before"]["downgrades"] == 0
    assert f["stats"] == u["stats"] and f["stats"]["downgrades"] & _lib.DOWNGRADE_HEAD and f["stats"]["head_terms"] == 0
    _same_pairs(f["pairs"], u["pairs"])
    assert len(f["pairs"][0]) > 50
    f, u = runs["fused"]["query_only"], runs["unfused"]["query_only"]
    assert any("query rows" in ln and "ingest fused:" in ln and "cuts none, df sample none" in ln for ln in _diag(f, "ingest")), f["diag"]
    assert f["size"] == u["size"] and f["stats"] == u["stats"]
    _same_pairs(f["pairs"], u["pairs"])
    assert len(f["pairs"][0]) > 100
    for key in ("normalize", "shard"):
        for mode in ("fused", "unfused"):
            ing = _diag(runs[mode][key], "ingest")
            assert ing and all("ingest unfused:" in ln and "(transform)" in ln for ln in ing), (key, mode, ing)
    _same_pairs(runs["fused"]["normalize"]["pairs"], runs["unfused"]["normalize"]["pairs"])
    assert runs["fused"]["shard"]["size"] == runs["unfused"]["shard"]["size"]


def test_rejected_query_batch_ends_the_earlier_results(runs):
    """a good query, then a defective query-only batch of 3,000 rows (its staging outgrows the buffers the first query's
    results point into): refused with the same error in both modes, and in both modes the result calls then answer
    APSS_E_STATE -- a query-type call ends the results of the one before, rejected or not -- never ids read from the
    rejected batch or from freed memory; the good query again gives its first answer"""
    from apss import _lib
    f, u = runs["fused"]["query_rejected"], runs["unfused"]["query_rejected"]
    assert any("ingest fused:" in ln and "3000 query rows" in ln for ln in _diag(f, "ingest")), f["diag"]
    assert any("ingest unfused:" in ln and "3000 query rows" in ln for ln in _diag(u, "ingest")), u["diag"]
    assert f["err"] is not None and f["err"] == u["err"] and f["err"][0] == _lib.E_INVALID and "malformed vector" in f["err"][1]
    assert f["after"] == u["after"] == ("error", _lib.E_STATE)
    assert f["size"] == u["size"]
    assert len(f["first"][0]) > 100
    for res in (f, u):
        _same_pairs(res["first"], res["again"])
    _same_pairs(f["first"], u["first"])


def test_default_decision_takes_the_cuts_of_the_ingest(runs, inputs, oracle):
    """nothing forced: 24 coarse tiles of 128 rows, three ranges, 50 entries per row -- build_tiles takes the run form by its own rule
    (build_plan), the ingest foresaw it with the same rule and its cuts are reused"""
    rp, idx, val = inputs["zipf"]
    f, u = runs["fused"]["default_runs"], runs["unfused"]["default_runs"]
    builds = [ln for ln in f["diag"] if ln.startswith("[apss] build ")]
    assert builds and all(": runs, 3 ranges of 16384 terms" in ln for ln in builds), builds
    assert any("cuts written" in ln for ln in _diag(f, "ingest")), f["diag"]
    cuts_f, cuts_u = _diag(f, "build"), _diag(u, "build")
    assert cuts_f and len(cuts_f) == len(builds) and all(ln.endswith("cuts reused") for ln in cuts_f), cuts_f
    assert cuts_u and all(ln.endswith("cuts computed") for ln in cuts_u), cuts_u
    assert f["stats"] == u["stats"] and f["stats"]["head_terms"] == 0
    assert f["stats"]["posting_visits"] == int(synth.workload_counts(DIM, rp, idx)[1])
    _same_pairs(f["pairs"], u["pairs"])
    assert_same_pairs(to_map(*f["pairs"]), to_map(*oracle.selfjoin_pairs(DIM, 0.6, rp, idx, val)), 0.6)
