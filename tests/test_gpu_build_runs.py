"""GPU tests of the run-reading LDS index build (k_row_cuts + k_tile_runs, apss_build.hpp): a (tile, term range) workgroup
reads the runs of its range out of the term-sorted rows instead of the whole tile.  Checked against the two builds it stands
beside -- the whole-tile streaming LDS kernels (APSS_DEBUG=build_stream) and the global-atomic kernels (build_atomic) -- on the
same input: same pair keys, same work counters; and against the CPU oracle.  `build_lds,build_runs` makes small inputs take
the path, `build_trace` makes the library say on stderr which kernels a build took."""
import re

import numpy as np
import pytest

from apss import synth
from build_inputs import corner_vectors as _corner_vectors
from helpers import assert_same_pairs, to_map

pytestmark = pytest.mark.gpu

RUNS = "build_lds,build_runs,build_trace"
STREAM = "build_lds,build_stream,build_trace"
ATOMIC = "build_atomic,build_trace"


@pytest.fixture(scope="module")
def engine():
    from apss import _lib, engine
    _lib.lib()  # raises if the HIP library is missing: no fallback
    return engine


def _join(engine, dim, theta, rp, idx, val, **kw):
    n = len(rp) - 1
    with engine.ApssIndex(dim, theta, **kw) as ix:
        q, c, s = ix.insert_and_query(np.arange(n), rp, idx, val)
        st = ix.stats()
    return to_map(q, c, s), st


def _took(capfd, what):
    """every index build since the last look took the `what` kernels (and there was one)"""
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[apss] build ")]
    assert lines and all(": %s," % what in ln for ln in lines), lines
    return lines


CASES = {
    # dim 100,000: 7 ranges of 16384 terms, the last one 1,696 terms short of full
    "dim100k": (100_000, 0.6, "", 16384),
    # the scatter in one pass (straight from the runs) instead of two (partitioned into sub-ranges first); narrow sub-ranges
    "dim100k_onepass": (100_000, 0.6, ",run_sub=0", 16384),
    "dim100k_sub64": (100_000, 0.6, ",run_sub=64", 16384),
    "dim100k_lanes4": (100_000, 0.6, ",run_lanes=4", 16384),
    "dim100k_lanes32": (100_000, 0.6, ",run_lanes=32", 16384),
    "dim100k_range8192": (100_000, 0.6, ",run_range=8192,run_lanes=8", 8192),
    # a dim below one range: a run is the whole row
    "dim2048": (2048, 0.6, "", 16384),
    # ... and the same dim cut into ranges of 512 terms, dim 2000: the last range is short
    "dim2000_range512": (2000, 0.6, ",run_range=512", 512),
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("path", ["two_pass", "exact_wave"])
def test_run_build_matches_stream_and_atomic_builds(engine, oracle, monkeypatch, capfd, case, path):
    from apss import _lib
    dim, theta, extra, rt = CASES[case]
    rp, idx, val = _corner_vectors(dim, seed=1234 + dim, range_terms=rt)
    n = len(rp) - 1
    flags = {"two_pass": 0, "exact_wave": _lib.FLAG_EXACT_ACCUM}[path]
    capfd.readouterr()
    monkeypatch.setenv("APSS_DEBUG", RUNS + extra)
    got, st = _join(engine, dim, theta, rp, idx, val, tile_rows=256, flags=flags)
    lines = _took(capfd, "runs")
    assert all("%d ranges of %d terms" % (-(-dim // rt), rt) in ln for ln in lines), lines
    monkeypatch.setenv("APSS_DEBUG", STREAM)
    ref, st_ref = _join(engine, dim, theta, rp, idx, val, tile_rows=256, flags=flags)
    _took(capfd, "stream")
    monkeypatch.setenv("APSS_DEBUG", ATOMIC)
    ato, st_ato = _join(engine, dim, theta, rp, idx, val, tile_rows=256, flags=flags)
    _took(capfd, "atomic")
    assert len(got) > 100 and got.keys() == ref.keys() == ato.keys()
    for other in (st_ref, st_ato):
        assert st["candidate_pairs"] == other["candidate_pairs"]
        assert st["posting_visits"] == other["posting_visits"] == int(synth.workload_counts(dim, rp, idx)[1])
        assert st["nnz"] == other["nnz"] == idx.size and st["rows"] == other["rows"] == n
        assert st["tiles"] == other["tiles"]
    sample = 600
    want = to_map(*oracle.selfjoin_pairs(dim, theta, rp, idx, val, 0, sample))
    assert len(want) > 30
    assert_same_pairs({k: v for k, v in got.items() if k[0] < sample}, want, theta)


def test_run_build_of_a_term_shard(engine, monkeypatch, capfd):
    """a handle that keeps terms [10,000, 60,000) of dim 100,000: the cuts fall inside ranges 0 and 3, ranges 4 .. 6 hold no
    term of the handle (their workgroups leave at once); same candidates as the same handle under build_stream"""
    dim, theta = 100_000, 0.5
    rp, idx, val = _corner_vectors(dim, seed=77)
    n = len(rp) - 1
    nq = 300
    out = {}
    for name, dbg, what in (("runs", RUNS, "runs"), ("stream", STREAM, "stream")):
        capfd.readouterr()
        monkeypatch.setenv("APSS_DEBUG", dbg)
        with engine.ApssIndex(dim, theta, term_range=(10_000, 60_000), tile_rows=256) as ix:
            first = to_map(*ix.insert_and_query(np.arange(n), rp, idx, val))
            st = ix.stats()
            later = to_map(*ix.query(np.arange(nq) + n, rp[:nq + 1], idx[:rp[nq]], val[:rp[nq]]))
        _took(capfd, what)
        out[name] = (first, later, st)
    (f1, l1, s1), (f0, l0, s0) = out["runs"], out["stream"]
    assert len(f1) > 50 and f1.keys() == f0.keys() and len(l1) > 50 and l1.keys() == l0.keys()
    assert max(abs(f1[k] - f0[k]) for k in f1) <= 1e-6 and max(abs(l1[k] - l0[k]) for k in l1) <= 1e-6
    kept = int(((idx >= 10_000) & (idx < 60_000)).sum())
    for key in ("candidate_pairs", "posting_visits", "nnz", "rows", "tiles"):
        assert s1[key] == s0[key], key
    assert s1["nnz"] == kept


def test_run_build_from_a_tail_view(engine, oracle, monkeypatch, capfd):
    """a handle with a dense-head block builds its index from the tail view (the rows without the block's entries, order
    kept): same pairs as under build_stream and as the oracle"""
    n, dim, nnz, theta = 3000, 10_000, 50, 0.6
    rp, idx, val = synth.make_vectors(n, dim, nnz, 1.0, seed=95, dup_frac=0.1)
    want = to_map(*oracle.selfjoin_pairs(dim, theta, rp, idx, val))
    assert len(want) > 100
    capfd.readouterr()
    monkeypatch.setenv("APSS_DEBUG", RUNS + ",run_range=2048")
    got, st = _join(engine, dim, theta, rp, idx, val, head_terms=64, tile_rows=256)
    lines = _took(capfd, "runs")
    assert all("5 ranges of 2048 terms" in ln for ln in lines), lines
    monkeypatch.setenv("APSS_DEBUG", STREAM)
    ref, st_ref = _join(engine, dim, theta, rp, idx, val, head_terms=64, tile_rows=256)
    _took(capfd, "stream")
    assert st["head_terms"] == st_ref["head_terms"] == 64
    assert got.keys() == ref.keys()
    for key in ("candidate_pairs", "posting_visits", "nnz", "head_pairs"):
        assert st[key] == st_ref[key], key
    assert_same_pairs(got, want, theta)


@pytest.mark.parametrize("hook", ["", ",no_append"])
@pytest.mark.parametrize("path", ["two_pass", "exact_wave"])
def test_second_batch_on_a_run_built_index(engine, oracle, monkeypatch, capfd, hook, path):
    """two batches: the second lands in the partly filled last tile of a run-built index -- appended to (k_tile_shift), or with
    no_append rebuilt whole by the run-reading kernels from a tile that is not the first -- and fills tiles beyond it; every
    batch's pairs are the oracle worker's.  On the coarse rendering (two_pass) and on the exact one (exact_wave)."""
    from apss import _lib
    flags = {"two_pass": 0, "exact_wave": _lib.FLAG_EXACT_ACCUM}[path]
    dim, theta, tr = 100_000, 0.6, 256
    rp, idx, val = _corner_vectors(dim, seed=4242)
    n = len(rp) - 1
    m = 2 * tr + 188  # the first batch ends inside its third tile
    w = oracle.Worker(dim, theta)
    capfd.readouterr()
    monkeypatch.setenv("APSS_DEBUG", RUNS + hook)
    with engine.ApssIndex(dim, theta, tile_rows=tr, flags=flags) as ix:
        for b0, b1 in ((0, m), (m, n)):
            sl = slice(rp[b0], rp[b1])
            args = (np.arange(b0, b1), rp[b0:b1 + 1] - rp[b0], idx[sl], val[sl])
            want = to_map(*w.index_data(*args))
            got = to_map(*ix.insert_and_query(*args))
            assert_same_pairs(got, want, theta)
        assert ix.size() == (n, idx.size)
        whole = to_map(*oracle.selfjoin_pairs(dim, theta, rp, idx, val))
        assert len(whole) > 100
        assert_same_pairs(to_map(*ix.self_join()), whole, theta)
        assert ix.stats()["posting_visits"] == int(synth.workload_counts(dim, rp, idx)[1])
    lines = _took(capfd, "runs")
    # builds that did not start at the first tile: the tiles beyond the appended-to one, or (no_append) the partly filled one on
    assert any(re.search(r"tiles \[[1-9]", ln) for ln in lines), lines
