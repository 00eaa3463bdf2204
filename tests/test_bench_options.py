"""bench.py without a GPU: what --dump-outputs writes (order, dtypes, the size limit and its fixed sample) and the options
that are refused before anything touches a device."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _pairs(n, seed):
    rng = np.random.default_rng(seed)
    key = rng.choice(1 << 40, size=n, replace=False)
    return key >> 20, key & ((1 << 20) - 1), rng.random(n).astype(np.float32)


def test_outputs_are_sorted_float_arrays(bench):
    q, c, s = _pairs(5000, 1)
    out = bench.output_arrays(q, c, s)
    assert sorted(out) == ["candidate_ids", "query_ids", "scores"]
    assert out["query_ids"].dtype == np.float64 and out["candidate_ids"].dtype == np.float64 and out["scores"].dtype == np.float32
    order = np.lexsort((c, q))
    assert np.array_equal(out["query_ids"], q[order]) and np.array_equal(out["candidate_ids"], c[order])
    assert np.array_equal(out["scores"], s[order])


def test_large_outputs_are_a_fixed_sample_within_the_limit(bench):
    q, c, s = _pairs(20000, 2)
    limit = 3 * 4096 + 1000 * bench.DUMP_BYTES_PER_PAIR
    out = bench.output_arrays(q, c, s, limit_bytes=limit)
    assert out["scores"].size == 1000 and sum(a.nbytes for a in out.values()) <= limit
    # the sample does not depend on the order the pairs come in, and every kept pair keeps its own score
    perm = np.random.default_rng(3).permutation(q.size)
    again = bench.output_arrays(q[perm], c[perm], s[perm], limit_bytes=limit)
    for k in out:
        assert np.array_equal(out[k], again[k])
    score = {(int(a), int(b)): v for a, b, v in zip(q, c, s)}
    assert all(score[(int(a), int(b))] == v for a, b, v in zip(out["query_ids"], out["candidate_ids"], out["scores"]))
    # a pair's membership depends on the pair alone: dropping pairs outside the sample leaves the sample as it was
    inside = {(int(a), int(b)) for a, b in zip(out["query_ids"], out["candidate_ids"])}
    mask = np.array([(int(a), int(b)) in inside or i % 2 == 0 for i, (a, b) in enumerate(zip(q, c))])
    fewer = bench.output_arrays(q[mask], c[mask], s[mask], limit_bytes=limit)
    for k in out:
        assert np.array_equal(out[k], fewer[k])


def test_write_outputs_writes_npy_files(bench, tmp_path):
    q, c, s = _pairs(300, 4)
    bench.write_outputs(str(tmp_path / "out"), q, c, s)
    assert sorted(os.listdir(tmp_path / "out")) == ["candidate_ids.npy", "query_ids.npy", "scores.npy"]
    assert np.load(tmp_path / "out" / "scores.npy").size == 300


@pytest.mark.parametrize("args", [["--steps", "0"], ["--warmup", "-1"], ["--dump-outputs", "x", "--gpus", "2"],
                                  ["--dump-outputs", "x", "--solo", "2,1,0,0"]])
def test_refused_options(args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=120,
                         cwd=ROOT)
    assert out.returncode == 2 and "error" in out.stderr, (out.returncode, out.stderr[-500:])


def test_full_and_dump_outputs_are_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120,
                         cwd=ROOT)
    assert out.returncode == 0 and "--full" in out.stdout and "--dump-outputs" in out.stdout
