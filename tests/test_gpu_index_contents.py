"""GPU tests of what the index build leaves in HBM: every built posting of a rendering against a host reference
(tests/index_view.py; the comparison itself is tested without a GPU in test_index_compare.py).

The join re-scores every survivor from the fp32 store, so a wrong index mostly still joins correctly at test sizes: a posting
with a wrong slot is a spurious candidate that k_rescore throws away, a weight rounded the wrong way or a posting dropped at a
range, sub-range or tile boundary lowers one filter sum by about 0.01, padding words, segment starts, max_seg / long_segs and
tile_min are invisible to a result test.  Here the view of a built rendering (apss_index_view_get) is read back and held to:
segment lengths of every (tile, term), aligned and disjoint extents, tile bases, the postings of every segment as sorted
multisets of (slot, weight bits) bit for bit, zero padding and no zero posting, max_seg, long_segs, tile_min.  Every case also
joins and compares the pairs with the oracle, so a view that disagreed with what the probe reads would show.

`build_trace` makes the library say which kernels a build took; every case checks it."""
import functools

import numpy as np
import pytest

import index_view as iv
from apss import synth
from build_inputs import index_inputs, two_long_segments
from helpers import assert_same_pairs, to_map
from store_view import read_store

pytestmark = pytest.mark.gpu

THETA = 0.6
TR = 256          # tile_rows of the handle: 256 rows per exact tile, 512 per coarse tile
SHARD_CAP = 0.005  # postings whose three admissible roundings differ (index_view: expected 0.07 %)


@pytest.fixture(scope="module")
def engine():
    from apss import _lib, engine
    _lib.lib()  # raises if the HIP library is missing: no fallback
    return engine


def _trace(capfd):
    return [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[apss] ")]


def _builds(lines):
    return [ln for ln in lines if ln.startswith("[apss] build ")]


def _took(capfd, what, *also):
    """every index build since the last look took the `what` kernels (and there was one); `also`: text each build's lines hold"""
    lines = _trace(capfd)
    builds = _builds(lines)
    assert builds and all(": %s," % what in ln for ln in builds), lines
    for text in also:
        assert sum(text in ln for ln in lines) >= len(builds), (text, lines)
    return builds


def _check(ix, rendering, form, cb, long_segs="exact", head_terms=None, ref=None):
    """the view of a rendering against the reference of the store as the device holds it; returns (view, reference, postings off the central
    rounding: 0 unless the weights are scaled)"""
    got = iv.read_index(ix, rendering)
    assert got is not None, "rendering %d is not built" % rendering
    assert (got.form, got.cb, got.align) == (form, cb, 16 if form == "exact" else 32), (got.form, got.cb, got.align)
    if ref is None:
        ref = iv.reference_index(read_store(ix), got.cb, got.built_rows, got.form, head_terms=head_terms, sub=got.sub, dim=got.dim)
    got_off = iv.assert_index_equal(got, ref, long_segs)
    assert got_off == 0 or got.scaled
    return got, ref, got_off


@functools.lru_cache(maxsize=None)
def _inputs(dim, cb, align):
    return index_inputs(dim, seed=500 + dim, cb=cb, align=align, range_terms=512 if dim == 2000 else 16384)


_oracle_pairs = {}


def _want_pairs(oracle, key, dim, rp, idx, val, theta=THETA):
    """the oracle's self-join of an input, computed once and shared"""
    if key not in _oracle_pairs:
        _oracle_pairs[key] = to_map(*oracle.selfjoin_pairs(dim, theta, rp, idx, val))
    return _oracle_pairs[key]


def _assert_lengths_reached(ref, align):
    """the input does what it was built for: segments of align - 1, align, align + 1 and of more than 256 postings"""
    lens = set(np.unique(iv.segment_counts(ref)).tolist())
    assert {align - 1, align, align + 1} <= lens and max(lens) > iv.LONG_LEN, sorted(lens)[-8:]


# ---- build kinds on the coarse slot * 2 form: every kind's view equals the same reference ----
KINDS = {
    "atomic": ("build_atomic", "atomic", ()),
    "stream": ("build_lds,build_stream", "stream", ()),
    "runs_two_pass": ("build_lds,build_runs", "runs", ("sub-ranges of 256 terms",)),
    "runs_one_pass": ("build_lds,build_runs,run_sub=0", "runs", ("sub-ranges of 0 terms",)),
    "runs_sub64": ("build_lds,build_runs,run_sub=64", "runs", ("sub-ranges of 64 terms",)),
    "runs_lanes4": ("build_lds,build_runs,run_lanes=4", "runs", ("4 lanes per row",)),
    "runs_lanes32": ("build_lds,build_runs,run_lanes=32", "runs", ("32 lanes per row",)),
    "runs_range8192": ("build_lds,build_runs,run_range=8192", "runs", ("of 8192 terms",)),
}
DIMS = (2000, 4097, 16385, 100_000)  # a short last range (ranges of 512); one term past a scan block of 4,096; 16,385; 7 ranges
_kind_refs = {}


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_build_kinds_leave_the_reference_index(engine, oracle, monkeypatch, capfd, kind, dim):
    hooks, what, also = KINDS[kind]
    if dim == 2000 and what == "runs" and "run_range" not in hooks:
        hooks += ",run_range=512"
        also += ("4 ranges of 512 terms",)
    rp, idx, val, common = _inputs(dim, 2 * TR, 32)
    n = len(rp) - 1
    capfd.readouterr()
    monkeypatch.setenv("APSS_DEBUG", hooks + ",build_trace")
    with engine.ApssIndex(dim, THETA, tile_rows=TR) as ix:
        ix.insert(np.arange(n), rp, idx, val)
        _took(capfd, what, *also)
        store = read_store(ix)
        if dim not in _kind_refs:  # one reference per input, shared by the kinds: their views are thereby compared pairwise
            got = iv.read_index(ix, 1)
            ref = iv.reference_index(store, 2 * TR, n, "slot2", dim=dim)
            _assert_lengths_reached(ref, 32)
            assert got.n_tiles == 5 and n % (2 * TR) and ref.bits.size == idx.size
            _kind_refs[dim] = (store, ref)
            # (the comparison bites on what the device wrote: one fp16 ulp in one posting of the read-back view is found)
            bad = got._replace(post=got.post.copy())
            bad.post[int(got.base[1] + got.seg[1, common, 0])] ^= 1 << 16
            with pytest.raises(AssertionError, match=r"tile 1 term %d posting \d+ of the sorted segment" % common):
                iv.assert_index_equal(bad, ref)
        first, ref = _kind_refs[dim]
        assert all(np.array_equal(a, b) for a, b in zip(store[:4], first[:4])), "the store differs between build kinds"
        got, _, _ = _check(ix, 1, "slot2", 2 * TR, ref=ref)
        assert not got.scaled and got.sub is None and got.tile_min is None and got.chunk_weight > 0
        assert iv.read_index(ix, 0) is None  # the exact rendering is built by the first call that needs it
        pairs = to_map(*ix.self_join())
    want = _want_pairs(oracle, ("kinds", dim), dim, rp, idx, val)
    assert len(want) > 30
    assert_same_pairs(pairs, want, THETA)


# ---- the exact rendering ----
@pytest.mark.parametrize("kind", ["atomic", "stream", "runs_two_pass"])
def test_exact_rendering(engine, oracle, monkeypatch, capfd, kind):
    """FLAG_EXACT_ACCUM: 8-B postings {slot, fp32 w}, 256 rows per tile, 16 postings per aligned unit; the run-reading build
    scatters in one pass there (the two-pass form is the coarse renderings').  A tile of 256 rows holds no segment of more
    than 256 postings: the longest is a whole tile's."""
    from apss import _lib
    hooks, what, _ = KINDS[kind]
    dim = 100_000
    rp, idx, val, common = _inputs(dim, TR, 16)
    n = len(rp) - 1
    capfd.readouterr()
    monkeypatch.setenv("APSS_DEBUG", hooks + ",build_trace")
    with engine.ApssIndex(dim, THETA, tile_rows=TR, flags=_lib.FLAG_EXACT_ACCUM) as ix:
        ix.insert(np.arange(n), rp, idx, val)
        builds = _took(capfd, what, *(("sub-ranges of 0 terms",) if what == "runs" else ()))
        assert all("build exact" in ln for ln in builds)
        got, ref, off = _check(ix, 0, "exact", TR)
        lens = set(np.unique(iv.segment_counts(ref)).tolist())
        assert {15, 16, 17} <= lens and TR - 8 < max(lens) <= TR and got.n_tiles == 9 and got.max_seg == max(lens) and got.long_segs == 0
        assert iv.read_index(ix, 1) is None
        pairs = to_map(*ix.self_join())
    assert_same_pairs(pairs, _want_pairs(oracle, ("exact", dim), dim, rp, idx, val), THETA)


# ---- the other posting forms ----
def _signed(rp, idx, val, seed):
    """weights of either sign, and in every fifth row one weight below fp16's range (of either sign)"""
    rng = np.random.default_rng(seed)
    val = val * rng.choice([-1.0, 1.0], val.size)
    for r in range(0, len(rp) - 1, 5):
        if rp[r + 1] - rp[r] >= 3:
            val[rp[r] + 1] = 1e-9 if r % 10 else -1e-9
    return val


@pytest.mark.parametrize("signed", [False, True])
def test_plain_slot_form(engine, oracle, monkeypatch, capfd, signed):
    """65536-row tiles (the cx_tile hook): the slot field holds the plain slot.  Signed: the sign bit of the fp16 is kept, a weight
    below fp16's range becomes bits 1 (0x8000 with the sign), never the zero word."""
    dim = 16385
    rp, idx, val, _ = _inputs(dim, 2 * TR, 32)
    if signed:
        val = _signed(rp, idx, val, 11)
    n = len(rp) - 1
    capfd.readouterr()
    monkeypatch.setenv("APSS_DEBUG", "cx_tile=65536,build_trace")
    with engine.ApssIndex(dim, THETA, tile_rows=TR) as ix:
        ix.insert(np.arange(n), rp, idx, val)
        assert _builds(_trace(capfd))
        got, ref, off = _check(ix, 1, "plain", 65536)
        assert got.n_tiles == 1 and got.max_seg > iv.LONG_LEN
        if signed:
            _assert_signed(ref)
        pairs = to_map(*ix.self_join())
    assert_same_pairs(pairs, _want_pairs(oracle, ("plain", signed), dim, rp, idx, val), THETA)


def _assert_signed(ref):
    neg = ref.bits & 0x8000 != 0
    assert 0.3 < neg.mean() < 0.7
    assert (ref.bits == 1).sum() > 50 and (ref.bits == 0x8000).sum() > 50 and (ref.bits != 0).all()


@pytest.mark.parametrize("kind", ["atomic", "runs_two_pass"])
def test_signed_weights_on_the_slot2_form(engine, oracle, monkeypatch, capfd, kind):
    hooks, what, also = KINDS[kind]
    dim = 16385
    rp, idx, val, _ = _inputs(dim, 2 * TR, 32)
    val = _signed(rp, idx, val, 12)
    n = len(rp) - 1
    capfd.readouterr()
    monkeypatch.setenv("APSS_DEBUG", hooks + ",build_trace")
    with engine.ApssIndex(dim, THETA, tile_rows=TR) as ix:
        ix.insert(np.arange(n), rp, idx, val)
        _took(capfd, what, *also)
        got, ref, off = _check(ix, 1, "slot2", 2 * TR)
        _assert_signed(ref)
        pairs = to_map(*ix.self_join())
    assert_same_pairs(pairs, _want_pairs(oracle, ("signed", 12), dim, rp, idx, val), THETA)


def test_wide_form_by_the_librarys_own_policy(engine, oracle, monkeypatch, capfd):
    """tile_rows = 0 leaves the tile to the library: non-negative unit rows of 10 terms at dim 100,000 give 32768 * 10 / 100,000
    = 3.3 postings per segment of a 32768-row tile -- under 8, so it takes 131072-row tiles with 8-bit accumulators, whose
    postings are slot << 15 | fp15."""
    n, dim = 2500, 100_000
    rp, idx, val = synth.make_vectors(n, dim, 10, 0.0, seed=808, dup_frac=0.1)
    assert (val >= 0).all()
    capfd.readouterr()
    monkeypatch.setenv("APSS_DEBUG", "build_trace")
    with engine.ApssIndex(dim, THETA) as ix:
        ix.insert(np.arange(n), rp, idx, val)
        assert _builds(_trace(capfd))
        got, ref, off = _check(ix, 1, "wide", 131072)
        assert got.n_tiles == 1 and (ref.bits < 0x8000).all()
        pairs = to_map(*ix.self_join())
        after = iv.read_index(ix, 1)
        assert after.form == "wide", "the join left the 8-bit filter: %s" % ix.stats()["downgrades"]
    want = _want_pairs(oracle, "wide", dim, rp, idx, val)
    assert len(want) > 100
    assert_same_pairs(pairs, want, THETA)


# ---- bucketed build of a large dim ----
def test_bucketed_build(engine, oracle, monkeypatch, capfd):
    """dim 300,000 = 19 ranges of 16384 terms, more than the LDS kinds take: the entries are bucketed by 37 ranges of 8192 terms
    first, five coarse tiles from tile 0.  One tile group only: several groups need more entries than their scratch holds
    (6e8), which no test size reaches."""
    dim = 300_000
    rp, idx, val, _ = _inputs(dim, 2 * TR, 32)
    n = len(rp) - 1
    capfd.readouterr()
    monkeypatch.setenv("APSS_DEBUG", "build_trace")
    with engine.ApssIndex(dim, THETA, tile_rows=TR) as ix:
        ix.insert(np.arange(n), rp, idx, val)
        _took(capfd, "bucketed", "37 ranges of 8192 terms", "tiles [0, 5)")
        got, ref, off = _check(ix, 1, "slot2", 2 * TR)
        _assert_lengths_reached(ref, 32)
        pairs = to_map(*ix.self_join())
    assert_same_pairs(pairs, _want_pairs(oracle, "bucketed", dim, rp, idx, val), THETA)


# ---- k_tile_place_sub: a corner too large to assemble in LDS ----
def test_place_sub_writes_a_large_corner_posting_by_posting(engine, oracle, monkeypatch, capfd):
    """default tile_rows (32768 coarse rows per tile), 20,000 rows of 20 terms that all hold terms 5 and 9: the sub-range
    [0, 256) of the one tile holds two segments of 20,000 postings -- 160 KB, over the 60 KB a workgroup of k_tile_place_sub
    stages -- so its postings are written one by one.  (32768 * 22 / 20,000 = 36 postings per segment: the policy keeps
    32768-row tiles.)"""
    n, dim = 20_000, 20_000
    rp, idx, val = two_long_segments(n, dim, 20, seed=31)
    capfd.readouterr()
    monkeypatch.setenv("APSS_DEBUG", "build_lds,build_runs,build_trace")
    with engine.ApssIndex(dim, THETA) as ix:
        ix.insert(np.arange(n), rp, idx, val)
        _took(capfd, "runs", "sub-ranges of 256 terms")
        got, ref, off = _check(ix, 1, "slot2", 32768)
        cnt = iv.reference_counts(ref)
        assert got.n_tiles == 1 and cnt[0, 5] == cnt[0, 9] == n and got.max_seg == n and got.long_segs == 2
        # the corner of sub-range 0: from term 0's start to term 256's
        assert int(got.seg[0, 256, 0]) - int(got.seg[0, 0, 0]) > 15360
        nq = 300
        sl = slice(0, rp[nq])
        pairs = to_map(*ix.query(np.arange(nq) + n, rp[:nq + 1], idx[sl], val[sl]))
    want = {(q + n, c): s for (q, c), s in to_map(*oracle.selfjoin_pairs(dim, THETA, rp, idx, val, 0, nq)).items()}
    for q in range(nq):  # (an outside batch also meets its own stored copy)
        want[(q + n, q)] = float(np.dot(val[rp[q]:rp[q + 1]], val[rp[q]:rp[q + 1]]))
    want = {k: v for k, v in want.items() if v >= THETA}
    assert len(want) > nq
    assert_same_pairs(pairs, want, THETA)


# ---- append ----
@pytest.mark.parametrize("hook", ["", ",no_append"])
@pytest.mark.parametrize("path", ["coarse", "exact"])
def test_view_after_every_batch(engine, oracle, monkeypatch, capfd, hook, path):
    """Four batches.  The second lands in the partly filled last tile only (k_tile_shift moves the tile's postings, the new ones
    go behind them; with no_append the tile is rebuilt by the run-reading kernels from a tile that is not the first); the third,
    40 rows, waits outside the coarse index (built_rows < rows: the view covers built_rows only); the fourth folds it in, fills
    the tile and builds the tiles beyond.  The common term is held by the first 400 rows of the appended-to coarse tile: its
    segment passes 256 postings DURING the append.

    max_seg is exact after every batch (segments only grow, and the device keeps the maximum).  long_segs is what
    k_tile_scan_part's count_long promises: the long segments of every tile AS IT WAS WHEN LAST BUILT WHOLE, summed since the
    last build from tile 0 -- an append does not recount its tile ("an appended-to tile was counted before"), so a segment that
    grows long by an append is missed, and a tile rebuilt from tile0 > 0 (no_append) is counted again.  The probe reads it only
    to choose between two correct filter kernels (few_longs); what it needs for correctness is max_seg."""
    from apss import _lib
    coarse = path == "coarse"
    cb, form, rendering = (2 * TR, "slot2", 1) if coarse else (TR, "exact", 0)
    dim = 100_000
    rp, idx, val, common = index_inputs(dim, seed=4242, cb=2 * TR, align=32, counts={2: 400})
    n = len(rp) - 1
    cuts = (0, 2 * 2 * TR + 188, 2 * 2 * TR + 288, 2 * 2 * TR + 328, n)
    capfd.readouterr()
    monkeypatch.setenv("APSS_DEBUG", "build_lds,build_runs,build_trace" + hook)
    with engine.ApssIndex(dim, THETA, tile_rows=TR, flags=0 if coarse else _lib.FLAG_EXACT_ACCUM) as ix:
        promised = 0
        for b, (b0, b1) in enumerate(zip(cuts[:-1], cuts[1:])):
            sl = slice(rp[b0], rp[b1])
            ix.insert(np.arange(b0, b1), rp[b0:b1 + 1] - rp[b0], idx[sl], val[sl])
            builds = _builds(_trace(capfd))
            waits = coarse and b == 2
            built = cuts[2] if waits else b1
            prev_built = 0 if b == 0 else (cuts[2] if coarse and b == 3 else b0)
            got = iv.read_index(ix, rendering)
            assert got.built_rows == built and ix.size()[0] == b1
            ref = iv.reference_index(read_store(ix), cb, built, form, dim=dim)
            cnt = iv.reference_counts(ref)
            longs = (cnt > iv.LONG_LEN).sum(axis=1)
            t0 = prev_built // cb  # the partly filled tile the batch lands in
            if b == 0:
                promised = int(longs.sum())
                assert builds and all("tiles [0," in ln for ln in builds)
            elif waits:
                assert not builds
            elif hook:  # rebuilt from the partly filled tile on: counted again
                promised += int(longs[t0:].sum())
                assert builds and all("tiles [%d," % t0 in ln and ": runs," in ln for ln in builds), builds
            else:       # appended to: not recounted; the tiles beyond are
                promised += int(longs[t0 + 1:].sum())
                assert all("tiles [%d," % (t0 + 1) in ln for ln in builds) and bool(builds) == (got.n_tiles > t0 + 1), builds
            iv.assert_index_equal(got, ref, long_segs=promised)
            if coarse and b < 2:
                held = sum(int(common in idx[rp[r]:rp[r + 1]]) for r in range(2 * cb, b1))  # (every non-empty row of the tile so far)
                assert cnt[2, common] == held == got.max_seg and b1 - 2 * cb - 7 <= held
                assert (held > iv.LONG_LEN) == (b == 1)  # the segment passes 256 postings during the append
                assert got.long_segs == (1 if hook and b == 1 else 0)
        assert got.n_tiles == -(-n // cb)
        pairs = to_map(*ix.self_join())
    assert_same_pairs(pairs, _want_pairs(oracle, "append", dim, rp, idx, val), THETA)


# ---- term shard ----
@pytest.fixture(scope="module")
def shard_device(engine):
    """the shard engines hand torch tensors to the library: torch and its device start once, outside the tests' own time"""
    import torch
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    return dev


@pytest.mark.parametrize("kind", ["runs_two_pass", "stream"])
def test_term_shard(engine, oracle, shard_device, monkeypatch, capfd, kind):
    """terms [10,000, 60,000) of dim 100,000 as one of three shards that together join like the oracle.  The shard's coarse
    weights are stored divided by sub[row] (inside the band of one fp32 division, index_view), sub is |x_g| / |x| of the whole
    input rows inside its derived bound, tile_min the smallest positive sub of each tile, and every segment of a term outside the
    range is empty."""
    from apss.dist import HipShardEngine, join_shards_local
    hooks, what, also = KINDS[kind]
    dim, lo, hi = 100_000, 10_000, 60_000
    rp, idx, val, _ = _inputs(dim, 2 * TR, 32)
    n = len(rp) - 1
    capfd.readouterr()
    monkeypatch.setenv("APSS_DEBUG", hooks + ",build_trace")
    engines = [HipShardEngine(dim, THETA, tr, shard_device, tile_rows=TR) for tr in ((0, lo), (lo, hi), (hi, dim))]
    try:
        for e in engines:
            e.load(rp, idx, val)
        q, c, s, _ = join_shards_local(engines, n, THETA)
        _took(capfd, what, *also)
        ix = engines[1].ix
        store = read_store(ix)
        inside = (idx >= lo) & (idx < hi)
        assert store.indices.size == int(inside.sum()) and np.array_equal(store.indices, idx[inside])
        got, ref, off = _check(ix, 1, "slot2", 2 * TR)
        assert got.scaled and got.sub is not None and got.tile_min is not None
        share = iv.excused_share(ref)
        print("term shard (%s): %d postings, excused share %.4f %% (cap %.1f %%), %d off the central rounding" %
              (kind, ref.bits.size, 100 * share, 100 * SHARD_CAP, off))
        assert share < SHARD_CAP and off <= share * ref.bits.size
        worst = iv.assert_sub_close(got.sub, rp, idx, val, (lo, hi))
        print("term shard (%s): worst sub error %.3f of its bound" % (kind, worst))
        cnt = iv.reference_counts(ref)
        assert cnt[:, :lo].sum() == 0 and cnt[:, hi:].sum() == 0 and not got.seg[:, :lo, 1].any() and not got.seg[:, hi:, 1].any()
        assert (got.tile_min > 0).all()
    finally:
        for e in engines:
            e.ix.close()
    assert_same_pairs(to_map(q, c, s), _want_pairs(oracle, ("kinds", dim), dim, rp, idx, val), THETA)


# ---- dense head ----
@pytest.mark.parametrize("kind", ["runs", "stream"])
def test_dense_head_index_is_the_store_minus_the_heads_terms(engine, oracle, monkeypatch, capfd, kind):
    """head_terms = 64 on Zipf rows: the block's terms are in no posting list (the index is built from the tail view), and the
    sparse half runs under the shard rule -- weights divided by the tail's share of the row"""
    n, dim, nnz = 3000, 10_000, 50
    rp, idx, val = synth.make_vectors(n, dim, nnz, 1.0, seed=95, dup_frac=0.1)
    capfd.readouterr()
    monkeypatch.setenv("APSS_DEBUG", {"runs": "build_lds,build_runs,run_range=2048", "stream": "build_lds,build_stream"}[kind] + ",build_trace")
    with engine.ApssIndex(dim, THETA, head_terms=64, tile_rows=TR) as ix:
        ix.insert(np.arange(n), rp, idx, val)
        _took(capfd, kind, *(("5 ranges of 2048 terms",) if kind == "runs" else ()))
        head = ix.head_terms()
        assert len(head) == 64
        got, ref, off = _check(ix, 1, "slot2", 2 * TR, head_terms=head)
        assert got.scaled and ref.bits.size == int((~np.isin(idx, head)).sum()) < idx.size
        assert not got.seg[:, np.asarray(head), 1].any()
        share = iv.excused_share(ref)
        print("dense head (%s): %d postings, excused share %.4f %%, %d off the central rounding" % (kind, ref.bits.size, 100 * share, off))
        assert share < SHARD_CAP and off <= share * ref.bits.size
        pairs = to_map(*ix.self_join())
        assert ix.stats()["head_terms"] == 64
    want = _want_pairs(oracle, "head", dim, rp, idx, val)
    assert len(want) > 100
    assert_same_pairs(pairs, want, THETA)


# ---- after a removal and a compaction ----
def test_rebuilt_index_after_compaction(engine, oracle, monkeypatch, capfd):
    dim = 16385
    rp, idx, val, _ = _inputs(dim, 2 * TR, 32)
    n = len(rp) - 1
    rng = np.random.default_rng(3)
    gone = np.sort(rng.choice(n, 300, replace=False))
    keep = np.setdiff1d(np.arange(n), gone)
    monkeypatch.setenv("APSS_DEBUG", "build_lds,build_runs,build_trace")
    with engine.ApssIndex(dim, THETA, tile_rows=TR) as ix:
        ix.insert(np.arange(n) + 7000, rp, idx, val)
        before, _, _ = _check(ix, 1, "slot2", 2 * TR)
        capfd.readouterr()
        ix.remove(gone + 7000)
        ix.compact()
        _took(capfd, "runs", "tiles [0, 4)")
        store = read_store(ix)
        assert np.array_equal(store.ext_ids, keep + 7000) and np.array_equal(np.diff(store.rowptr), np.diff(rp)[keep])
        got, ref, off = _check(ix, 1, "slot2", 2 * TR)
        assert got.built_rows == n - 300 and got.n_tiles == 4 and before.n_tiles == 5
        pairs = to_map(*ix.self_join())
    whole = _want_pairs(oracle, ("kinds", dim), dim, rp, idx, val)
    gone_set = set(gone.tolist())
    want = {(a + 7000, b + 7000): s for (a, b), s in whole.items() if a not in gone_set and b not in gone_set}
    assert_same_pairs(pairs, want, THETA)
