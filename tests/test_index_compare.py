"""CPU checks of the index comparison itself (tests/index_view.py): a small reference index built in numpy and rendered into
the device layout is accepted in every posting form, and every planted fault -- the slips an index build can make without the
join noticing -- is rejected with the tile, term and posting it sits at.  No GPU: the GPU tests (test_gpu_index_contents.py)
lean on exactly this comparison."""
import re

import numpy as np
import pytest

import index_view as iv
from store_view import Store

DIM, CB, ROWS = 40, 64, 150  # three tiles, the last one partial (22 rows)
ALIGN = {"exact": 16, "slot2": 32, "plain": 32, "wide": 32}
COMMON = 7  # a term every row of tile 0 holds: a segment of exactly 64 postings (two aligned units, no padding)


def _store(signed=True):
    rng = np.random.default_rng(5)
    rows = []
    for r in range(ROWS):
        t = rng.choice(DIM, size=int(rng.integers(0, 9)), replace=False)
        if r < CB:
            t = np.union1d(t, [COMMON])
        if r == CB - 1:
            t = np.union1d(t, [5])  # the last row of tile 0 holds term 5
        t = np.sort(t).astype(np.int32)
        v = rng.uniform(0.05, 1.0, t.size)
        if signed:
            v *= rng.choice([-1.0, 1.0], t.size)
        rows.append((t, v))
    rows[3] = (np.array([2, COMMON, 9], np.int32), np.array([1e-9, 0.5, -1e-9]))  # below fp16's range: bits 1 and 0x8000, never the zero word
    rp = np.concatenate([[0], np.cumsum([t.size for t, _ in rows])]).astype(np.int64)
    return Store(rp, np.concatenate([t for t, _ in rows]).astype(np.int32),
                 np.concatenate([v for _, v in rows]).astype(np.float32), np.arange(ROWS, dtype=np.int64), None)


def _ref(form, sub=None, signed=True):
    return iv.reference_index(_store(signed), CB, ROWS, form, sub=sub, dim=DIM)


def _copy(g):
    return g._replace(seg=g.seg.copy(), base=g.base.copy(), post=g.post.copy(),
                      tile_min=None if g.tile_min is None else g.tile_min.copy())


def _at(g, T, t):
    """absolute position of the first posting and the length of segment (T, t)"""
    return int(g.base[T] + g.seg[T, t, 0]), int(g.seg[T, t, 1])


def _rejects(g, ref, pattern, where=None):
    with pytest.raises(AssertionError) as e:
        iv.assert_index_equal(g, ref)
    msg = str(e.value)
    assert re.search(pattern, msg), msg
    if where is not None:
        m = re.search(r"tile (\d+)(?: term (\d+))?(?: posting (\d+))?", msg)
        assert m and tuple(int(x) for x in m.groups() if x is not None) == tuple(where), (msg, where)
    return msg


@pytest.mark.parametrize("form", ["exact", "slot2", "plain", "wide"])
def test_a_rendered_reference_is_accepted(form):
    ref = _ref(form, signed=form != "wide")
    for rng in (None, np.random.default_rng(1)):
        assert iv.assert_index_equal(iv.render(ref, ALIGN[form], rng), ref) == 0
    cnt = iv.reference_counts(ref)
    assert cnt[0, COMMON] == CB and cnt.shape == (3, DIM) and (cnt == 0).any()


def test_expected_weight_bits():
    w = np.array([1.0, -1.0, 1e-9, -1e-9, 0.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 6e-8, 65504.0], np.float32)
    # round to nearest EVEN at the two ties; below the range: the smallest subnormal for +, the bare sign for - (never zero)
    assert iv.weight_bits(w, "slot2").tolist() == [0x3c00, 0xbc00, 1, 0x8000, 1, 0x3c00, 0x3c02, 1, 0x7bff]
    assert iv.weight_bits(w, "wide").tolist() == [0x3c00, 0x3c00, 1, 1, 1, 0x3c00, 0x3c02, 1, 0x7bff]
    assert iv.weight_bits(w, "exact").tolist() == w.view(np.uint32).tolist()
    ref = _ref("slot2")
    tiny = (ref.row == 3) & (ref.key % DIM != COMMON)
    assert sorted(ref.bits[tiny].tolist()) == [1, 0x8000]
    for form in ("slot2", "plain", "wide"):
        slot = np.array([0, 1, 63, 32767 if form == "slot2" else 65535], np.uint32)
        bits = np.array([1, 0x3c00, 0x7bff, 0x0400], np.uint32)
        words = (slot << 15 | bits) if form == "wide" else ((slot << 1 if form == "slot2" else slot) | bits << 16)
        s, b = iv.decode(words, form)
        assert s.tolist() == slot.tolist() and b.tolist() == bits.tolist()


def _seg_with(g, T, lo, hi, not_full=False, after=-1):
    """a term of tile T behind `after` whose segment holds lo .. hi postings (and, not_full, padding behind them)"""
    for t in range(after + 1, DIM):
        n = int(g.seg[T, t, 1])
        if lo <= n <= hi and (not not_full or n % g.align):
            return t
    raise AssertionError("no such segment")


def test_dropped_and_duplicated_postings_are_located():
    ref = _ref("slot2")
    good = iv.render(ref, 32)
    t = _seg_with(good, 1, 2, 31)
    p, n = _at(good, 1, t)
    g = _copy(good)
    g.post[p + n - 1] = 0
    g.seg[1, t, 1] = n - 1  # (the count adjusted to match)
    _rejects(g, ref, r"segment length %d, reference %d" % (n - 1, n), (1, t))
    g = _copy(good)
    g.post[p + n] = g.post[p + n - 1]
    g.seg[1, t, 1] = n + 1
    _rejects(g, ref, r"segment length %d, reference %d" % (n + 1, n), (1, t))
    g = _copy(good)  # ... and with the count left alone: the multiset differs
    g.post[p + 1] = g.post[p]
    _rejects(g, ref, r"posting 1 of the sorted segment", (1, t, 1))


def test_swapped_slots_are_located():
    ref = _ref("slot2")
    good = iv.render(ref, 32)
    t = _seg_with(good, 0, 2, 31)
    p, _ = _at(good, 0, t)
    g = _copy(good)
    a, b = int(g.post[p]), int(g.post[p + 1])
    assert a >> 16 != b >> 16
    g.post[p], g.post[p + 1] = (a & 0xffff0000) | (b & 0xffff), (b & 0xffff0000) | (a & 0xffff)
    _rejects(g, ref, r"weight bits", (0, t, 0))


def test_posting_moved_to_the_neighbouring_term_or_tile_is_located():
    ref = _ref("slot2")
    good = iv.render(ref, 32)
    t = next(t for t in range(DIM - 1) if 1 <= good.seg[2, t, 1] < 31 and good.seg[2, t + 1, 1] % 32 not in (0, 31))
    g = _copy(good)
    (p, n), (p1, n1) = _at(g, 2, t), _at(g, 2, t + 1)
    g.post[p1 + n1], g.post[p + n - 1] = g.post[p + n - 1], 0
    g.seg[2, t, 1], g.seg[2, t + 1, 1] = n - 1, n1 + 1
    _rejects(g, ref, r"segment length %d, reference %d" % (n - 1, n), (2, t))
    # the last row of tile 0 (slot 63) holds term 5; its posting lands in tile 1 as slot 0
    g = _copy(good)
    (p, n), (p1, n1) = _at(g, 0, 5), _at(g, 1, 5)
    assert n1 % 32 not in (0, 31)
    words = g.post[p:p + n]
    i = int(np.nonzero((words & 0xffff) >> 1 == CB - 1)[0][0])
    moved = int(words[i]) & 0xffff0000
    g.post[p + i] = g.post[p + n - 1]
    g.post[p + n - 1] = 0
    g.post[p1 + n1] = moved
    g.seg[0, 5, 1], g.seg[1, 5, 1] = n - 1, n1 + 1
    _rejects(g, ref, r"segment length %d, reference %d" % (n - 1, n), (0, 5))
    g = _copy(good)  # the same slip with the row kept in its tile but numbered as in the next one: slot 63 -> 0
    g.post[p + i] = moved
    _rejects(g, ref, r"slot 0, weight bits", (0, 5, 0))


@pytest.mark.parametrize("step", [+1, -1])
def test_weight_off_by_one_fp16_ulp_is_located(step):
    ref = _ref("slot2")
    good = iv.render(ref, 32)
    t = _seg_with(good, 1, 1, 31)
    p, _ = _at(good, 1, t)
    g = _copy(good)
    g.post[p] = int(g.post[p]) + step * (1 << 16)
    _rejects(g, ref, r"weight bits", (1, t, 0))
    ref = _ref("exact")  # one fp32 ulp in the exact rendering
    good = iv.render(ref, 16)
    g = _copy(good)
    p, _ = _at(good, 1, t)
    g.post[p, 1] = int(g.post[p, 1]) + step
    _rejects(g, ref, r"weight bits", (1, t, 0))


def test_zero_word_lost_sign_and_padding_are_located():
    ref = _ref("slot2")
    good = iv.render(ref, 32)
    t = _seg_with(good, 1, 2, 31)
    p, n = _at(good, 1, t)
    g = _copy(good)
    g.post[p + 1] = 0  # a weight flushed to zero in slot 0 would be this word
    _rejects(g, ref, r"the zero word", (1, t, 1))
    neg = np.nonzero(good.post & 0x80000000)[0]
    assert neg.size
    g = _copy(good)
    g.post[neg[0]] &= 0x7fffffff
    msg = _rejects(g, ref, r"weight bits")
    m = re.search(r"bits 0x([0-9a-f]+)\), reference \(slot \d+ = row \d+, weight bits 0x([0-9a-f]+)", msg)
    assert int(m.group(1), 16) | 0x8000 == int(m.group(2), 16)
    g = _copy(good)
    g.post[p + n] = 0x3c000002
    _rejects(g, ref, r"padding word 0 behind the segment's %d postings" % n, (1, t))
    g = _copy(good)
    g.post[p + 31] = 1  # the last word of the aligned unit
    _rejects(g, ref, r"padding word %d" % (31 - n), (1, t))


def test_layout_faults_are_located():
    ref = _ref("slot2")
    good = iv.render(ref, 32)
    t = _seg_with(good, 1, 1, 31)
    g = _copy(good)
    g.seg[1, t, 0] += 1
    _rejects(g, ref, r"segment start \d+ is not a multiple of 32", (1, t))
    t2 = _seg_with(good, 1, 1, 31, after=t)
    g = _copy(good)
    g.seg[1, t2, 0] = g.seg[1, t, 0]
    _rejects(g, ref, r"the extents of term %d \[\d+, \d+\) and term %d \[\d+, \d+\) overlap" % (t, t2), (1,))
    g = _copy(good)  # the two-unit segment of the common term reaching into its neighbour
    g.seg[0, COMMON, 0] -= 32
    _rejects(g, ref, r"overlap", (0,))
    g = _copy(good)
    g.base[1] += 32
    _rejects(g, ref, r"base\[1\] - base\[0\]", (0,))
    g = _copy(good)
    g.base[3] += 32
    _rejects(g, ref, r"base\[3\] - base\[2\]", (2,))
    _rejects(good._replace(post_used=good.post_used + 32, post=np.concatenate([good.post, np.zeros(32, np.uint32)])), ref,
             r"base\[3\] = \d+, post_used")


def test_statistics_are_checked():
    ref = _ref("slot2")
    good = iv.render(ref, 32)
    assert good.max_seg == CB
    _rejects(good._replace(max_seg=CB - 1), ref, r"max_seg is 63, the longest segment of the reference holds 64 \(tile 0 term %d\)" % COMMON)
    _rejects(good._replace(long_segs=1), ref, r"long_segs is 1, expected 0")
    iv.assert_index_equal(good._replace(long_segs=1), ref, long_segs=1)
    iv.assert_index_equal(good._replace(long_segs=5), ref, long_segs=None)
    _rejects(good._replace(cb=128), ref, r"rows per tile")


def test_scaled_weights_band_and_tile_min():
    rng = np.random.default_rng(9)
    sub = rng.uniform(0.3, 1.0, ROWS).astype(np.float32)
    sub[rng.choice(ROWS, 10, replace=False)] = 0.0  # rows without weight in the range: stored as they are
    ref = _ref("slot2", sub=sub)
    assert ref.scaled and ref.alt.shape == (3, ref.bits.size)
    share = iv.excused_share(ref)
    assert share < 0.005, share
    zero = sub[ref.row] == 0
    assert zero.any() and (ref.alt[0][zero] == ref.alt[2][zero]).all()
    good = iv.render(ref, 32, sub=sub)
    assert iv.assert_index_equal(good, ref) == 0
    # the band: the roundings of q (1 -+ d) pass where they differ, one fp16 ulp beyond does not
    widened = ref._replace(alt=np.stack([ref.bits - 1, ref.bits, ref.bits + 1]))
    lo = iv.render(ref._replace(bits=ref.bits - 1), 32, sub=sub)
    assert iv.assert_index_equal(lo, widened) == ref.bits.size
    t = _seg_with(good, 1, 1, 31)
    _rejects(lo, ref, r"band 0x[0-9a-f]+ \.\. 0x[0-9a-f]+")
    # tile_min: taken over the wrong tile
    assert ref.tile_min.shape == (3,) and len(set(ref.tile_min.tolist())) == 3
    for T in range(3):
        part = sub[T * CB:(T + 1) * CB]
        assert ref.tile_min[T] == part[part > 0].min()
    g = _copy(good)
    g.tile_min[1] = g.tile_min[2]
    _rejects(g, ref, r"tile_min", (1,))
    _rejects(good._replace(tile_min=None), ref, r"carries no tile_min")
    _rejects(good._replace(scaled=False), ref, r"weights_scaled")
    assert t >= 0


def test_shard_factor_reference_and_bound():
    rng = np.random.default_rng(2)
    lens = np.array([0, 1, 16, 17, 700])
    rp = np.concatenate([[0], np.cumsum(lens)])
    idx = np.concatenate([np.sort(rng.choice(1000, n, replace=False)) for n in lens]).astype(np.int32)
    val = rng.uniform(0.1, 1.0, idx.size)
    want = iv.reference_sub(rp, idx, val, (200, 600))
    assert want[0] == 0.0 and (want[1:] <= iv.HAIR).all()
    r = 4
    ins = (idx[rp[r]:] >= 200) & (idx[rp[r]:] < 600)
    v32 = val[rp[r]:].astype(np.float32).astype(np.float64)
    assert abs(want[r] - np.sqrt((v32[ins] ** 2).sum() / (v32 ** 2).sum()) * iv.HAIR) < 1e-15
    tol = iv.sub_rel_tol(lens)
    assert tol[1] == 6.5 * 2.0 ** -23 and tol[4] == ((44 + 4 + 1) / 2 + 3.5) * 2.0 ** -23
    assert iv.assert_sub_close(want.astype(np.float32), rp, idx, val, (200, 600)) <= 1.0
    off = want.astype(np.float32)
    off[4] = np.float32(off[4] * (1 + 40 * 2.0 ** -23))
    with pytest.raises(AssertionError, match="row 4: sub"):
        iv.assert_sub_close(off, rp, idx, val, (200, 600))
    # the undocumented ratio (without the hair) is outside the bound for a short row
    off = want.astype(np.float32)
    off[2] = np.float32(want[2] / iv.HAIR)
    with pytest.raises(AssertionError, match="row 2: sub"):
        iv.assert_sub_close(off, rp, idx, val, (200, 600))
