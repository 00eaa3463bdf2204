"""What the index build left in HBM, read back posting by posting, and the same posting lists restated in numpy.

read_index(ix, rendering)   one built rendering (apss_index_view_get) copied to the host: segment table, tile bases, postings,
                            shard factors, per-tile minima, the statistics the probe was told
reference_index(...)        the posting lists of the store AS THE DEVICE HOLDS IT (store_view.read_store), per (tile, term) the
                            multiset of (slot, expected weight bits)
assert_index_equal(...)     every invariant the probe kernels lean on, the message naming the first offending tile, term, posting
excused_share(ref)          share of the scaled postings whose three admissible roundings differ (from the reference alone)
reference_sub / sub_rel_tol the shard factor |x_g| / |x| in float64 and its derived bound

Expected weight bits.  Exact rendering: the stored fp32 bits.  Coarse renderings: max(bits(float16 round-to-nearest-even of w), 1)
with the sign kept (pack_coarse), the wide form the same with the sign bit cleared (pack_coarse_wide).  Unscaled weights get no
band at all.  Where the weights are stored divided by sub[row] (shard rule; w = val where sub <= 0) the quotient is ONE fp32
division on the device, which HIP documents to 2.5 ulp when it is not correctly rounded: the float64 quotient q of the read-back
bits is taken and the float16 rounding of q (1 - d), q or q (1 + d), d = 3 * 2^-23, is accepted -- the fp32 quotient lies in
[q (1 - d), q (1 + d)], float16 rounding is monotone, and the two ends round to the same or to neighbouring numbers.  That is
a cap, not a licence: the three roundings differ only where q lies within d of a float16 rounding boundary, an expected share
of d / 2^-11 = 0.07 % of the postings; the tests assert the share (excused_share) under 0.5 %.

The shard factor.  k_ingest_count leaves sub[row] = min(1, sqrtf(sub2 / full2)) * 0.999999f: |x_g| / |x| rounded DOWN a hair on
purpose (as a threshold factor and as a weight divisor it then errs on the side of reporting more).  The comparison is against
float64 |x_g| / |x| of the test's whole input rows times that documented constant (its fp32 value), inside the relative bound
(inputs exact in fp32, u = 2^-24, D = ceil(nnz / 16) + 4 the addition chain of a 16-lane row sum, as in store_view):
  * two sums of squares, each <= (D + 1) u, halved by the square root: (D + 1) / 4 * 2^-23 each
  * two square roots and one division, 2^-23 each (not promised to round correctly; the device takes one root of the quotient,
    which errs no more)
  * the product with the constant rounds once: 2^-24
  sum: ((D + 1) / 2 + 3.5) * 2^-23 =: sub_rel_tol.  nnz <= 16: D = 5, 6.5 * 2^-23 = 7.7e-7; nnz = 2,247: D = 145, 9.1e-6."""
import collections
import ctypes as C

import numpy as np

from apss import _lib
from store_view import _to_host

Index = collections.namedtuple(
    "Index", "form cb align dim n_tiles built_rows post_used scaled seg base post sub tile_min max_seg long_segs chunk_weight")
# form "exact" | "slot2" | "plain" | "wide"; seg uint32 [n_tiles, dim, 2] = {start, length}; base int64 [n_tiles + 1];
# post uint32 [post_used, 2] = {slot, fp32 bits} (exact) or uint32 [post_used] (coarse words); sub float32 [built_rows] and
# tile_min float32 [n_tiles] of a handle that scales, else None

Reference = collections.namedtuple("Reference", "form cb dim n_tiles built_rows scaled key slot bits alt row tile_min")
# one entry per posting, sorted by (tile, term, slot): key = tile * dim + term, slot = row - tile * cb, bits = expected weight
# bits; alt uint32 [3, n] = the admissible bits of a scaled weight (rounding of q (1 - d), q, q (1 + d)) or None; row = store
# row; tile_min float32 [n_tiles] expected per-tile minimum of the positive sub, or None

LONG_LEN = 256  # kLongLenW: what the probe kernels sweep as a long segment
DELTA = 3.0 * 2.0 ** -23
FORMS = {(0, _lib.SLOT_PLAIN): "exact", (1, _lib.SLOT_TIMES2): "slot2", (1, _lib.SLOT_PLAIN): "plain", (1, _lib.SLOT_WIDE): "wide"}


def index_view(ix, rendering):
    v = _lib.IndexView()
    v.struct_size = C.sizeof(_lib.IndexView)
    assert ix._L.apss_index_view_get(ix._h, rendering, C.byref(v)) == _lib.OK
    assert v.struct_size == C.sizeof(_lib.IndexView) and v.rendering == rendering
    return v


def read_index(ix, rendering):
    """every library call has synchronised before it returned: plain blocking copies are enough.  None: not built."""
    v = index_view(ix, rendering)
    if v.n_tiles == 0:
        assert not (v.d_seg or v.d_base or v.d_post or v.d_sub or v.d_tile_min) and v.built_rows == 0 and v.post_used == 0
        return None
    form = FORMS[(rendering, v.slot_form)]
    assert v.posting_bytes == (8 if form == "exact" else 4)
    seg = _to_host(v.d_seg, v.n_tiles * v.dim * 2, np.uint32).reshape(v.n_tiles, v.dim, 2)
    base = _to_host(v.d_base, v.n_tiles + 1, np.int64)
    post = _to_host(v.d_post, v.post_used * (2 if form == "exact" else 1), np.uint32)
    if form == "exact":
        post = post.reshape(-1, 2)
    sub = _to_host(v.d_sub, v.built_rows, np.float32) if v.d_sub else None
    tile_min = _to_host(v.d_tile_min, v.n_tiles, np.float32) if v.d_tile_min else None
    return Index(form, v.tile_rows, v.seg_align, v.dim, v.n_tiles, v.built_rows, v.post_used, bool(v.weights_scaled), seg, base,
                 post, sub, tile_min, v.max_seg, v.long_segs, v.chunk_weight)


def weight_bits(w, form):
    """expected weight bits of float64 (or float32) weights in a rendering's form"""
    if form == "exact":
        return np.asarray(w, np.float32).view(np.uint32).copy()
    with np.errstate(over="ignore"):
        h = np.asarray(w).astype(np.float16).view(np.uint16).astype(np.uint32)
    if form == "wide":
        h &= 0x7fff
    return np.maximum(h, 1).astype(np.uint32)


def reference_index(store, cb, built_rows, form, head_terms=None, sub=None, dim=None):
    """dim: terms per tile (the store does not know it; without it the keys stay (tile, term) until with_dim).
    store: the device's rows (read_store); built_rows: the rows the rendering covers; head_terms: the terms of a dense-head
    block (apss_get_head_terms), whose entries are not in the inverted index; sub: float32 per row as read back from the device
    when the weights are stored divided by it (coarse renderings of a handle that scales), else None"""
    rowptr = np.asarray(store.rowptr, np.int64)
    nnz = int(rowptr[built_rows])
    row = np.repeat(np.arange(built_rows, dtype=np.int64), np.diff(rowptr[:built_rows + 1]))
    term = np.asarray(store.indices[:nnz], np.int64)
    val = np.asarray(store.values[:nnz], np.float32)
    if head_terms is not None and len(head_terms):
        keep = ~np.isin(term, np.asarray(head_terms, np.int64))
        row, term, val = row[keep], term[keep], val[keep]
    tile = row // cb
    alt = None
    if sub is not None and form != "exact":
        s = np.asarray(sub, np.float32).astype(np.float64)[row]
        q = np.where(s > 0.0, val.astype(np.float64) / np.where(s > 0.0, s, 1.0), val.astype(np.float64))
        bits = weight_bits(q, form)
        alt = np.stack([weight_bits(q * (1.0 - DELTA), form), bits, weight_bits(q * (1.0 + DELTA), form)])
        alt[:, ~(s > 0.0)] = bits[~(s > 0.0)]  # (no division, no band)
    else:
        bits = weight_bits(val, form)
    n_tiles = -(-built_rows // cb)
    tile_min = None
    if sub is not None:
        s32 = np.asarray(sub, np.float32)[:built_rows]
        tile_min = np.zeros(n_tiles, np.float32)
        for t in range(n_tiles):
            part = s32[t * cb:(t + 1) * cb]
            part = part[part > 0]
            tile_min[t] = part.min() if part.size else 0.0
    ref = Reference(form, cb, None, n_tiles, built_rows, sub is not None and form != "exact", (tile, term), row - tile * cb, bits,
                    alt, row, tile_min)
    return ref if dim is None else with_dim(ref, dim)


def with_dim(ref, dim):
    """the reference with its (tile, term) keys flattened and its postings sorted by (tile, term, slot)"""
    tile, term = ref.key
    assert term.size == 0 or (term.min() >= 0 and term.max() < dim)
    key = tile * dim + term
    o = np.lexsort((ref.slot, key))
    return ref._replace(dim=dim, key=key[o], slot=ref.slot[o].astype(np.uint32), bits=ref.bits[o],
                        alt=None if ref.alt is None else ref.alt[:, o], row=ref.row[o])


def excused_share(ref):
    """share of the postings whose admissible roundings differ: what assert_index_equal could excuse, from the reference alone"""
    if ref.alt is None or ref.bits.size == 0:
        return 0.0
    return float(np.mean((ref.alt[0] != ref.alt[1]) | (ref.alt[2] != ref.alt[1])))


def reference_counts(ref):
    """uint32 [n_tiles, dim]: postings per (tile, term)"""
    return np.bincount(ref.key, minlength=ref.n_tiles * ref.dim).astype(np.int64).reshape(ref.n_tiles, ref.dim)


def decode(words, form):
    """(slot, weight bits) of coarse posting words"""
    words = np.asarray(words, np.uint32)
    if form == "wide":
        return words >> 15, words & 0x7fff
    slot = words & 0xffff
    return (slot >> 1 if form == "slot2" else slot), words >> 16


def _fail(fmt, *a):
    raise AssertionError(fmt % a)


def assert_index_equal(got, want, long_segs="exact"):
    """got: Index (read_index, or rendered by a test); want: Reference (with_dim applied).  long_segs: "exact" (a rendering built
    whole from tile 0), an int (what the build promises otherwise), or None (not checked).  Returns the number of postings whose
    bits differed from the central rounding inside the band (0 for unscaled weights)."""
    assert want.dim is not None, "with_dim() first"
    if (got.form, got.cb, got.dim, got.n_tiles, got.built_rows) != (want.form, want.cb, want.dim, want.n_tiles, want.built_rows):
        _fail("rendering is (%s, %d rows per tile, dim %d, %d tiles, %d rows), reference (%s, %d, %d, %d, %d)", got.form, got.cb,
              got.dim, got.n_tiles, got.built_rows, want.form, want.cb, want.dim, want.n_tiles, want.built_rows)
    if got.scaled != want.scaled:
        _fail("rendering says weights_scaled = %s, reference %s", got.scaled, want.scaled)
    coarse = got.form != "exact"
    T, dim, al = got.n_tiles, got.dim, int(got.align)
    assert got.seg.shape == (T, dim, 2) and got.base.shape == (T + 1,) and got.post.shape[0] == got.post_used
    start, length = got.seg[:, :, 0].astype(np.int64), got.seg[:, :, 1].astype(np.int64)
    cnt = reference_counts(want)
    # 1. lengths, every term of every tile (terms without a posting and terms outside a shard's range: 0)
    bad = np.argwhere(length != cnt)
    if bad.size:
        t, k = bad[0]
        _fail("tile %d term %d: segment length %d, reference %d", t, k, length[t, k], cnt[t, k])
    # 2. starts on the alignment
    bad = np.argwhere(start % al != 0)
    if bad.size:
        t, k = bad[0]
        _fail("tile %d term %d: segment start %d is not a multiple of %d", t, k, start[t, k], al)
    # 3. aligned extents pairwise disjoint and inside the tile; 4. tile bases
    ext = -(-length // al) * al
    if got.base[0] != 0:
        _fail("base[0] is %d", got.base[0])
    for t in range(T):
        total = int(got.base[t + 1] - got.base[t])
        if total != int(ext[t].sum()):
            _fail("tile %d: base[%d] - base[%d] = %d, the aligned segments need %d", t, t + 1, t, total, int(ext[t].sum()))
        ks = np.nonzero(length[t])[0]
        ks = ks[np.argsort(start[t, ks], kind="stable")]
        end = start[t, ks] + ext[t, ks]
        over = np.nonzero(end[:-1] > start[t, ks[1:]])[0]
        if over.size:
            i = int(over[0])
            _fail("tile %d: the extents of term %d [%d, %d) and term %d [%d, %d) overlap", t, ks[i], start[t, ks[i]], end[i],
                  ks[i + 1], start[t, ks[i + 1]], end[i + 1])
        if ks.size and end[-1] > total:
            _fail("tile %d term %d: extent [%d, %d) ends behind the tile's %d postings", t, ks[-1], start[t, ks[-1]], end[-1], total)
    if got.base[T] != got.post_used:
        _fail("base[%d] = %d, post_used = %d", T, got.base[T], got.post_used)
    # 5. the postings of every segment, as sorted multisets (order inside a segment is free)
    flat_len = length.reshape(-1)
    keys = np.nonzero(flat_len)[0]  # ascending (tile, term): the reference's order
    lens = flat_len[keys]
    first = np.cumsum(lens) - lens
    n = int(lens.sum())
    seg_of = np.repeat(np.arange(keys.size), lens)
    within = np.arange(n, dtype=np.int64) - first[seg_of]
    pos = (got.base[:-1, None] + start).reshape(-1)[keys][seg_of] + within

    def where(i):  # (tile, term, position in the segment) of gathered posting i
        k = int(keys[seg_of[i]])
        return k // dim, k % dim, int(within[i])

    if coarse:
        words = got.post[pos]
        zero = np.nonzero(words == 0)[0]
        if zero.size:
            _fail("tile %d term %d posting %d: the zero word (it marks padding: a posting must never be zero)", *where(int(zero[0])))
        g_slot, g_bits = decode(words, got.form)
    else:
        g_slot, g_bits = got.post[pos, 0], got.post[pos, 1]
    o = np.lexsort((g_bits, g_slot, seg_of))
    g_slot, g_bits = g_slot[o], g_bits[o]
    assert want.key.size == n and np.array_equal(np.repeat(keys, lens), want.key)
    ok_bits = g_bits == want.bits if want.alt is None else (g_bits == want.alt[0]) | (g_bits == want.alt[1]) | (g_bits == want.alt[2])
    bad = np.nonzero((g_slot != want.slot) | ~ok_bits)[0]
    if bad.size:
        i = int(bad[0])
        t, k, _ = where(i)
        _fail("tile %d term %d posting %d of the sorted segment: (slot %d, weight bits 0x%x), reference (slot %d = row %d, weight bits "
              "0x%x%s)", t, k, i - int(first[seg_of[i]]), g_slot[i], g_bits[i], want.slot[i], want.row[i], want.bits[i],
              "" if want.alt is None else ", band 0x%x .. 0x%x" % (want.alt[0][i], want.alt[2][i]))
    # 6. coarse: every word of an aligned extent behind the segment's length is zero
    if coarse:
        pad = (ext.reshape(-1)[keys] - lens)
        pseg = np.repeat(np.arange(keys.size), pad)
        pw = np.arange(int(pad.sum()), dtype=np.int64) - (np.cumsum(pad) - pad)[pseg]
        ppos = (got.base[:-1, None] + start).reshape(-1)[keys][pseg] + lens[pseg] + pw
        nz = np.nonzero(got.post[ppos] != 0)[0]
        if nz.size:
            i = int(nz[0])
            k = int(keys[pseg[i]])
            _fail("tile %d term %d: padding word %d behind the segment's %d postings is 0x%x, not zero", k // dim, k % dim, int(pw[i]),
                  lens[pseg[i]], got.post[ppos[i]])
    # 7. what the probe was told
    longest = int(cnt.max()) if cnt.size else 0
    if got.max_seg != longest:
        _fail("max_seg is %d, the longest segment of the reference holds %d (tile %d term %d)", got.max_seg, longest,
              *np.unravel_index(int(np.argmax(cnt)), cnt.shape))
    if long_segs is not None:
        expect = int((cnt > LONG_LEN).sum()) if long_segs == "exact" else int(long_segs)
        if got.long_segs != expect:
            _fail("long_segs is %d, expected %d (the reference holds %d segments of more than %d postings)", got.long_segs, expect,
                  int((cnt > LONG_LEN).sum()), LONG_LEN)
    # 8. shard rule: the per-tile minimum of the positive factors, bit for bit
    if want.tile_min is not None:
        if got.tile_min is None:
            _fail("the rendering carries no tile_min, the reference does")
        bad = np.nonzero(got.tile_min.view(np.uint32) != want.tile_min.view(np.uint32))[0]
        if bad.size:
            t = int(bad[0])
            _fail("tile %d: tile_min %r, the smallest positive sub of its rows is %r", t, float(got.tile_min[t]), float(want.tile_min[t]))
    return 0 if want.alt is None else int(np.sum(g_bits != want.alt[1]))


def segment_counts(ref):
    """the reference's segment lengths as a flat array (for tests that assert which lengths an input reaches)"""
    return np.bincount(ref.key, minlength=ref.n_tiles * ref.dim)


def render(ref, align, rng=None, sub=None):
    """a Reference rendered into the device layout (tests of the comparer): segments laid out in term order, postings of a
    segment shuffled when an rng is given"""
    cnt = reference_counts(ref)
    ext = -(-cnt // align) * align
    start = np.cumsum(ext, axis=1) - ext
    base = np.concatenate([[0], np.cumsum(ext.sum(axis=1))]).astype(np.int64)
    seg = np.stack([start, cnt], axis=2).astype(np.uint32)
    coarse = ref.form != "exact"
    post = np.zeros(int(base[-1]) if coarse else (int(base[-1]), 2), np.uint32)
    keys, lens = np.unique(ref.key, return_counts=True)
    first = np.cumsum(lens) - lens
    seg_of = np.repeat(np.arange(keys.size), lens)
    within = np.arange(ref.key.size) - first[seg_of]
    if rng is not None:
        for i in range(keys.size):
            within[first[i]:first[i] + lens[i]] = rng.permutation(int(lens[i]))
    pos = (base[:-1, None] + start).reshape(-1)[keys][seg_of] + within
    if ref.form == "exact":
        post[pos, 0], post[pos, 1] = ref.slot, ref.bits
    elif ref.form == "wide":
        post[pos] = (ref.slot << 15) | ref.bits
    else:
        post[pos] = (ref.slot << 1 if ref.form == "slot2" else ref.slot) | (ref.bits << 16)
    return Index(ref.form, ref.cb, align, ref.dim, ref.n_tiles, ref.built_rows, int(base[-1]), ref.scaled, seg, base, post,
                 None if sub is None else np.asarray(sub, np.float32), None if ref.tile_min is None else ref.tile_min.copy(),
                 int(cnt.max()), int((cnt > LONG_LEN).sum()), 0.0)


# ---- the shard factor ----
HAIR = float(np.float32(0.999999))  # k_ingest_count rounds the factor down by this constant (module docstring)


def sub_rel_tol(src_nnz):
    """((D + 1) / 2 + 3.5) * 2^-23 with D = ceil(nnz / 16) + 4 (module docstring), per row"""
    d = -(-np.asarray(src_nnz, np.int64) // 16) + 4
    return ((d + 1) / 2.0 + 3.5) * 2.0 ** -23


def reference_sub(rowptr, indices, values, term_range):
    """float64 min(1, |x_g| / |x|) * HAIR of whole input rows (values as the device is handed them: fp32), x_g the row's entries
    in [lo, hi); 0 for a row without weight"""
    rowptr = np.asarray(rowptr, np.int64)
    v = np.asarray(values, np.float32).astype(np.float64)
    sq = v * v
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    ins = (np.asarray(indices) >= term_range[0]) & (np.asarray(indices) < term_range[1])
    full = np.bincount(rows, sq, minlength=rowptr.size - 1)
    part = np.bincount(rows[ins], sq[ins], minlength=rowptr.size - 1)
    return np.where(full > 0, np.minimum(1.0, np.sqrt(part) / np.sqrt(np.where(full > 0, full, 1.0))) * HAIR, 0.0)


def assert_sub_close(got_sub, rowptr, indices, values, term_range):
    """every row's factor inside its bound of the float64 reference; returns the worst error in units of its bound"""
    want = reference_sub(rowptr, indices, values, term_range)
    tol = sub_rel_tol(np.diff(np.asarray(rowptr, np.int64)))
    got = np.asarray(got_sub, np.float32).astype(np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    err = np.abs(got - want)
    bad = np.nonzero(~(err <= tol * want))[0]
    if bad.size:
        r = int(bad[0])
        _fail("row %d: sub %r, reference %r: relative error %.3g * 2^-23 > bound %.3g * 2^-23", r, got[r], want[r],
              err[r] / want[r] * 2.0 ** 23 if want[r] else float("inf"), tol[r] * 2.0 ** 23)
    pos = want > 0
    return float(np.max(err[pos] / (tol[pos] * want[pos]))) if pos.any() else 0.0
