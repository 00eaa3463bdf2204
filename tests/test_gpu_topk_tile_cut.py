"""The per-round cut inside the theta <= 0 probe kernel (apss_set_top_k_tile_cut, DESIGN.md 5e "Cut inside the probe").

Exact list equality: the device lists (query row, candidate slot, score) of two calls compare equal as int32, int32 and float
BITS.  predict() is this file's numpy restatement of the rule -- a round is (query row, candidate slot // tile_rows); a round
with more than k pairs emits those whose score key is >= the top 16 bits of its k-th largest key -- applied to the k = 0 device
list of the same call, which is code the setting does not touch.  On the fixed-point path the scores of a call are
reproducible bit for bit, so pairs_emitted == predict(...) and rounds_cut are exact assertions."""
import numpy as np
import pytest

from apss import _lib, synth
from apss.engine import ApssError, ApssIndex
from test_gpu_topk import LOWER, check_topk

pytestmark = pytest.mark.gpu

FIVE = ("k", "pairs_over_theta", "kept", "queries_cut", "longest_segment")


def device_list(ix):
    import torch
    _, _, _, n = ix.results_dev()
    q = torch.empty(n, dtype=torch.int32, device="cuda")
    c = torch.empty(n, dtype=torch.int32, device="cuda")
    s = torch.empty(n, dtype=torch.float32, device="cuda")
    if n:
        ix.results_to(q, c, s)
    torch.cuda.synchronize()
    return q.cpu().numpy(), c.cpu().numpy(), s.cpu().numpy()


def same_list(a, b):
    return (len(a[0]) == len(b[0]) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and
            np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)))


def topk_key(s):
    b = np.ascontiguousarray(s, dtype=np.float32).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    neg = (b & 0x80000000) != 0
    return np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def predict(list0, k, tile_rows):
    """(pairs the cut probe emits, rounds it cuts) for the uncut list `list0` of the same call"""
    q, c, s = list0
    if len(q) == 0:
        return 0, 0
    key = topk_key(s).astype(np.int64)
    g = q.astype(np.int64) * (1 << 32) + c.astype(np.int64) // tile_rows
    order = np.lexsort((-key, g))
    g, key = g[order], key[order]
    first = np.flatnonzero(np.concatenate([[True], g[1:] != g[:-1]]))
    size = np.diff(np.concatenate([first, [len(g)]]))
    cut = size > k
    kth = key[np.minimum(first + k - 1, len(g) - 1)]
    floor = np.where(cut, kth & ~np.int64(0xffff), np.int64(0))  # a round of at most k pairs emits all of them
    emitted = key >= np.repeat(floor, size)
    return int(emitted.sum()), int(cut.sum())


def run(dim, theta, tile_rows, k, cut, calls, window=0):
    """calls: [(method name, ids, rp, idx, val), ...]; the device list, infos and stats after the last one"""
    with ApssIndex(dim, theta, tile_rows=tile_rows, top_k=k, top_k_window=window, top_k_tile_cut=cut) as ix:
        for name, ids, rp, idx, val in calls:
            getattr(ix, name)(ids, rp, idx, val)
        return dict(lst=device_list(ix), got=ix.fetch(), info=ix.topk_info(), cut=ix.topk_tile_cut_info(), st=ix.stats(),
                    win=ix.topk_window_info(), cuts=ix.topk_window_cuts())


def check_on_off(dim, theta, tile_rows, k, calls, kernel):
    """the call with the cut off, on, and at k = 0: same list, same five info fields, the prediction"""
    off = run(dim, theta, tile_rows, k, False, calls)
    on = run(dim, theta, tile_rows, k, True, calls)
    zero = run(dim, theta, tile_rows, 0, False, calls)
    want_emit, want_rounds = predict(zero["lst"], k, tile_rows)
    print("k=%d %s: emitted %d (predicted %d) of %d, rounds cut %d (predicted %d)" %
          (k, on["st"]["probe_kernel"], on["cut"]["pairs_emitted"], want_emit, on["info"]["pairs_over_theta"],
           on["cut"]["rounds_cut"], want_rounds))
    assert same_list(off["lst"], on["lst"])
    for f in FIVE:
        assert off["info"][f] == on["info"][f], f
    assert on["info"]["pairs_over_theta"] == len(zero["lst"][0])
    assert on["cut"]["applied"] == 1 and on["cut"]["declined"] == _lib.TILE_CUT_RAN and on["cut"]["prefix_bits"] == 16
    assert on["st"]["probe_kernel"] == kernel and off["st"]["probe_kernel"] == kernel.replace(", true>", ">")
    assert off["cut"]["applied"] == 0 and off["cut"]["declined"] == _lib.TILE_CUT_OFF
    assert off["cut"]["pairs_emitted"] == off["info"]["pairs_over_theta"] and off["cut"]["rounds_cut"] == 0
    assert on["cut"]["pairs_emitted"] == want_emit and on["cut"]["rounds_cut"] == want_rounds
    return off, on, zero


# ---- 1, 2. the theta = 0 shape of tests/test_gpu_topk.py: four 512-row tiles, 8000 rounds, every one cut
@pytest.fixture(scope="module")
def shape_zero(oracle):
    rp, idx, val = synth.make_vectors(2000, 64, 8, 0.0, seed=5, dup_frac=0.1)
    ids = np.arange(2000, dtype=np.int64)
    orc = oracle.selfjoin_pairs(64, 0.0 - LOWER, rp, idx, val)
    sign = np.where(np.random.Generator(np.random.PCG64(9)).random(val.size) < 0.5, -1.0, 1.0)
    orc_signed = oracle.selfjoin_pairs(64, -0.2 - LOWER, rp, idx, val * sign)
    return dict(rp=rp, idx=idx, val=val, ids=ids, orc=orc, val_signed=val * sign, orc_signed=orc_signed)


@pytest.mark.parametrize("k", [1, 8, 64])
def test_parity_and_prediction_theta_zero(shape_zero, k):
    z = shape_zero
    calls = [("insert_and_query", z["ids"], z["rp"], z["idx"], z["val"])]
    off, on, _ = check_on_off(64, 0.0, 512, k, calls, "k_probe<2, 512, true, true>")
    info = on["info"]
    assert (info["pairs_over_theta"], info["queries_cut"], info["longest_segment"], info["kept"]) == (2710116, 2000, 1431, 2000 * k)
    assert on["cut"]["rounds_cut"] == 8000
    assert on["cut"]["pairs_emitted"] < info["pairs_over_theta"]
    check_topk(on["got"], z["orc"], k, 0.0, z["ids"])


def test_signed_scores(shape_zero):
    z = shape_zero
    calls = [("insert_and_query", z["ids"], z["rp"], z["idx"], z["val_signed"])]
    off, on, zero = check_on_off(64, -0.2, 512, 8, calls, "k_probe<2, 512, true, true>")
    s0 = zero["lst"][2]
    assert (s0 < 0).any() and (s0 > 0).any()  # keys on both sides of zero
    assert on["cut"]["pairs_emitted"] < on["info"]["pairs_over_theta"]
    check_topk(on["got"], z["orc_signed"], 8, -0.2, z["ids"])


# ---- 3. round boundaries: one 64-row tile and a partial one of 10 rows, k = 4, theta = 0.  Five blocks of rows, each sharing
# ONE term of its own with a `hub` row of weight 1.0 (a pair's score is then the product of two weights, exact in fixed point);
# the other rows of tile 0 hold a term of their own each and meet nobody.
#   A  hub + 3 rows in tile 0, 4 rows in tile 1: the hub's rounds have k - 1 and k pairs, a tile-1 row's k and k - 1: none is cut
#   B  hub + 5 rows of weight 0.5 in tile 0: k + 1 pairs, all scores equal -> everything emitted, the round still counts as cut
#   C  hub + 0.75 x 3, 0.5 + 2^-12 (the k-th), 0.5 (the k + 1-th): one 16-bit prefix, different below it -> both emitted
#   D  hub + 0.75 x 3, 0.5 (the k-th), 0.125 (the k + 1-th): the first 8-bit digit differs -> the last one is cut
#   E  in tile 1: hub, a second row with the hub's vector AND external id, 4 rows of weights 0.75, 0.5, 0.125, 0.03125: the hub's
#      own row and its twin would be the two best candidates of the round; neither counts, so the round has exactly k pairs and
#      is not cut (counted, they would make it 6 and the floor would drop the two weakest rows from the final list)
# Rounds cut, by hand: every row of B, C and D sees the 5 others of its block in tile 0 (18 rounds); E's four plain rows see
# hub, twin and 3 others = 5 (4 rounds); hub and twin see 4; A's rounds have 3 or 4.  22.
def _boundary_store():
    rows = []  # (term, weight, ext id)
    nxt = [100]

    def add(term, w, ext=None):
        rows.append((term, w, nxt[0] if ext is None else ext))
        nxt[0] += 1
        return len(rows) - 1

    hub_a = add(0, 1.0)
    for w in (0.75, 0.5, 0.25):
        add(0, w)
    hub_b = add(1, 1.0)
    for _ in range(5):
        add(1, 0.5)
    hub_c = add(2, 1.0)
    for w in (0.75, 0.75, 0.75, 0.5 + 2.0 ** -12, 0.5):
        add(2, w)
    hub_d = add(3, 1.0)
    for w in (0.75, 0.75, 0.75, 0.5, 0.125):
        add(3, w)
    term = 5
    while len(rows) < 64:  # loners: a term of their own
        add(term, 1.0)
        term += 1
    for w in (0.875, 0.625, 0.375, 0.3125):  # A's rows of tile 1
        add(0, w)
    hub_e = add(4, 1.0, ext=7000)
    add(4, 1.0, ext=7000)
    for w in (0.75, 0.5, 0.125, 0.03125):
        add(4, w)
    assert len(rows) == 74 and term <= 64
    ids = np.array([r[2] for r in rows], dtype=np.int64)
    rp = np.arange(75, dtype=np.int64)
    idx = np.array([r[0] for r in rows], dtype=np.int32)
    val = np.array([r[1] for r in rows], dtype=np.float64)
    return ids, rp, idx, val, dict(a=hub_a, b=hub_b, c=hub_c, d=hub_d, e=hub_e)


def test_round_boundaries():
    ids, rp, idx, val, hub = _boundary_store()
    calls = [("insert_and_query", ids, rp, idx, val)]
    off, on, zero = check_on_off(64, 0.0, 64, 4, calls, "k_probe<2, 512, true, true>")
    q0, c0, s0 = zero["lst"]
    rounds = {}
    for q, c in zip(q0, c0):
        rounds[(int(q), int(c) // 64)] = rounds.get((int(q), int(c) // 64), 0) + 1
    assert (rounds[(hub["a"], 0)], rounds[(hub["a"], 1)]) == (3, 4)  # k - 1 and k
    assert rounds[(64, 0)] == 4 and rounds[(64, 1)] == 3             # a row of A in tile 1
    assert rounds[(hub["b"], 0)] == rounds[(hub["c"], 0)] == rounds[(hub["d"], 0)] == 5  # k + 1
    assert rounds[(hub["e"], 1)] == 4 and (hub["e"], 0) not in rounds  # the hub's own row and its twin do not count
    assert on["cut"]["rounds_cut"] == 22
    # what the rule leaves of the hubs' rounds, by hand: B all 5, C all 5, D 4; a round that is not cut keeps everything
    for h, want in (("b", 5), ("c", 5), ("d", 4)):
        mine = q0 == hub[h]
        emit, cut = predict((q0[mine], c0[mine], s0[mine]), 4, 64)
        assert (emit, cut) == (want, 1), (h, emit, cut)
    # the final list of E's hub: its four plain rows, best first
    q1, c1, s1 = on["lst"]
    assert list(s1[q1 == hub["e"]]) == [0.75, 0.5, 0.125, 0.03125]
    # rows with more than k pairs over both tiles: the 22 above and A's eight (3 + 4 each)
    assert on["info"]["queries_cut"] == 30 and on["info"]["pairs_over_theta"] == len(q0)


# ---- 4. call shapes, on the first 1000 rows of the shape of case 1 (tiles of 128 rows), k = 8
@pytest.fixture(scope="module")
def slice_zero(shape_zero):
    z = shape_zero
    n = 1000
    rp, idx, val = z["rp"][:n + 1], z["idx"][:z["rp"][n]], z["val"][:z["rp"][n]]

    def rows(a, b):
        return z["ids"][a:b] + 50000, rp[a:b + 1] - rp[a], idx[rp[a]:rp[b]], val[rp[a]:rp[b]]

    return rows


def test_batch_onto_a_store(slice_zero):
    calls = [("insert",) + slice_zero(0, 600), ("insert_and_query",) + slice_zero(600, 1000)]
    _, on, _ = check_on_off(64, 0.0, 128, 8, calls, "k_probe<2, 512, true, true>")
    assert 0 < on["cut"]["pairs_emitted"] < on["info"]["pairs_over_theta"]


def test_outside_batch(slice_zero):
    calls = [("insert",) + slice_zero(0, 600), ("query",) + slice_zero(600, 1000)]
    _, on, _ = check_on_off(64, 0.0, 128, 8, calls, "k_probe<2, 512, true, true>")
    assert 0 < on["cut"]["pairs_emitted"] < on["info"]["pairs_over_theta"]


def test_windows(slice_zero):
    calls = [("insert_and_query",) + slice_zero(0, 1000)]
    plain = run(64, 0.0, 128, 8, False, calls)
    zero = run(64, 0.0, 128, 0, False, calls)
    both = run(64, 0.0, 128, 8, True, calls, window=250000)
    assert both["win"]["windows"] >= 3 and len(both["cuts"]) == both["win"]["windows"] + 1
    assert same_list(plain["lst"], both["lst"])
    for f in FIVE:
        assert plain["info"][f] == both["info"][f], f
    q0, c0, s0 = zero["lst"]
    emit = rounds = 0
    for a, b in zip(both["cuts"][:-1], both["cuts"][1:]):
        mine = (q0 >= a) & (q0 < b)
        e, r = predict((q0[mine], c0[mine], s0[mine]), 8, 128)
        emit += e
        rounds += r
    assert both["cut"]["applied"] == 1
    assert (both["cut"]["pairs_emitted"], both["cut"]["rounds_cut"]) == (emit, rounds)
    assert 0 < both["win"]["pairs_window_max"] <= emit  # the emitted list is what a window held


def test_overflow_and_rerun_counts_once(slice_zero, monkeypatch):
    calls = [("insert_and_query",) + slice_zero(0, 1000)]
    roomy = run(64, 0.0, 128, 8, True, calls)
    monkeypatch.setenv("APSS_DEBUG", "res_cap=4096")
    tight = run(64, 0.0, 128, 8, True, calls)
    assert tight["st"]["probe_launches"] > roomy["st"]["probe_launches"]  # the hook did make the probe run again
    assert same_list(roomy["lst"], tight["lst"])
    for f in FIVE:
        assert roomy["info"][f] == tight["info"][f], f
    assert tight["cut"] == roomy["cut"]


# ---- 5. the 1024-thread instantiation: a 16384-row tile and a partial one
def test_block_1024():
    rp, idx, val = synth.make_vectors(17000, 2048, 8, 0.0, seed=3)
    ids = np.arange(17000, dtype=np.int64)
    calls = [("insert_and_query", ids, rp, idx, val)]
    _, on, zero = check_on_off(2048, 0.0, 16384, 8, calls, "k_probe<2, 1024, true, true>")
    assert len(zero["lst"][0]) > 8000000 and int(zero["lst"][1].max()) >= 16384
    assert on["cut"]["pairs_emitted"] < on["info"]["pairs_over_theta"]


# ---- 6. fp32 accumulators: row norms of about 5 put the score bound over what fixed point holds.  LDS float atomics add in
# no fixed order, so no bit equality is asked: check_topk against the oracle.  (The weights are multiples of 1/64 up to 5, every
# product a multiple of 2^-12 and every sum below 2^5, so that the fp32 sums carry no rounding of their own into the 1e-5.)
def test_fp32_accumulators(oracle):
    n, dim, tile, k = 600, 64, 64, 5
    rp, idx, val = synth.make_vectors(n, dim, 8, 0.0, seed=12, dup_frac=0.1)
    val = np.maximum(np.round(val * 5.0 * 64.0), 1.0) / 64.0
    assert np.sqrt(np.add.reduceat(val * val, rp[:-1]).min()) > 4.0
    ids = np.arange(n, dtype=np.int64) + 10
    orc = oracle.selfjoin_pairs(dim, 0.0 - LOWER, rp, idx, val)
    oq, oc = np.asarray(orc[0]), np.asarray(orc[1])
    # at theta = 0 with positive weights every pair that shares a term is a result: the oracle's pairs ARE the rounds' sizes
    sizes = np.unique(oq.astype(np.int64) * 1024 + oc.astype(np.int64) // tile, return_counts=True)[1]
    calls = [("insert_and_query", ids, rp, idx, val)]
    off = run(dim, 0.0, tile, k, False, calls)
    on = run(dim, 0.0, tile, k, True, calls)
    assert on["st"]["probe_kernel"] == "k_probe<2, 512, false, true>" and off["st"]["probe_kernel"] == "k_probe<2, 512, false>"
    orc_ids = (oq + 10, oc + 10, orc[2])
    check_topk(on["got"], orc_ids, k, 0.0, ids)
    check_topk(off["got"], orc_ids, k, 0.0, ids)
    print("fp32: emitted %d of %d, floor %d, rounds cut %d" % (on["cut"]["pairs_emitted"], on["info"]["pairs_over_theta"],
                                                             int(np.minimum(sizes, k).sum()), on["cut"]["rounds_cut"]))
    assert on["cut"]["applied"] == 1
    assert on["info"]["pairs_over_theta"] == len(oq) == off["info"]["pairs_over_theta"]
    assert int(np.minimum(sizes, k).sum()) <= on["cut"]["pairs_emitted"] < on["info"]["pairs_over_theta"]
    assert on["cut"]["rounds_cut"] == int((sizes > k).sum())
    for f in FIVE:
        assert off["info"][f] == on["info"][f], f


# ---- 7. declined paths
def test_declined_paths():
    rp, idx, val = synth.make_vectors(1500, 300, 12, 1.0, seed=21, dup_frac=0.1)
    ids = np.arange(1500, dtype=np.int64) + 100
    calls = [("insert_and_query", ids, rp, idx, val)]
    off = run(300, 0.45, 512, 8, False, calls)
    on = run(300, 0.45, 512, 8, True, calls)
    assert on["cut"]["applied"] == 0 and on["cut"]["declined"] == _lib.TILE_CUT_PATH and on["cut"]["rounds_cut"] == 0
    assert on["cut"]["pairs_emitted"] == on["info"]["pairs_over_theta"]
    assert same_list(off["lst"], on["lst"]) and on["st"]["probe_kernel"] == off["st"]["probe_kernel"]
    assert off["cut"]["declined"] == _lib.TILE_CUT_OFF
    no_k = run(300, 0.0, 512, 0, True, calls)
    assert no_k["cut"]["applied"] == 0 and no_k["cut"]["declined"] == _lib.TILE_CUT_NO_K
    assert no_k["st"]["probe_kernel"] == "k_probe<2, 512, true>"
    with ApssIndex(300, 0.45, tile_rows=512) as ix:
        for bad in (2, -1):
            with pytest.raises(ApssError) as e:
                ix._chk(ix._L.apss_set_top_k_tile_cut(ix._h, bad))
            assert e.value.code == _lib.E_INVALID
    with ApssIndex(300, 0.45, term_range=(0, 150)) as shard:
        with pytest.raises(ApssError) as e:
            shard.set_top_k_tile_cut(True)
        assert e.value.code == _lib.E_UNSUPPORTED and "term shard" in str(e.value)
        shard.set_top_k_tile_cut(False)
