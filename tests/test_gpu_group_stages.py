"""GPU tests of the branches a split of the group's phase into stages can get wrong (csrc/apss_group.hip: member_phase and its
stages, range_final_list): a member of the copies exchange without a candidate, a phase with nothing to exchange, the two
transports on the same union, a grid's mirrored outside phase behind an exchange and its triples without one, a member's
refusal on a grid (two row ranges, one failure flag).  Smallest shapes that reach them -- dim 96, 128 rows of 6 terms, theta 0.7
-- against the CPU oracle at the suite's tolerance for group scores; every case has a group of its own.
Planting: rows 2k and 2k + 1 are identical, so the list holds at least 128 directed pairs whatever else is drawn; base row
k + 32 is base row k with its values disturbed, so a 2-way split of the rows has pairs across its two spans."""
import numpy as np
import pytest

from apss import _lib
from helpers import assert_same_pairs, to_map

pytestmark = pytest.mark.gpu

DIM, ROWS, NNZ, THETA = 96, 128, 6, 0.7


def _planted(term_hi=DIM, seed=11):
    """128 rows of 6 terms below term_hi, unit norm: rows 2k, 2k + 1 identical; base k + 32 = base k, values disturbed"""
    rng = np.random.default_rng(seed)
    base_idx = np.stack([np.sort(rng.choice(term_hi, NNZ, replace=False)) for _ in range(ROWS // 4)])
    base_val = rng.uniform(0.3, 1.0, size=(ROWS // 4, NNZ))
    near_val = base_val * rng.uniform(0.8, 1.25, size=base_val.shape)
    idx = np.repeat(np.concatenate([base_idx, base_idx]), 2, axis=0)
    val = np.repeat(np.concatenate([base_val, near_val]), 2, axis=0)
    val /= np.sqrt((val * val).sum(axis=1, keepdims=True))
    rp = np.arange(0, (ROWS + 1) * NNZ, NNZ, dtype=np.int64)
    ids = np.arange(ROWS, dtype=np.int64) * 3 + 1000
    return ids, rp, idx.reshape(-1).astype(np.int32), val.reshape(-1).astype(np.float64)


@pytest.fixture(scope="module")
def planted(oracle):
    """the planted batch and the oracle's list of its self-join (computed once, read only)"""
    ids, rp, idx, val = _planted()
    oq, oc, os_ = oracle.selfjoin_pairs(DIM, THETA, rp, idx, val)
    want = to_map(ids[oq], ids[oc], os_)
    assert len(want) >= 128 and all((ids[2 * k], ids[2 * k + 1]) in want for k in range(ROWS // 2))
    assert sum((q < ids[64]) != (c < ids[64]) for q, c in want) >= 128  # pairs across the two halves of the rows
    return (ids, rp, idx, val), want


def _group(T, D=1, **kw):
    from apss.engine import ApssGroup
    return ApssGroup(DIM, kw.pop("theta", THETA), [0] * (T * D), row_ranges=D, head_terms=-1, **kw)


def test_copies_exchange_with_a_member_without_candidates(oracle):
    """three members on device 0, every term below 64: with the equal cuts of a small first batch (0, 32, 64, 96) the third
    member holds no posting and brings no candidate -- pack, gather and reduce skip its empty list -- and the answer is the oracle's"""
    ids, rp, idx, val = _planted(term_hi=64, seed=12)
    oq, oc, os_ = oracle.selfjoin_pairs(DIM, THETA, rp, idx, val)
    want = to_map(ids[oq], ids[oc], os_)
    assert len(want) >= 128
    with _group(3) as g:
        got = to_map(*g.insert_and_query(ids, rp, idx, val))
        st = g.stats()
        ms = [g.member_stats(i) for i in range(3)]
    print("candidates per member", [m["result_pairs"] for m in ms], "union", st["union_pairs"], "results", len(got))
    assert st["exchange"] == _lib.EXCHANGE_COPIES and st["term_cuts"] == [0, 32, 64, 96]
    assert ms[2]["nnz"] == 0 and ms[2]["result_pairs"] == 0 and ms[0]["result_pairs"] > 0 and ms[1]["result_pairs"] > 0
    assert st["candidates_max"] > 0 and st["candidates_sum"] == sum(m["result_pairs"] for m in ms)
    assert st["all_gather_bytes"] == 8 * st["candidates_sum"]  # (total - least, and the least is the empty list)
    assert st["result_pairs"] == len(got) <= st["union_pairs"] <= st["candidates_sum"]
    assert_same_pairs(got, want, THETA)


def test_nothing_to_exchange_then_the_next_call(oracle):
    """no member has a candidate: every member leaves the phase together before the pack, the call answers 0 pairs, and the
    group's next call runs the whole exchange.  Row r holds term t = r mod 96 and one more of t's member's range (t + 1, or
    t + 2 for the rows from 96 on, cyclic in the range): two rows share one term at most, the cosine stays below 0.65"""
    theta = 0.99
    t = np.arange(ROWS) % DIM
    lo = t // 32 * 32
    other = lo + (t - lo + np.where(np.arange(ROWS) < DIM, 1, 2)) % 32
    idx = np.sort(np.stack([t, other], axis=1), axis=1).astype(np.int32)
    val = np.where(idx == t[:, None], 0.8, 0.6)
    rp = np.arange(0, 2 * ROWS + 1, 2, dtype=np.int64)
    ids = np.arange(ROWS, dtype=np.int64) + 5000
    w = oracle.Worker(DIM, theta)
    assert w.index_data(ids, rp, idx.reshape(-1), val.reshape(-1))[0].size == 0
    pids, prp, pidx, pval = _planted()
    want = to_map(*w.index_data(pids, prp, pidx, pval))
    assert len(want) >= 128
    with _group(3, theta=theta) as g:
        q, c, s = g.insert_and_query(ids, rp, idx.reshape(-1), val.reshape(-1))
        st = g.stats()
        assert q.size == 0 and g.result_count() == 0
        assert st["exchange"] == _lib.EXCHANGE_COPIES and st["rows"] == ROWS
        assert st["candidates_sum"] == 0 and st["union_pairs"] == 0 and st["all_gather_bytes"] == 0 and st["posting_visits"] > 0
        got = to_map(*g.insert_and_query(pids, prp, pidx, pval))
        st = g.stats()
        assert st["rows"] == 2 * ROWS and st["union_pairs"] >= len(got) > 0
    assert_same_pairs(got, want, theta)


def test_both_transports_give_the_same_list_bit_for_bit(planted):
    """one member made to exchange, over RCCL and over copies: the same union and the same single partial score per pair, so
    the two lists are equal as sets with scores equal bit for bit (and are the oracle's)"""
    (ids, rp, idx, val), want = planted
    lists = {}
    for name, flags, exchange in (("rccl", _lib.GROUP_FORCE_EXCHANGE, _lib.EXCHANGE_RCCL),
                                  ("copies", _lib.GROUP_FORCE_EXCHANGE | _lib.GROUP_NO_RCCL, _lib.EXCHANGE_COPIES)):
        with _group(1, group_flags=flags) as g:
            q, c, s = g.insert_and_query(ids, rp, idx, val)
            st = g.stats()
        assert st["exchange"] == exchange and st["union_pairs"] == st["candidates_sum"] == q.size
        assert s.dtype == np.float32
        lists[name] = {(int(a), int(b)): v.tobytes() for a, b, v in zip(q, c, s)}
        assert len(lists[name]) == q.size
        assert_same_pairs(to_map(q, c, s), want, THETA)
    assert lists["rccl"] == lists["copies"]


def test_grid_mirrored_outside_phase_with_and_without_an_exchange(planted):
    """2 x 2 on device 0, the batch inserted-and-queried into the empty group: symmetric ranges, so row range 0 meets span 1 as
    a mirrored outside batch and appends its triples behind an exchange.  Then 1 x 2 (top-k off): a row range of one member, whose
    triples come straight from the handle's list"""
    (ids, rp, idx, val), want = planted
    with _group(2, 2) as g:
        got = to_map(*g.insert_and_query(ids, rp, idx, val))
        st, gr = g.stats(), g.grid()
    assert st["exchange"] == _lib.EXCHANGE_COPIES and st["n_members"] == 4 and st["result_pairs"] == len(got)
    assert gr["symmetric_ranges"] == 1 and gr["mirrored_pairs"] > 0 and gr["rows_in_range"] == [64, 64]
    assert st["union_pairs"] >= len(got) - gr["mirrored_pairs"] > 0
    assert_same_pairs(got, want, THETA)
    with _group(1, 2) as g:
        got1 = to_map(*g.insert_and_query(ids, rp, idx, val))
        st, gr = g.stats(), g.grid()
    assert st["exchange"] == _lib.EXCHANGE_NONE and st["n_members"] == 2 and st["result_pairs"] == len(got1)
    assert gr["symmetric_ranges"] == 1 and gr["mirrored_pairs"] > 0
    assert st["union_pairs"] == len(got1) - gr["mirrored_pairs"]
    assert_same_pairs(got1, want, THETA)


def test_a_members_refusal_stops_both_row_ranges(oracle, planted):
    """one row of the batch names a term >= dim: the members that are handed it refuse, ONE flag stops the threads of both row
    ranges of the 2 x 2 grid, the call fails with APSS_E_INVALID and the member's message, and the group goes on answering: a
    query of the frozen index at once (nothing was committed), an insert-and-query after a clear"""
    from apss.engine import ApssError
    (ids, rp, idx, val), want = planted
    bad = idx.copy()
    bad[100 * NNZ + NNZ - 1] = DIM + 3  # (row 100, in the second span; still strictly increasing)
    w = oracle.Worker(DIM, THETA)
    w.index_data(ids, rp, idx, val)
    want_query = to_map(*w.index_data(ids + 7, rp, idx, val, query_only=True))
    assert len(want_query) >= 2 * ROWS  # (every row meets itself and its twin under other ids)
    with _group(2, 2) as g:
        assert_same_pairs(to_map(*g.insert_and_query(ids, rp, idx, val)), want, THETA)
        with pytest.raises(ApssError) as e:
            g.query(ids + 7, rp, bad, val)
        assert e.value.code == _lib.E_INVALID and "member" in str(e.value)
        assert_same_pairs(to_map(*g.query(ids + 7, rp, idx, val)), want_query, THETA)
        with pytest.raises(ApssError) as e:
            g.insert_and_query(ids + 7, rp, bad, val)
        assert e.value.code == _lib.E_INVALID and "member" in str(e.value)
        with pytest.raises(ApssError):
            g.fetch()  # (a failed call leaves no list behind)
        g.clear()
        assert_same_pairs(to_map(*g.insert_and_query(ids, rp, idx, val)), want, THETA)
        assert g.grid()["rows_in_range"] == [64, 64]
