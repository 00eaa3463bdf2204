"""The persistent launch of the thin-round filter (csrc/apss_even.hpp, csrc/apss_worklist.hpp): resident workgroups take items
{tile, rounds} of a work list through a counter instead of one workgroup running one (tile, chunk) cell of a grid.

Every scenario of persist_child.py runs twice, each time in a process of its own (APSS_DEBUG differs): with the persistent
launch and with APSS_DEBUG=no_persist.  The two runs must report the same sorted (query, candidate, score) list bit for bit and
the same posting_visits, device_posting_visits, candidate_pairs and filter_survivors; the thin-round kernel ran in both; the
`[apss diag] persist:` line says what was launched.  One configuration per input is also checked against the oracle."""
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

import persist_child as pc
from helpers import assert_same_pairs, to_map

pytestmark = pytest.mark.gpu

COUNTERS = ("posting_visits", "device_posting_visits", "candidate_pairs", "filter_survivors", "result_pairs", "thin_launches",
            "probe_kernel", "query_chunk", "symmetric", "queries_per_round", "tiles")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    out = {}
    d = tmp_path_factory.mktemp("persist")
    for mode in ("persist", "grid"):
        path = str(d / (mode + ".pkl"))
        env = {k: v for k, v in os.environ.items() if k != "APSS_DEBUG"}
        r = subprocess.run([sys.executable, os.path.join(pc.HERE, "persist_child.py"), mode, path], env=env, capture_output=True,
                           text=True, timeout=600)
        err = open(path + ".stderr").read()[-3000:] if os.path.exists(path + ".stderr") else ""
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:], err)
        with open(path, "rb") as f:
            out[mode] = pickle.load(f)
    return out


@pytest.fixture(scope="module")
def inputs():
    return pc.scenario_inputs()


@pytest.fixture(scope="module")
def wanted(oracle, inputs):
    """the oracle's pairs of every input's self-join (theta as the child runs it), computed once"""
    return {key: to_map(*oracle.selfjoin_pairs(dim, 0.7 if key == "shards" else pc.THETA, rp, idx, val))
            for key, (dim, rp, idx, val) in inputs.items()}


def _launch(diag):
    """(items, pieces, workgroups) of every `[apss diag] persist:` line"""
    return [tuple(int(x) for x in m.groups()) for ln in diag
            for m in [re.match(r"\[apss diag\] persist: items (\d+) fine (\d+) workgroups (\d+)", ln)] if m]


def _calls(res):
    return res["calls"] if "calls" in res else [res]


@pytest.mark.parametrize("name", [s[0] for s in pc.SCENARIOS])
def test_same_as_the_grid_launch(runs, name):
    for p, g in zip(_calls(runs["persist"][name]), _calls(runs["grid"][name])):
        assert _launch(p["diag"]) and not _launch(g["diag"]), (p["diag"], g["diag"])
        for a, b in zip(p["pairs"], g["pairs"]):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
        assert len(p["pairs"][0]) > 50
        ps, gs = (x["stats"] if isinstance(x["stats"], list) else [x["stats"]] for x in (p, g))
        for sp, sg in zip(ps, gs):
            assert sp["probe_kernel"].startswith("k_probe_even") and sp["thin_launches"] > 0, sp["probe_kernel"]
            for k in COUNTERS:
                assert sp[k] == sg[k], (k, sp[k], sg[k])
        for items, fine, wgs in _launch(p["diag"]):
            assert 0 < wgs <= items and 0 <= fine <= items


@pytest.mark.parametrize("name,wgs", [("many_wgs1", 1), ("many_wgs3", 3), ("rare_wgs1", 1), ("stale_wgs1", 1), ("shards_merged_wgs1", 1)])
def test_forced_workgroup_counts(runs, name, wgs):
    launches = _launch(runs["persist"][name]["diag"])
    assert launches and all(w == wgs and items > 10 * wgs for items, _, w in launches), launches


def test_more_items_than_workgroups_whatever_their_number(runs):
    """one, three and all resident workgroups over the same list's cells: the same pairs"""
    a, b, c = (runs["persist"][n] for n in ("many_wgs1", "many_wgs3", "many_default"))
    for x in (b, c):
        for u, v in zip(a["pairs"], x["pairs"]):
            assert u.tobytes() == v.tobytes()
    assert a["stats"]["tiles"] >= 4 and _launch(a["diag"])[0][0] >= 48


def test_fewer_items_than_workgroups(runs):
    assert _launch(runs["persist"]["one_item"]["diag"]) == [(1, 0, 1)]
    assert _launch(runs["persist"]["two_items"]["diag"]) == [(2, 0, 2)]


def test_symmetric_join_lists_no_cell_above_the_diagonal(runs, inputs):
    """2,600 rows, filter tiles of 512, chunks of 64 rows (the last one of 40 in a sixth tile of 40 rows): chunk c of query tile
    c div 8 meets the tiles 0 .. c div 8, so the list holds the sum of (c div 8 + 1) over the 41 chunks"""
    res = runs["persist"]["many_uncut"]
    st = res["stats"]
    n = inputs["many"][1].size - 1
    assert st["symmetric"] == 1 and st["query_chunk"] == 64 and st["filter_tile_rows"] == 512 and st["tiles"] == 6
    n_chunks = -(-n // 64)
    assert n % 64 and n % 512  # a short last chunk, a last tile partly filled
    want = sum(c * 64 // 512 + 1 for c in range(n_chunks))
    assert want == 126 and want < n_chunks * st["tiles"]
    (items, fine, wgs), = _launch(res["diag"])
    assert (items, fine) == (want, 0) and wgs == min(want, wgs)
    # ... and cut in pieces of 16 rounds by three workgroups: the last six cells are four pieces each, the short chunk's three
    (items, fine, wgs), = _launch(runs["persist"]["many_wgs3"]["diag"])
    short = -(-(n - (n_chunks - 1) * 64) // 16)
    assert short == 3 and fine == 4 * 4 + 2 * short and items == want - 6 + fine and wgs == 3


def test_pieces_of_one_two_and_three_rounds(runs):
    """chunks of 7 rounds and a last one of 3: pieces of 1; of 2 with a last one of 1; of 4 and 3 -- odd totals on every item
    boundary of the adding waves' loop, which steps by two"""
    for name, per_chunk, last in (("nosym_fine1", 7, 3), ("nosym_fine2", 4, 2), ("nosym_fine4", 2, 1)):
        res = runs["persist"][name]
        st = res["stats"]
        assert st["symmetric"] == 0 and st["query_chunk"] == 7 and st["tiles"] == 6
        (items, fine, wgs), = _launch(res["diag"])
        cells = 372 * 6
        if name != "nosym_fine4":  # five workgroups: the last ten cells are cut, the sixth tile's last chunks, the very last one short
            assert wgs == 5 and fine == 9 * per_chunk + last and items == cells - 10 + fine, (items, fine)
        else:
            assert fine >= per_chunk and items >= cells
    for name in ("outside_fine1", "outside_fine2"):
        st = runs["persist"][name]["stats"]
        assert st["symmetric"] == 0 and st["query_chunk"] == 7


def test_against_the_oracle(runs, inputs, wanted):
    """one configuration per input: pairs and scores (the persistent launch's; the grid launch's are the same bytes)"""
    for name, key, theta in (("many_wgs3", "many", pc.THETA), ("one_item", "few", pc.THETA), ("nosym_fine1", "many", pc.THETA),
                             ("rare_fine32", "rare", pc.THETA), ("stale_fine16", "stale", pc.THETA), ("shards_merged_wgs1", "shards", 0.7),
                             ("shards_unmerged", "shards", 0.7), ("regrow", "many", pc.THETA)):
        q, c, s = runs["persist"][name]["pairs"]
        got = to_map(q, c, s)
        assert len(got) == len(q), "a pair reported twice"
        assert_same_pairs(got, wanted[key], theta)
        assert len(wanted[key]) > 50, (name, len(wanted[key]))


def test_rare_rounds_end_items(runs, inputs):
    """the heavy term's segment in the first tile is a long one (more than 256 postings) and the last row of every 64 of the
    second tile holds it: those rounds are swept and end with a whole-tile clear, as the last round of an item"""
    dim, rp, idx, val = inputs["rare"]
    row = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    holders = row[idx == pc.HEAVY]
    assert (holders < 512).sum() > 256
    assert set(range(575, 1024, 64)) <= set(holders.tolist())
    st = runs["persist"]["rare_wgs1"]["stats"]
    assert st["query_chunk"] == 64 and st["tiles"] == 2 and st["symmetric"] == 0
    assert _launch(runs["persist"]["rare_wgs1"]["diag"]) == [(32, 0, 1)]
    assert _launch(runs["persist"]["rare_fine32"]["diag"]) == [(34, 4, 1)]  # (one workgroup: the last two cells in halves)


def test_regrowth_runs_the_list_again_from_its_start(runs):
    """the candidate list starts at 64 entries: the probe overflows it, grows it and runs again -- behind the memset that
    zeroes the work counter.  Same pairs as without the hook"""
    a, b = runs["persist"]["regrow"], runs["persist"]["many_wgs3"]
    assert len(_launch(a["diag"])) >= 2 and len(_launch(b["diag"])) == 1
    for u, v in zip(a["pairs"], b["pairs"]):
        assert u.tobytes() == v.tobytes()
    for k in ("posting_visits", "candidate_pairs", "filter_survivors"):
        assert a["stats"][k] == b["stats"][k]


def test_cached_list_is_rebuilt_for_another_batch_size(runs, inputs, wanted):
    """500, then 777 outside query rows on one handle, 50 chunks asked for: 50 chunks of 10 rows, then 49 of 16 (the last one of
    9), over 6 tiles, the last four cells in pieces of 4 rounds; both answers against the oracle (a query row is a copy of a
    stored row: its pairs are that row's and the row itself)"""
    dim, rp, idx, val = inputs["many"]
    calls = runs["persist"]["cache"]["calls"]
    for call, m in zip(calls, (500, 777)):
        q_chunk = -(-m // 50)
        assert call["stats"]["query_chunk"] == q_chunk and q_chunk == (10, 16)[m == 777]
        cells = -(-m // q_chunk) * 6
        fine = 3 * -(-q_chunk // 4) + -(-(m - (-(-m // q_chunk) - 1) * q_chunk) // 4)
        assert _launch(call["diag"]) == [(cells - 4 + fine, fine, 2)], (_launch(call["diag"]), cells, fine)
        want = {(q + pc.QUERY_ID0, c): s for (q, c), s in wanted["many"].items() if q < m}
        want.update({(q + pc.QUERY_ID0, q): 1.0 for q in range(m)})
        q, c, s = call["pairs"]
        got = to_map(q, c, s)
        assert len(got) == len(q)
        assert_same_pairs(got, want, pc.THETA)
    assert _launch(calls[0]["diag"]) != _launch(calls[1]["diag"])
