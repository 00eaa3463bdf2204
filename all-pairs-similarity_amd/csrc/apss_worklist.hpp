// The WORK LIST of a persistent filter launch (k_probe_even, k_probe_even_merged; apss_even.hpp): what the (tile, chunk) grid
// of the launch holds, as a list of items {candidate tile, first round, last round} that resident workgroups take one after
// another through a counter.  Plain C++ (no HIP): probe() builds the list on the host, host/worklist_selftest.cpp checks it.
//
//  * tile-major, as the grid was: the chip works on one tile's postings at a time and they stay in L2 / Infinity Cache;
//  * only cells that do work: the mirrored half of a symmetric join (tile above the queries' tile) is not listed;
//  * coarse items of the launch's q_chunk rounds, and the LAST coarse items -- two fills of the resident slots -- cut into
//    pieces of `fine` rounds (a power of two), so that the launch ends within one short item of all slots falling idle
//    instead of within one whole chunk;
//  * an item's rounds are counted on ITS OWN scale: a cell whose candidate tile holds rows of its own chunk runs its rows one
//    per round (`own`, see MERGED rounds in apss_even.hpp) -- decided per CELL here, exactly as the grid launch decides it, and
//    inherited by the pieces of a cut cell, so that both launches report the same rounds.  A piece of a symmetric join's cell
//    lies inside one query tile because the cell does.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace apss {

struct alignas(16) ProbeItem {
  int32_t tile;    // candidate tile
  int32_t v0, v1;  // rounds [v0, v1): query rows when `own` (or nothing is merged), else merged rounds of 2^merge_log2 rows
  int32_t own;     // 1: the candidate tile holds rows of the cell's own chunk (merged launches only)
};

// everything a list depends on
struct WorkListKey {
  int64_t q_slot_base = -1;  // slot of query row 0 when the batch is stored in the index, else -1 (decides `own`)
  int32_t nq = 0;            // rounds of the launch
  int32_t nq_rows = 0;       // query rows
  int32_t q_chunk = 0;       // rounds per cell
  int32_t n_chunks = 0;
  int32_t cb = 0;            // rows per tile
  int32_t tri = 0;
  int32_t merge_log2 = 0;
  int32_t tile0 = 0, n_tiles = 0;  // the launch's tiles
  int32_t fine = 0;          // rounds per piece of a cut cell (a power of two; 0 or >= q_chunk: nothing is cut)
  int32_t slots = 0;         // workgroups the chip holds at a time
  bool operator==(const WorkListKey &o) const {
    return q_slot_base == o.q_slot_base && nq == o.nq && nq_rows == o.nq_rows && q_chunk == o.q_chunk && n_chunks == o.n_chunks &&
           cb == o.cb && tri == o.tri && merge_log2 == o.merge_log2 && tile0 == o.tile0 && n_tiles == o.n_tiles && fine == o.fine &&
           slots == o.slots;
  }
};

// the cell (tile, chunk) as the grid launch's workgroup derives it; false: the cell does no work
inline bool work_cell(const WorkListKey &k, int32_t tile, int32_t chunk, ProbeItem &it) {
  const int m = k.merge_log2;
  const int64_t c0 = (int64_t)chunk * k.q_chunk;
  const int64_t row_lo = c0 << m, row_hi = std::min<int64_t>(k.nq_rows, (c0 + k.q_chunk) << m);
  if (k.tri && tile > row_lo / k.cb) return false;
  const bool own = m != 0 && k.q_slot_base >= 0 && (k.q_slot_base + row_lo) / k.cb <= tile && tile <= (k.q_slot_base + row_hi - 1) / k.cb;
  it.tile = tile;
  it.own = own ? 1 : 0;
  it.v0 = (int32_t)(own ? row_lo : c0);
  it.v1 = (int32_t)(own ? row_hi : std::min<int64_t>(k.nq, c0 + k.q_chunk));
  return it.v1 > it.v0;
}

// appends the launch's items to `out`; returns how many of them are pieces of cut cells
inline int64_t build_work_list(const WorkListKey &k, std::vector<ProbeItem> &out) {
  const size_t first = out.size();
  ProbeItem it;
  for (int32_t tile = k.tile0; tile < k.tile0 + k.n_tiles; ++tile)
    for (int32_t chunk = 0; chunk < k.n_chunks; ++chunk)
      if (work_cell(k, tile, chunk, it)) out.push_back(it);
  if (k.fine <= 0 || k.fine >= k.q_chunk || k.slots <= 0) return 0;
  const size_t n = out.size() - first;
  const size_t n_cut = std::min<size_t>(n, 2 * (size_t)k.slots);
  std::vector<ProbeItem> cut(out.end() - (std::ptrdiff_t)n_cut, out.end());
  out.resize(out.size() - n_cut);
  int64_t n_fine = 0;
  for (const ProbeItem &c : cut)
    for (int32_t v = c.v0; v < c.v1; v += k.fine, ++n_fine) out.push_back(ProbeItem{c.tile, v, std::min(c.v1, v + k.fine), c.own});
  return n_fine;
}

}  // namespace apss
