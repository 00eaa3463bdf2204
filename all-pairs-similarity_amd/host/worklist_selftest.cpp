// Work lists of the persistent filter launch (csrc/apss_worklist.hpp) against the grid they replace, on the CPU.
// For a handful of launch shapes: every round of every (tile, chunk) cell of the grid launch that does work -- derived here
// the way the kernel derives it from blockIdx (csrc/apss_even.hpp, probe_even_body) -- is covered by exactly one item, on the
// same scale (own_tile) and nothing else is; no item of a symmetric join straddles a tile of the query side; the items before
// the cut pieces are whole cells in tile-major order, and the pieces come last.  Built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <tuple>
#include <vector>

#include "../csrc/apss_worklist.hpp"

using apss::ProbeItem;
using apss::WorkListKey;

namespace {

int failures = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      ++failures;                              \
      std::fprintf(stderr, "FAIL %s: ", name); \
      std::fprintf(stderr, __VA_ARGS__);       \
      std::fprintf(stderr, "\n");              \
    }                                          \
  } while (0)

struct Cell {
  int tile, v0, v1;
  bool own;
};

// the cell of workgroup b of the grid launch, as the kernel works it out; false: it leaves at once
bool grid_cell(const WorkListKey &k, int64_t b, Cell &c) {
  const int mlaunch = k.merge_log2;
  const int tile = k.tile0 + (int)(b / k.n_chunks);
  const int c0 = (int)(b % k.n_chunks) * k.q_chunk;
  const int row_lo = c0 << mlaunch;
  const int row_hi = mlaunch ? std::min(k.nq_rows, (c0 + k.q_chunk) << mlaunch) : 0;
  const bool own = mlaunch != 0 && k.q_slot_base >= 0 && (k.q_slot_base + row_lo) / k.cb <= tile && tile <= (k.q_slot_base + row_hi - 1) / k.cb;
  if (k.tri && tile > row_lo / k.cb) return false;
  c.tile = tile;
  c.own = own;
  c.v0 = own ? row_lo : c0;
  c.v1 = own ? row_hi : std::min(k.nq, c0 + k.q_chunk);
  return true;
}

void check_shape(const char *name, const WorkListKey &k) {
  std::vector<ProbeItem> items;
  const int64_t n_fine = apss::build_work_list(k, items);
  // what the grid does: (tile, own, round) -> 1
  std::map<std::tuple<int, int, int>, int> todo;
  std::vector<Cell> cells;
  for (int64_t b = 0; b < (int64_t)k.n_tiles * k.n_chunks; ++b) {
    Cell c;
    if (!grid_cell(k, b, c)) continue;
    cells.push_back(c);
    for (int v = c.v0; v < c.v1; ++v) todo[std::make_tuple(c.tile, (int)c.own, v)] += 1;
  }
  size_t rounds = todo.size();
  for (const ProbeItem &it : items) {
    CHECK(it.v1 > it.v0, "empty item tile %d [%d, %d)", it.tile, it.v0, it.v1);
    for (int v = it.v0; v < it.v1; ++v) {
      auto f = todo.find(std::make_tuple(it.tile, it.own, v));
      CHECK(f != todo.end() && f->second == 1, "round %d of tile %d (own %d) is not the grid's, or covered twice", v, it.tile, it.own);
      if (f != todo.end()) f->second -= 1;
    }
    if (k.tri) {
      const int mlog = it.own ? 0 : k.merge_log2;
      const int64_t lo = (int64_t)it.v0 << mlog, hi = std::min<int64_t>(k.nq_rows, (int64_t)it.v1 << mlog);
      CHECK(lo / k.cb == (hi - 1) / k.cb, "item [%d, %d) straddles a query tile", it.v0, it.v1);
      CHECK(it.tile <= lo / k.cb, "item of tile %d above the diagonal (query tile %lld)", it.tile, (long long)(lo / k.cb));
    }
  }
  for (const auto &kv : todo) CHECK(kv.second == 0, "round %d of tile %d left uncovered", std::get<2>(kv.first), std::get<0>(kv.first));
  // whole cells first, in the grid's order; the pieces of the cut cells last
  const size_t n_whole = items.size() - (size_t)n_fine;
  CHECK(n_fine >= 0 && (size_t)n_fine <= items.size(), "pieces %lld of %zu items", (long long)n_fine, items.size());
  for (size_t i = 0; i < n_whole && i < cells.size(); ++i)
    CHECK(items[i].tile == cells[i].tile && items[i].v0 == cells[i].v0 && items[i].v1 == cells[i].v1 && (items[i].own != 0) == cells[i].own,
          "item %zu is not cell %zu of the grid", i, i);
  for (size_t i = n_whole; i < items.size(); ++i) {
    CHECK(items[i].v1 - items[i].v0 <= k.fine, "piece %zu is %d rounds long (fine %d)", i, items[i].v1 - items[i].v0, k.fine);
    if (i > n_whole) CHECK(items[i].tile >= items[i - 1].tile, "piece %zu leaves the tile-major order", i);
  }
  if (n_fine > 0) {
    const size_t want_cut = std::min<size_t>(cells.size(), 2 * (size_t)k.slots);
    CHECK(n_whole == cells.size() - want_cut, "%zu whole items, want %zu cells - %zu cut", n_whole, cells.size(), want_cut);
  } else {
    CHECK(items.size() == cells.size(), "%zu items for %zu cells", items.size(), cells.size());
  }
  std::printf("%-28s cells %6zu rounds %9zu items %6zu pieces %6lld\n", name, cells.size(), rounds, items.size(), (long long)n_fine);
}

WorkListKey shape(int nq_rows, int merge_log2, int want_chunks, int cb, int tri, int64_t q_slot_base, int tile0, int n_tiles, int fine, int slots) {
  WorkListKey k;
  const int M = 1 << merge_log2;
  int q_chunk = std::max(1, (nq_rows + want_chunks - 1) / want_chunks);
  if (tri) {
    int qc = 1;
    while (qc < q_chunk) qc <<= 1;
    q_chunk = qc;
  }
  const int qc_rows = (q_chunk + M - 1) / M * M;  // (a chunk is a whole number of merged rounds)
  k.q_chunk = qc_rows / M;
  k.n_chunks = (nq_rows + qc_rows - 1) / qc_rows;
  k.nq = (nq_rows + M - 1) / M;
  k.nq_rows = nq_rows;
  k.merge_log2 = merge_log2;
  k.cb = cb;
  k.tri = tri;
  k.q_slot_base = q_slot_base;
  k.tile0 = tile0;
  k.n_tiles = n_tiles;
  k.fine = fine;
  k.slots = slots;
  return k;
}

}  // namespace

int main() {
  // the flagship: 1M rows, 31 tiles of 32768, symmetric, chunks of 1024 rounds, 512 resident slots
  check_shape("c3 symmetric", shape(1000000, 0, 1024, 32768, 1, 0, 0, 31, 256, 512));
  check_shape("c3 symmetric fine 128", shape(1000000, 0, 1024, 32768, 1, 0, 0, 31, 128, 512));
  check_shape("c3 two-directional", shape(1000000, 0, 1024, 32768, 0, 0, 0, 31, 256, 512));
  // small symmetric join: a last tile partly filled, a last chunk shorter than the others, more pieces than cells
  check_shape("small symmetric", shape(4100, 0, 32, 1024, 1, 0, 0, 5, 16, 4));
  check_shape("small symmetric all cut", shape(4100, 0, 32, 1024, 1, 0, 0, 5, 8, 4096));
  // an outside batch, odd sizes, the smallest pieces, one tile range of a split launch
  check_shape("outside batch fine 1", shape(777, 0, 13, 512, 0, -1, 2, 3, 1, 3));
  check_shape("outside batch fine 2", shape(778, 0, 7, 512, 0, -1, 0, 4, 2, 1));
  check_shape("nothing cut", shape(300, 0, 64, 1024, 0, -1, 0, 2, 256, 512));
  check_shape("one item", shape(5, 0, 1, 1024, 0, -1, 0, 1, 256, 512));
  // merged rounds: a stored batch whose diagonal cells run unmerged, appended behind 1500 stored rows; odd row count
  check_shape("merged whole store", shape(6001, 1, 24, 1024, 0, 0, 0, 6, 32, 2));
  check_shape("merged appended", shape(2049, 1, 16, 1024, 0, 1500, 0, 4, 16, 3));
  check_shape("merged outside", shape(2049, 2, 16, 1024, 0, -1, 0, 4, 16, 3));
  check_shape("merged symmetric", shape(5000, 1, 20, 1024, 1, 0, 0, 5, 64, 2));
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("worklist selftest ok\n");
  return 0;
}
