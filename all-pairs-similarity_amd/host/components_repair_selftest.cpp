// components_repair_selftest.cpp -- the per-slot decisions of the components' repair (csrc/apss_components_repair_core.hpp) in
// plain C++: the very touch / detach / renumber the kernels k_cr_touch, k_cr_detach and k_cr_remap take, run slot by slot over
// arrays as the kernels run them, against a textbook recomputation (a union-find of the live-live edges, a renumbering by rank).
//   forests: random edge lists (sparse, a giant component, dense), a path, a star whose hub is not its smallest slot
//   marks:   rows marked by an EARLIER call -- singletons, no edge touches them: the kernels never see a marked row with an edge
//            from an earlier call -- and rows marked by THIS call: roots, leaves and inner slots of their components
// After flatten + touch + detach: every slot of a touched component is a singleton, every other slot is where it was, the selected
// rows are the live rows of the touched components, the unions given back are the detached slots that were no root, and the
// flagged roots number the rows marked earlier plus the touched components.  After the re-join (every live-live edge with a
// selected end, hooked with cc_link as k_cc_hook does): the roots are those of the textbook over the live-live edges, marked rows
// are singletons, unions == live rows - live components.  After the renumbering: the textbook's labels, renumbered by rank.
// No GPU.  Build: see Makefile in this directory (tests/test_components_repair_host.py builds it under the sanitizers and runs it).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <random>
#include <utility>
#include <vector>

#include "../csrc/apss_components_repair_core.hpp"

using apss::CcHostAtomics;
using Edge = std::pair<int32_t, int32_t>;

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                \
    }                                                         \
  } while (0)

// the textbook structure: union by smallest member, find with compression
struct Textbook {
  std::vector<int32_t> p;
  explicit Textbook(int32_t n) : p((size_t)n) { std::iota(p.begin(), p.end(), 0); }
  int32_t find(int32_t x) {
    while (p[(size_t)x] != x) x = p[(size_t)x] = p[(size_t)p[(size_t)x]];
    return x;
  }
  void unite(int32_t a, int32_t b) {
    a = find(a), b = find(b);
    if (a != b) p[(size_t)std::max(a, b)] = std::min(a, b);
  }
};

static void flatten(std::vector<int32_t> &parent) {  // (k_cc_label mode 0)
  for (int32_t x = 0; x < (int32_t)parent.size(); ++x) (void)apss::cc_root_flat<CcHostAtomics>(parent.data(), x);
}

// edges: between rows that were live before this call (none touches a row of `old_dead`); new_dead: the rows this call marks
static void run_case(const char *what, int32_t rows, const std::vector<Edge> &edges, const std::vector<uint8_t> &old_dead,
                     const std::vector<uint8_t> &new_dead) {
  const size_t n = (size_t)rows;
  std::vector<uint8_t> dead(n);
  int64_t n_old = 0, n_dead = 0;
  for (size_t x = 0; x < n; ++x) {
    dead[x] = old_dead[x] | new_dead[x];
    n_old += old_dead[x];
    n_dead += dead[x];
  }
  for (const Edge &e : edges) CHECK(!old_dead[(size_t)e.first] && !old_dead[(size_t)e.second]);
  // the forest before the call, its unions word, and the textbook's view of it
  std::vector<int32_t> parent(n);
  std::iota(parent.begin(), parent.end(), 0);
  int64_t unions = 0;
  Textbook before(rows);
  for (const Edge &e : edges) {
    if (e.first != e.second) unions += apss::cc_link<CcHostAtomics>(parent.data(), e.first, e.second);
    before.unite(e.first, e.second);
  }
  // ---- flatten, touch, detach and select, slot by slot
  flatten(parent);
  std::vector<uint8_t> flag(n, 0);
  for (size_t x = 0; x < n; ++x) {
    const int32_t f = apss::cr_touch(dead[x] != 0, parent[x]);
    if (f >= 0) flag[(size_t)f] = 1;
  }
  const std::vector<int32_t> flat = parent;
  std::vector<uint8_t> keep(n, 0);
  int64_t unhooked = 0, flagged_roots = 0, selected = 0;
  for (size_t x = 0; x < n; ++x) {
    const int32_t p = parent[x];
    const bool flagged = flag[(size_t)p] != 0;
    const apss::CrDetach d = apss::cr_detach((int32_t)x, p, flagged, dead[x] != 0);
    if (d.detach) parent[x] = (int32_t)x;
    keep[x] = d.select;
    selected += d.select;
    unhooked += d.unhook;
    flagged_roots += flagged && p == (int32_t)x;
  }
  unions -= unhooked;
  // what detach leaves
  std::vector<uint8_t> touched(n, 0);  // by the textbook: components that hold a row marked by this call
  for (size_t x = 0; x < n; ++x)
    if (new_dead[x]) touched[(size_t)before.find((int32_t)x)] = 1;
  int64_t n_touched = 0, bad = 0, want_selected = 0;
  for (size_t x = 0; x < n; ++x) {
    n_touched += touched[x];
    const bool in_touched = touched[(size_t)before.find((int32_t)x)] != 0;
    bad += parent[x] != (in_touched || dead[x] ? (int32_t)x : flat[x]);
    bad += keep[x] != (uint8_t)(in_touched && !dead[x]);
    want_selected += in_touched && !dead[x];
  }
  CHECK(bad == 0);
  CHECK(selected == want_selected);
  CHECK(flagged_roots == n_old + n_touched);
  // ---- the re-join: every live-live edge with a selected end, as the probe of the selected rows lists them
  Textbook after(rows);
  for (const Edge &e : edges) {
    const size_t u = (size_t)e.first, v = (size_t)e.second;
    if (dead[u] || dead[v]) continue;
    after.unite(e.first, e.second);
    if ((keep[u] || keep[v]) && u != v) unions += apss::cc_link<CcHostAtomics>(parent.data(), e.first, e.second);
  }
  flatten(parent);
  int64_t live_comps = 0, bad_root = 0;
  for (size_t x = 0; x < n; ++x) {
    bad_root += parent[x] != after.find((int32_t)x);
    bad_root += dead[x] && parent[x] != (int32_t)x;
    live_comps += !dead[x] && after.find((int32_t)x) == (int32_t)x;
  }
  CHECK(bad_root == 0);
  CHECK(unions == (rows - n_dead) - live_comps);
  // ---- the renumbering of a compaction
  std::vector<int64_t> rank(n + 1, 0);
  for (size_t x = 0; x < n; ++x) rank[x + 1] = rank[x] + !dead[x];
  const size_t live = (size_t)rank[n];
  std::vector<int32_t> out(live, -1);
  for (size_t x = 0; x < n; ++x) {
    if (dead[x]) continue;
    const int32_t p = parent[x];
    out[(size_t)rank[x]] = apss::cr_renumber((int32_t)rank[x], (int32_t)rank[(size_t)p], dead[(size_t)p] != 0);
  }
  int64_t bad_remap = 0;
  for (size_t x = 0; x < n; ++x) {
    if (dead[x]) continue;
    const int32_t got = out[(size_t)rank[x]], want = (int32_t)rank[(size_t)after.find((int32_t)x)];
    bad_remap += got != want || got > (int32_t)rank[x];
  }
  CHECK(bad_remap == 0);
  if (bad || bad_root || bad_remap)
    std::printf("%s: %d rows, %lld wrong after detach, %lld wrong roots after the re-join, %lld wrong after the renumbering\n", what, rows,
                (long long)bad, (long long)bad_root, (long long)bad_remap);
}

// a row under a marked root (the invariant broken on purpose): the renumbering makes it a singleton, never a neighbour's child
static void broken_invariant() {
  CHECK(apss::cr_renumber(4, 2, false) == 2);
  CHECK(apss::cr_renumber(4, 2, true) == 4);
  CHECK(apss::cr_touch(false, 3) == -1 && apss::cr_touch(true, 3) == 3);
  const apss::CrDetach live_leaf = apss::cr_detach(5, 2, true, false), dead_root = apss::cr_detach(2, 2, true, true),
                       untouched = apss::cr_detach(7, 6, false, false);
  CHECK(live_leaf.detach && live_leaf.unhook && live_leaf.select);
  CHECK(dead_root.detach && !dead_root.unhook && !dead_root.select);
  CHECK(!untouched.detach && !untouched.unhook && !untouched.select);
}

int main() {
  std::mt19937 rng(11);
  auto marks = [&](int32_t rows, double frac, const std::vector<uint8_t> *avoid) {
    std::vector<uint8_t> m((size_t)rows, 0);
    for (int32_t x = 0; x < rows; ++x)
      m[(size_t)x] = (rng() % 10000) < frac * 10000 && !(avoid && (*avoid)[(size_t)x]);
    return m;
  };
  // random forests: sparse (many components), about rows edges (a giant one forms), dense; marks of both kinds
  for (const int32_t rows : {1, 2, 97, 5000})
    for (const double per_row : {0.3, 1.0, 4.0})
      for (const double new_frac : {0.0, 0.002, 0.05}) {
        const std::vector<uint8_t> old_dead = marks(rows, 0.1, nullptr);
        std::vector<Edge> edges;
        const size_t m = (size_t)(rows * per_row);
        for (size_t i = 0; i < m; ++i) {
          const Edge e{(int32_t)(rng() % (uint32_t)rows), (int32_t)(rng() % (uint32_t)rows)};
          if (!old_dead[(size_t)e.first] && !old_dead[(size_t)e.second]) edges.push_back(e);
        }
        run_case("random", rows, edges, old_dead, marks(rows, new_frac, &old_dead));
      }
  // a path: its middle, its root (the label) and its last leaf marked, each alone and all three; edges given reversed
  {
    const int32_t rows = 20000;
    std::vector<Edge> edges;
    for (int32_t i = rows - 1; i > 0; --i) edges.push_back({i, i - 1});
    const std::vector<uint8_t> none((size_t)rows, 0);
    for (const std::vector<int32_t> &which : {std::vector<int32_t>{rows / 2}, {0}, {rows - 1}, {0, rows / 2, rows - 1}}) {
      std::vector<uint8_t> nd((size_t)rows, 0);
      for (int32_t x : which) nd[(size_t)x] = 1;
      run_case("path", rows, edges, none, nd);
    }
  }
  // a star whose hub is not the smallest slot: the hub marked (every leaf a singleton), the root marked, a leaf marked
  {
    const int32_t rows = 4000, hub = 1234;
    std::vector<Edge> edges;
    for (int32_t i = 0; i < rows; ++i)
      if (i != hub) edges.push_back({hub, i});
    std::shuffle(edges.begin(), edges.end(), rng);
    const std::vector<uint8_t> none((size_t)rows, 0);
    for (const int32_t x : {hub, 0, rows - 1}) {
      std::vector<uint8_t> nd((size_t)rows, 0);
      nd[(size_t)x] = 1;
      run_case("star", rows, edges, none, nd);
    }
  }
  // dead roots and dead leaves of many small components at once, among rows marked earlier
  {
    const int32_t rows = 6000;  // components {3k, 3k + 1, 3k + 2}, every tenth triple marked earlier and without edges
    std::vector<uint8_t> old_dead((size_t)rows, 0), nd((size_t)rows, 0);
    std::vector<Edge> edges;
    for (int32_t k = 0; k < rows / 3; ++k) {
      if (k % 10 == 0) {
        old_dead[(size_t)(3 * k)] = old_dead[(size_t)(3 * k + 1)] = old_dead[(size_t)(3 * k + 2)] = 1;
        continue;
      }
      edges.push_back({3 * k + 2, 3 * k + 1});
      edges.push_back({3 * k + 1, 3 * k});
      if (k % 4 == 1) nd[(size_t)(3 * k)] = 1;      // the root
      if (k % 4 == 2) nd[(size_t)(3 * k + 2)] = 1;  // a leaf
      if (k % 4 == 3) nd[(size_t)(3 * k + 1)] = 1;  // the slot between them: the two others fall apart
    }
    run_case("triples", rows, edges, old_dead, nd);
  }
  broken_invariant();
  if (fails) std::printf("components repair selftest: %d FAILED\n", fails);
  else std::printf("components repair selftest ok\n");
  return fails ? 1 : 0;
}
