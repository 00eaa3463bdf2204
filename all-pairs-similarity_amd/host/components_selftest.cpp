// components_selftest.cpp -- the union-find core of apss_set_components (csrc/apss_components_core.hpp) in plain C++: the very
// find / link / shorten the kernels run, through the host atomics policy, against a textbook union-find.
//   sequential: random edge lists; a path given forward, reversed and shuffled; a star; duplicate edges and self-loops
//   threads:    8 std::threads hook disjoint slices of one shuffled edge list into one forest (the mode -fsanitize=thread runs)
// After every run the root of every slot (cc_root_flat, as the labelling does) is the SMALLEST slot of its component, the links
// that reported a join number rows - components, and parent[x] <= x holds everywhere.
// No GPU.  Build: see Makefile in this directory (tests/test_components_host.py builds it under the sanitizers and runs it).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <random>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../csrc/apss_components_core.hpp"

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

// the textbook structure: union by smallest member, find with full compression, one thread
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

static int64_t hook_slice(std::vector<int32_t> &parent, const std::vector<Edge> &edges, size_t lo, size_t hi) {
  int64_t joined = 0;
  for (size_t i = lo; i < hi; ++i) {
    const int32_t u = edges[i].first, v = edges[i].second;
    if (u == v || apss::cc_same_parent<CcHostAtomics>(parent.data(), u, v)) continue;  // (as k_cc_hook)
    joined += apss::cc_link<CcHostAtomics>(parent.data(), u, v);
  }
  return joined;
}

static void run_case(const char *what, int32_t rows, const std::vector<Edge> &edges, int threads) {
  std::vector<int32_t> parent((size_t)rows);
  std::iota(parent.begin(), parent.end(), 0);
  int64_t joined = 0;
  if (threads <= 1) {
    joined = hook_slice(parent, edges, 0, edges.size());
  } else {
    std::vector<int64_t> part((size_t)threads, 0);
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t)
      pool.emplace_back([&, t] {
        part[(size_t)t] = hook_slice(parent, edges, edges.size() * (size_t)t / (size_t)threads, edges.size() * (size_t)(t + 1) / (size_t)threads);
      });
    for (std::thread &th : pool) th.join();
    joined = std::accumulate(part.begin(), part.end(), (int64_t)0);
  }
  Textbook ref(rows);
  for (const Edge &e : edges) ref.unite(e.first, e.second);
  int64_t comps = 0, bad_root = 0, bad_order = 0;
  for (int32_t x = 0; x < rows; ++x) {
    bad_order += parent[(size_t)x] > x;
    const int32_t r = apss::cc_root_flat<CcHostAtomics>(parent.data(), x);
    bad_root += r != ref.find(x);
    comps += ref.find(x) == x;
  }
  for (int32_t x = 0; x < rows; ++x) bad_root += parent[(size_t)x] != ref.find(x);  // (flat after the labelling's walk)
  if (bad_root || bad_order || joined != rows - comps)
    std::printf("%s (%d thread%s): %lld wrong roots, %lld parents above their slot, %lld joins for %lld components of %d rows\n", what, threads,
                threads == 1 ? "" : "s", (long long)bad_root, (long long)bad_order, (long long)joined, (long long)comps, rows);
  CHECK(bad_root == 0);
  CHECK(bad_order == 0);
  CHECK(joined == rows - comps);
}

int main(int argc, char **argv) {
  const bool threaded = argc > 1 && std::string(argv[1]) == "threads";
  const int T = threaded ? 8 : 1;
  std::mt19937 rng(5);
  // random edge lists: sparse (many components), about rows edges (a giant one forms), dense
  for (const int32_t rows : {1, 2, 97, 5000})
    for (const double per_row : {0.3, 1.0, 4.0}) {
      std::vector<Edge> edges;
      const size_t m = (size_t)(rows * per_row);
      for (size_t i = 0; i < m; ++i) edges.push_back({(int32_t)(rng() % (uint32_t)rows), (int32_t)(rng() % (uint32_t)rows)});  // (self-loops included)
      run_case("random", rows, edges, T);
    }
  // a path, in the three orders: reversed is the one that leaves the longest chains
  {
    const int32_t rows = 20000;
    std::vector<Edge> fwd, rev, shuf;
    for (int32_t i = 0; i + 1 < rows; ++i) fwd.push_back({i + 1, i});
    rev.assign(fwd.rbegin(), fwd.rend());
    shuf = fwd;
    std::shuffle(shuf.begin(), shuf.end(), rng);
    run_case("path forward", rows, fwd, T);
    run_case("path reversed", rows, rev, T);
    run_case("path shuffled", rows, shuf, T);
  }
  // a star whose hub is not the smallest slot, every edge in both directions
  {
    const int32_t rows = 4000, hub = 1234;
    std::vector<Edge> edges;
    for (int32_t i = 0; i < rows; ++i)
      if (i != hub) {
        edges.push_back({hub, i});
        edges.push_back({i, hub});
      }
    std::shuffle(edges.begin(), edges.end(), rng);
    run_case("star", rows, edges, T);
  }
  // every edge five times
  {
    const int32_t rows = 3000;
    std::vector<Edge> edges;
    for (int i = 0; i < 2000; ++i) {
      const Edge e{(int32_t)(rng() % (uint32_t)rows), (int32_t)(rng() % (uint32_t)rows)};
      for (int k = 0; k < 5; ++k) edges.push_back(k % 2 ? Edge{e.second, e.first} : e);
    }
    std::shuffle(edges.begin(), edges.end(), rng);
    run_case("duplicates", rows, edges, T);
  }
  if (fails) std::printf("components selftest: %d FAILED\n", fails);
  else std::printf("components selftest ok (%s)\n", threaded ? "8 threads" : "sequential");
  return fails ? 1 : 0;
}
