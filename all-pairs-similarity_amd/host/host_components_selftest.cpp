// host_components_selftest.cpp -- cpslab.allpair.gpu.components through the mirrored reference interface: a GpuIndexingWorker
// with components = true that is sent its vectors in several IndexData messages reports, through groups(), for every live String
// id the representative a union-find over the pairs of its own replies gives (the member stored first); a withdrawn vector leaves
// the map and starts the groups over; a worker without the setting and a term-sharded worker answer an empty map and lastError().
// Needs a GPU.  Build: see Makefile in this directory.
#include <cmath>
#include <cstdio>
#include <map>

#include "../../include/apss.h"
#include "cpslab_host.hpp"

using namespace cpslab;

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                \
    }                                                         \
  } while (0)

int main() {
  // 60 unit vectors in dim 200: vector i has its own two terms, and every third one shares a heavy term with its predecessor, so
  // that chains of a few vectors form above theta = 0.5 while the rest stay alone
  const int n = 60, dim = 200;
  std::vector<IndexData> messages(4);
  std::vector<std::string> order;
  for (int i = 0; i < n; ++i) {
    std::vector<int> t{2 * i, 2 * i + 1};
    std::vector<double> v{0.3, 0.2};
    t.push_back(120 + (i % 3 == 0 ? i / 3 : (i - 1) / 3 + (i % 3 == 2 ? 40 : 0)));  // i = 3k and 3k + 1 share term 120 + k
    v.push_back(0.95);
    double nrm = 0;
    for (double x : v) nrm += x * x;
    for (double &x : v) x /= std::sqrt(nrm);
    const std::string name = "doc" + std::to_string(i);
    messages[(size_t)(i * 4 / n)].vectors.push_back({name, SparseVector(dim, t, v)});
    order.push_back(name);
  }

  Config conf;
  conf.similarityThreshold = 0.5;
  conf.vectorDim = dim;
  conf.tileRows = 64;
  conf.components = true;
  {
    std::vector<SimilarityOutput> got;
    GpuIndexingWorker w(conf, [&](const SimilarityOutput &o) { got.push_back(o); });
    for (const IndexData &m : messages) w.receive(m);
    CHECK(got.size() == messages.size() && w.lastError().empty());
    // the union-find over the replies' pairs, by arrival number; the smallest number represents
    std::map<std::string, int> at;
    for (int i = 0; i < n; ++i) at[order[(size_t)i]] = i;
    std::vector<int> p((size_t)n);
    for (int i = 0; i < n; ++i) p[(size_t)i] = i;
    auto find = [&](int x) {
      while (p[(size_t)x] != x) x = p[(size_t)x] = p[(size_t)p[(size_t)x]];
      return x;
    };
    size_t pairs = 0;
    for (const SimilarityOutput &o : got)
      for (auto &qe : o.output)
        for (auto &ce : qe.second) {
          const int a = find(at[qe.first]), b = find(at[ce.first]);
          if (a != b) p[(size_t)std::max(a, b)] = std::min(a, b);
          ++pairs;
        }
    CHECK(pairs >= 20);  // (the 20 pairs 3k - 3k + 1, at least in one direction)
    const auto groups = w.groups();
    CHECK(groups.size() == (size_t)n && w.lastError().empty());
    int grouped = 0;
    for (int i = 0; i < n; ++i) {
      const auto it = groups.find(order[(size_t)i]);
      CHECK(it != groups.end() && it->second == order[(size_t)find(i)]);
      grouped += find(i) != i;
    }
    CHECK(grouped >= 20);
    // a withdrawn vector is no key any more, and the groups start over: every live vector alone until pairs are seen again
    CHECK(w.remove({"doc0"}) == 1);
    const auto after = w.groups();
    CHECK(after.size() == (size_t)n - 1 && !after.count("doc0"));
    for (auto &kv : after) CHECK(kv.first == kv.second);
    CHECK(w.compact());
    const auto packed = w.groups();
    CHECK(packed.size() == (size_t)n - 1 && !packed.count("doc0") && packed.count("doc59") && packed.at("doc59") == "doc59");
    apss_components_info ci{};
    ci.struct_size = (int32_t)sizeof(ci);
    CHECK(ci.struct_size == 112);
  }

  // off: an empty map and a reason
  {
    Config off = conf;
    off.components = false;
    GpuIndexingWorker w(off, [](const SimilarityOutput &) {});
    w.receive(messages[0]);
    CHECK(w.groups().empty() && w.lastError().find("components") != std::string::npos);
  }

  // a term-sharded worker keeps none: said at construction, and groups() is empty
  {
    Config sharded = conf;
    sharded.devices = {0, 0};
    GpuIndexingWorker w(sharded, [](const SimilarityOutput &) {});
    CHECK(w.lastError().find("components") != std::string::npos);
    w.receive(messages[0]);
    CHECK(w.groups().empty());
  }

  std::printf(fails ? "host_components_selftest: %d FAILED\n" : "host_components_selftest: PASS\n", fails);
  return fails ? 1 : 0;
}
