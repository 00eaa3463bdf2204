// host_query_stored_selftest.cpp -- "what is similar to these vectors that you already hold?" through the mirrored reference
// interface: similarTo(names) on a GpuIndexingWorker that was fed three IndexData batches replies what a worker with the same
// store replies to an IndexData of those vectors once its index is frozen (stopUpdateIndex: a plain apss_query); unknown names
// are ignored; a withdrawn vector is neither asked nor found; a term-sharded worker refuses.
// Needs a GPU.  Build: see Makefile in this directory.
#include <cmath>
#include <cstdio>
#include <random>
#include <set>

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

using Reply = std::unordered_map<std::string, std::unordered_map<std::string, double>>;

static size_t pairs_of(const Reply &r) {
  size_t n = 0;
  for (auto &q : r) n += q.second.size();
  return n;
}

static void same_reply(const Reply &got, const Reply &want) {
  CHECK(got.size() == want.size());
  for (auto &q : got) {
    auto wq = want.find(q.first);
    CHECK(wq != want.end());
    if (wq == want.end()) continue;
    CHECK(q.second.size() == wq->second.size());
    for (auto &c : q.second) {
      auto wc = wq->second.find(c.first);
      CHECK(wc != wq->second.end() && std::fabs(wc->second - c.second) <= 1e-5);
    }
  }
}

int main() {
  // 96 unit vectors of 3 terms in dim 12 (every query has many neighbours above theta = 0.3), sent as three batches of 32
  const int n = 96, third = 32, dim = 12;
  std::mt19937 rng(29);
  std::vector<std::pair<std::string, SparseVector>> all;
  for (int i = 0; i < n; ++i) {
    int t0 = (int)(rng() % 4), t1 = 4 + (int)(rng() % 4), t2 = 8 + (int)(rng() % 4);
    double a = 0.2 + (rng() % 1000) / 1000.0, b = 0.2 + (rng() % 1000) / 1000.0, c = 0.2 + (rng() % 1000) / 1000.0;
    const double nrm = std::sqrt(a * a + b * b + c * c);
    all.push_back({"v" + std::to_string(i), SparseVector(dim, {t0, t1, t2}, {a / nrm, b / nrm, c / nrm})});
  }
  IndexData batches[3], asked;
  for (int i = 0; i < n; ++i) batches[i / third].vectors.push_back(all[(size_t)i]);
  std::vector<std::string> names;
  for (int i = 0; i < n; i += 5) {  // vectors of all three batches
    names.push_back(all[(size_t)i].first);
    asked.vectors.push_back(all[(size_t)i]);
  }
  std::vector<std::string> names_noise = names;
  names_noise.push_back("never-sent");      // unknown names are ignored
  names_noise.push_back(names[0]);          // and a repeated one asks nothing more
  names_noise.insert(names_noise.begin(), "also-never-sent");

  Config conf;
  conf.similarityThreshold = 0.3;
  conf.vectorDim = dim;
  conf.tileRows = 64;

  // the expectation: the same store, frozen, asked with the vectors themselves
  Reply want;
  {
    std::vector<SimilarityOutput> got;
    GpuIndexingWorker w(conf, [&](const SimilarityOutput &o) { got.push_back(o); });
    for (auto &b : batches) w.receive(b);
    w.receiveTimeout();
    w.receive(asked);
    CHECK(got.size() == 4 && w.lastError().empty() && w.storedVectors() == n);
    if (got.size() == 4) want = got[3].output;
  }
  CHECK(want.size() == names.size() && pairs_of(want) >= 50);

  {
    std::vector<SimilarityOutput> got;
    GpuIndexingWorker w(conf, [&](const SimilarityOutput &o) { got.push_back(o); });
    for (auto &b : batches) w.receive(b);
    const SimilarityOutput a = w.similarTo(names);
    CHECK(w.lastError().empty());
    same_reply(a.output, want);
    same_reply(w.similarTo(names_noise).output, want);
    CHECK(w.lastError().empty() && w.storedVectors() == n && got.size() == 3);  // nothing was inserted, nothing was replied
    CHECK(w.similarTo({}).output.empty() && w.similarTo({"never-sent"}).output.empty() && w.lastError().empty());
    // the worker goes on as before: the next batch sees the whole store
    IndexData again;
    again.vectors.push_back({"probe", all[0].second});
    w.receive(again);
    CHECK(got.size() == 4 && w.storedVectors() == n + 1);
    if (got.size() == 4) CHECK(got[3].output["probe"].count(all[0].first) == 1);
    // a withdrawn vector is neither asked nor found
    CHECK(w.remove({names[0], "probe"}) == 2);
    const SimilarityOutput b = w.similarTo(names);
    CHECK(w.lastError().empty() && b.output.size() == names.size());
    auto gone = b.output.find(names[0]);
    CHECK(gone != b.output.end() && gone->second.empty());
    for (auto &q : b.output) {
      CHECK(q.second.count(names[0]) == 0 && q.second.count("probe") == 0);
      if (q.first == names[0]) continue;
      auto wq = want.find(q.first);
      CHECK(wq != want.end());
      if (wq != want.end()) CHECK(q.second.size() == wq->second.size() - wq->second.count(names[0]));
    }
  }

  // a term-sharded worker holds slices of vectors
  {
    Config cf = conf;
    cf.devices = {0, 0};
    GpuIndexingWorker w(cf, nullptr);
    w.receive(batches[0]);
    CHECK(w.similarTo(names).output.empty() && w.lastError().find("term-sharded") != std::string::npos);
  }

  std::printf(fails ? "host_query_stored_selftest: %d FAILED\n" : "host_query_stored_selftest: PASS\n", fails);
  return fails ? 1 : 0;
}
