// host_remove_selftest.cpp -- removal through the mirrored reference interface: a GpuIndexingWorker whose client withdraws
// vectors (remove) replies what a worker that was never sent them replies; a vector sent again under a removed id is live;
// cpslab.allpair.gpu.autoCompact shrinks the store before the next IndexData; compact() does it on request; a term-sharded
// worker refuses.
// Needs a GPU.  Build: see Makefile in this directory.
#include <cmath>
#include <cstdio>
#include <map>
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

int main() {
  // 96 unit vectors of 3 terms in dim 12 (every query has many neighbours above theta = 0.3), sent as two batches of 48
  const int n = 96, half = 48, dim = 12;
  std::mt19937 rng(23);
  std::vector<std::pair<std::string, SparseVector>> all;
  for (int i = 0; i < n; ++i) {
    int t0 = (int)(rng() % 4), t1 = 4 + (int)(rng() % 4), t2 = 8 + (int)(rng() % 4);
    double a = 0.2 + (rng() % 1000) / 1000.0, b = 0.2 + (rng() % 1000) / 1000.0, c = 0.2 + (rng() % 1000) / 1000.0;
    const double nrm = std::sqrt(a * a + b * b + c * c);
    all.push_back({"v" + std::to_string(i), SparseVector(dim, {t0, t1, t2}, {a / nrm, b / nrm, c / nrm})});
  }
  IndexData first, second, first_live;
  std::set<std::string> gone;
  std::vector<std::string> gone_list;
  for (int i = 0; i < half; ++i) {
    first.vectors.push_back(all[(size_t)i]);
    if (i % 3 == 0) {
      gone.insert(all[(size_t)i].first);
      gone_list.push_back(all[(size_t)i].first);
    } else {
      first_live.vectors.push_back(all[(size_t)i]);
    }
  }
  for (int i = half; i < n; ++i) second.vectors.push_back(all[(size_t)i]);
  gone_list.push_back("never-sent");  // unknown ids are ignored
  gone_list.push_back(gone_list[0]);  // and so are repeated ones

  Config conf;
  conf.similarityThreshold = 0.3;
  conf.vectorDim = dim;
  conf.tileRows = 64;

  // the expectation: a worker that was only ever sent the live vectors
  Reply want;
  {
    std::vector<SimilarityOutput> got;
    GpuIndexingWorker w(conf, [&](const SimilarityOutput &o) { got.push_back(o); });
    w.receive(first_live);
    w.receive(second);
    CHECK(got.size() == 2 && w.lastError().empty());
    if (got.size() == 2) want = got[1].output;
  }
  size_t want_pairs = 0;
  for (auto &q : want) want_pairs += q.second.size();
  CHECK(want_pairs >= 50);

  auto same_reply = [&](const Reply &got) {
    CHECK(got.size() == want.size());
    size_t dropped_seen = 0;
    for (auto &q : got) {
      auto wq = want.find(q.first);
      CHECK(wq != want.end());
      if (wq == want.end()) continue;
      CHECK(q.second.size() == wq->second.size());
      for (auto &c : q.second) {
        dropped_seen += gone.count(c.first);
        auto wc = wq->second.find(c.first);
        // (the two stores differ in their slots, so a pair may be scored by another kernel: fp32 sums of three products)
        CHECK(wc != wq->second.end() && std::fabs(wc->second - c.second) <= 1e-5);
      }
    }
    CHECK(dropped_seen == 0);
  };

  // variant 0: remove, no compaction; 1: remove + compact(); 2: autoCompact = 0.25 (16 of 48 removed: the next IndexData compacts)
  for (int variant = 0; variant < 3; ++variant) {
    Config cf = conf;
    if (variant == 2) cf.autoCompact = 0.25;
    std::vector<SimilarityOutput> got;
    GpuIndexingWorker w(cf, [&](const SimilarityOutput &o) { got.push_back(o); });
    w.receive(first);
    size_t with_gone = 0;
    if (got.size() == 1)
      for (auto &q : got[0].output)
        for (auto &c : q.second) with_gone += gone.count(c.first);
    CHECK(with_gone >= 20);  // there is something to drop
    CHECK(w.remove(gone_list) == (int64_t)gone.size());
    CHECK(w.remove(gone_list) == 0);  // already removed
    CHECK(w.storedVectors() == half && w.liveVectors() == half - (int64_t)gone.size());
    if (variant == 1) {
      CHECK(w.compact());
      CHECK(w.storedVectors() == half - (int64_t)gone.size());
    }
    w.receive(second);
    CHECK(got.size() == 2 && w.lastError().empty());
    if (got.size() == 2) same_reply(got[1].output);
    CHECK(w.storedVectors() == (variant == 0 ? n : n - (int64_t)gone.size()));
    CHECK(w.liveVectors() == n - (int64_t)gone.size());
    // a vector sent again under a removed id is live: its reply names live candidates only, and later queries find it
    IndexData again, probe;
    again.vectors.push_back(all[0]);
    w.receive(again);
    CHECK(got.size() == 3);
    if (got.size() == 3) {
      for (auto &c : got[2].output[all[0].first]) CHECK(gone.count(c.first) == 0);
    }
    probe.vectors.push_back({"probe", all[0].second});
    w.receive(probe);
    CHECK(got.size() == 4);
    if (got.size() == 4) {
      auto &m = got[3].output["probe"];
      CHECK(m.count(all[0].first) == 1 && std::fabs(m[all[0].first] - 1.0) <= 1e-5);
      for (auto &c : m) CHECK(c.first == all[0].first || gone.count(c.first) == 0);
    }
  }

  // a bad fraction fails the worker's construction, as a refused topK does
  {
    Config cf = conf;
    cf.autoCompact = 1.0;
    bool threw = false;
    try {
      GpuIndexingWorker w(cf, nullptr);
    } catch (const std::runtime_error &e) {
      threw = std::string(e.what()).find("apss_set_auto_compact") != std::string::npos;
    }
    CHECK(threw);
  }

  // a term-sharded worker has no removal
  {
    Config cf = conf;
    cf.devices = {0, 0};
    GpuIndexingWorker w(cf, nullptr);
    w.receive(first);
    CHECK(w.remove(gone_list) == -1 && w.lastError().find("term-sharded") != std::string::npos);
    CHECK(!w.compact());
  }

  std::printf(fails ? "host_remove_selftest: %d FAILED\n" : "host_remove_selftest: PASS\n", fails);
  return fails ? 1 : 0;
}
