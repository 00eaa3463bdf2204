// host_top_pairs_selftest.cpp -- cpslab.allpair.gpu.topPairs through the mirrored reference interface: a GpuIndexingWorker with
// topPairs = 5 replies maps that hold exactly the five pairs a plain handle with apss_set_top_pairs(5) reports for the same rows,
// in the handle's rank order (score descending); a bad value fails the worker's construction; a term-sharded worker reports the
// setting through lastError() and answers with every pair.
// Needs a GPU.  Build: see Makefile in this directory.
#include <cmath>
#include <cstdio>
#include <map>
#include <random>

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
  // 48 unit vectors of 3 terms in dim 12: hundreds of pairs above theta = 0.1
  const int n = 48, dim = 12;
  const int64_t K = 5;
  std::mt19937 rng(11);
  IndexData batch;
  std::vector<int64_t> rowptr{0}, ids;
  std::vector<int32_t> idx;
  std::vector<double> val;
  for (int i = 0; i < n; ++i) {
    int t0 = (int)(rng() % 4), t1 = 4 + (int)(rng() % 4), t2 = 8 + (int)(rng() % 4);
    double a = 0.2 + (rng() % 1000) / 1000.0, b = 0.2 + (rng() % 1000) / 1000.0, c = 0.2 + (rng() % 1000) / 1000.0;
    const double nrm = std::sqrt(a * a + b * b + c * c);
    a /= nrm, b /= nrm, c /= nrm;
    batch.vectors.push_back({"v" + std::to_string(i), SparseVector(dim, {t0, t1, t2}, {a, b, c})});
    ids.push_back(i);  // the worker numbers its String ids in arrival order
    for (int t : {t0, t1, t2}) idx.push_back(t);
    for (double v : {a, b, c}) val.push_back(v);
    rowptr.push_back((int64_t)idx.size());
  }

  // the handle's own list for the same rows
  apss_config c{};
  c.struct_size = (int32_t)sizeof(c);
  c.dim = dim;
  c.theta = 0.1;
  c.tile_rows = 64;
  apss_handle *h = nullptr;
  CHECK(apss_create(&c, &h) == APSS_OK);
  if (!h) {
    std::printf("host_top_pairs_selftest: no handle (%s)\n", apss_last_error(nullptr));
    return 1;
  }
  CHECK(apss_set_top_pairs(h, -1) == APSS_E_INVALID);
  CHECK(apss_set_top_pairs(h, (int64_t)APSS_TOP_PAIRS_MAX + 1) == APSS_E_INVALID);
  CHECK(apss_set_top_pairs(h, K) == APSS_OK);
  int64_t n_res = 0;
  CHECK(apss_insert_and_query(h, n, rowptr.data(), idx.data(), val.data(), ids.data(), &n_res) == APSS_OK);
  CHECK(n_res == K);
  std::vector<int64_t> q((size_t)n_res), cc((size_t)n_res);
  std::vector<float> s((size_t)n_res);
  if (n_res) CHECK(apss_fetch_results(h, 0, n_res, q.data(), cc.data(), s.data()) == APSS_OK);
  apss_top_pairs_info ti{};
  ti.struct_size = (int32_t)sizeof(ti);
  CHECK(apss_top_pairs_get(h, &ti) == APSS_OK && ti.k_pairs == K && ti.kept == K && ti.pairs_in > K && ti.launches > 0 &&
        ti.above + ti.tied_kept == K && ti.tied >= ti.tied_kept);
  for (int64_t i = 0; i + 1 < n_res; ++i) CHECK(s[(size_t)i] >= s[(size_t)i + 1]);  // rank order
  if (n_res) CHECK((double)s[(size_t)n_res - 1] == ti.kth_score);
  std::map<std::string, std::map<std::string, double>> want;
  for (int64_t i = 0; i < n_res; ++i) want["v" + std::to_string(q[(size_t)i])]["v" + std::to_string(cc[(size_t)i])] = (double)s[(size_t)i];
  const int64_t all_pairs = ti.pairs_in;
  apss_destroy(h);

  // the worker: the same five pairs and nothing else
  {
    Config conf;
    conf.similarityThreshold = 0.1;
    conf.vectorDim = dim;
    conf.tileRows = 64;
    conf.topPairs = K;
    std::vector<SimilarityOutput> got;
    GpuIndexingWorker w(conf, [&](const SimilarityOutput &o) { got.push_back(o); });
    w.receive(batch);
    CHECK(got.size() == 1 && w.lastError().empty());
    if (got.size() == 1) {
      std::map<std::string, std::map<std::string, double>> have;
      for (auto &qe : got[0].output)
        for (auto &ce : qe.second) have[qe.first][ce.first] = ce.second;
      CHECK(have == want);
    }
  }

  // a bad value fails construction, as a refused topK does
  for (long bad : {-1L, (long)APSS_TOP_PAIRS_MAX + 1}) {
    Config conf;
    conf.similarityThreshold = 0.1;
    conf.vectorDim = dim;
    conf.topPairs = bad;
    bool threw = false;
    try {
      GpuIndexingWorker w(conf, [](const SimilarityOutput &) {});
    } catch (const std::runtime_error &e) {
      threw = std::string(e.what()).find("apss_set_top_pairs") != std::string::npos;
    }
    CHECK(threw);
  }

  // a term-sharded worker has no global cut: reported through lastError(), every pair is answered
  {
    Config conf;
    conf.similarityThreshold = 0.1;
    conf.vectorDim = dim;
    conf.tileRows = 64;
    conf.topPairs = K;
    conf.devices = {0, 0};
    std::vector<SimilarityOutput> got;
    GpuIndexingWorker w(conf, [&](const SimilarityOutput &o) { got.push_back(o); });
    CHECK(w.lastError().find("topPairs") != std::string::npos);
    w.receive(batch);
    CHECK(got.size() == 1);
    size_t pairs = 0;
    if (got.size() == 1)
      for (auto &qe : got[0].output) pairs += qe.second.size();
    CHECK((int64_t)pairs == all_pairs);
  }

  std::printf(fails ? "host_top_pairs_selftest: %d FAILED\n" : "host_top_pairs_selftest: PASS\n", fails);
  return fails ? 1 : 0;
}
