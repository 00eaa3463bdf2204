// host_topk_selftest.cpp -- cpslab.allpair.gpu.topK through the mirrored reference interface: a GpuIndexingWorker with
// topK = 2 replies inner maps of at most two candidates, the ones a plain handle with apss_set_top_k(2) reports for the same
// rows; a term-sharded worker does the same behind its exchange; so does a worker with topKWindowPairs set (the cut in windows
// of query rows); a worker with topKTileCut at similarityThreshold = 0 replies what the one without it does (the cut inside the
// probe kernel); a grid refuses and keeps answering with every pair.
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
  // 48 unit vectors of 3 terms in dim 12: every query has many neighbours above theta = 0.1
  const int n = 48, dim = 12, k = 2;
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
    std::printf("host_topk_selftest: no handle (%s)\n", apss_last_error(nullptr));
    return 1;
  }
  CHECK(apss_set_top_k(h, APSS_TOP_K_MAX + 1) == APSS_E_INVALID);
  CHECK(apss_set_top_k(h, k) == APSS_OK);
  int64_t n_res = 0;
  CHECK(apss_insert_and_query(h, n, rowptr.data(), idx.data(), val.data(), ids.data(), &n_res) == APSS_OK);
  std::vector<int64_t> q((size_t)n_res), cc((size_t)n_res);
  std::vector<float> s((size_t)n_res);
  if (n_res) CHECK(apss_fetch_results(h, 0, n_res, q.data(), cc.data(), s.data()) == APSS_OK);
  apss_topk_info ti{};
  ti.struct_size = (int32_t)sizeof(ti);
  CHECK(apss_topk_get(h, &ti) == APSS_OK && ti.k == k && ti.kept == n_res && ti.pairs_over_theta > n_res && ti.queries_cut > 0);
  std::map<std::string, std::map<std::string, double>> want;
  for (int64_t i = 0; i < n_res; ++i) want["v" + std::to_string(q[(size_t)i])]["v" + std::to_string(cc[(size_t)i])] = (double)s[(size_t)i];
  apss_destroy(h);

  // one handle; two term shards sharing GPU 0; one member with the exchange forced; one handle cutting in windows of query rows
  // (cpslab.allpair.gpu.topKWindowPairs = 100 < 48 x 48: the same maps, bit for bit)
  for (int variant = 0; variant < 4; ++variant) {
    Config conf;
    conf.similarityThreshold = 0.1;
    conf.vectorDim = dim;
    conf.tileRows = 64;
    conf.topK = k;
    if (variant == 1) conf.devices = {0, 0};
    if (variant == 2) { conf.devices = {0}; conf.groupFlags = 1u; }
    if (variant == 3) conf.topKWindowPairs = 100;
    std::vector<SimilarityOutput> got;
    GpuIndexingWorker w(conf, [&](const SimilarityOutput &o) { got.push_back(o); });
    w.receive(batch);
    CHECK(got.size() == 1 && w.lastError().empty());
    if (got.size() != 1) continue;
    size_t pairs = 0;
    for (auto &qe : got[0].output) {
      CHECK(qe.second.size() <= (size_t)k);
      pairs += qe.second.size();
      for (auto &ce : qe.second) {
        // the term-sharded sums may differ from the plain handle's in the last bits: compare the candidate when the scores
        // are clearly apart, the score always
        auto wq = want.find(qe.first);
        CHECK(wq != want.end());
        if (wq == want.end()) continue;
        auto wc = wq->second.find(ce.first);
        if (variant == 0 || variant == 3) CHECK(wc != wq->second.end() && wc->second == ce.second);
        else if (wc != wq->second.end()) CHECK(std::fabs(wc->second - ce.second) <= 1e-5);
        else {
          double lowest = 2.0;
          for (auto &x : wq->second) lowest = std::min(lowest, x.second);
          CHECK(std::fabs(lowest - ce.second) <= 2e-5);  // only a tie at the cut may pick another candidate
        }
      }
    }
    CHECK(pairs == (size_t)n_res);
  }

  // cpslab.allpair.gpu.topKTileCut at similarityThreshold = 0 (the reference's shipped value, where the probe's rounds are cut
  // before they are written): the same maps as the worker without it, bit for bit -- and more candidates than topK to cut from
  {
    std::vector<SimilarityOutput> got[2];
    for (int cut = 0; cut < 2; ++cut) {
      Config conf;
      conf.similarityThreshold = 0.0;
      conf.vectorDim = dim;
      conf.tileRows = 64;
      conf.topK = k;
      conf.topKTileCut = cut == 1;
      GpuIndexingWorker w(conf, [&](const SimilarityOutput &o) { got[cut].push_back(o); });
      w.receive(batch);
      CHECK(got[cut].size() == 1 && w.lastError().empty());
    }
    if (got[0].size() == 1 && got[1].size() == 1) {
      CHECK(got[0][0].output == got[1][0].output);
      size_t pairs = 0;
      for (auto &qe : got[1][0].output) pairs += qe.second.size();
      CHECK(pairs == (size_t)n * (size_t)k);
    }
  }

  // a grid does not support it: reported through lastError(), the worker answers with every pair
  {
    Config conf;
    conf.similarityThreshold = 0.1;
    conf.vectorDim = dim;
    conf.tileRows = 64;
    conf.topK = k;
    conf.devices = {0, 0};
    conf.rowRanges = 2;
    std::vector<SimilarityOutput> got;
    GpuIndexingWorker w(conf, [&](const SimilarityOutput &o) { got.push_back(o); });
    CHECK(w.lastError().find("topK") != std::string::npos);
    w.receive(batch);
    CHECK(got.size() == 1);
    size_t pairs = 0;
    if (got.size() == 1)
      for (auto &qe : got[0].output) pairs += qe.second.size();
    CHECK((int64_t)pairs == ti.pairs_over_theta);
  }

  std::printf(fails ? "host_topk_selftest: %d FAILED\n" : "host_topk_selftest: PASS\n", fails);
  return fails ? 1 : 0;
}
