// cpslab_host.cpp -- see cpslab_host.hpp.  Pure host code over the C ABI (include/apss.h); links libapss_hip.so.
#include "cpslab_host.hpp"

#include <fstream>
#include <iterator>
#include <map>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <sstream>
#include <unordered_set>

#include "../../include/apss.h"

namespace cpslab {

SparseVector::SparseVector(int size_, std::vector<int32_t> idx, std::vector<double> val)
    : size(size_), indices(std::move(idx)), values(std::move(val)) {
  if (indices.size() != values.size()) throw std::invalid_argument("requirement failed");  // SparseVector.scala:202
}

std::string SparseVector::toString() const {
  std::ostringstream o;
  o.precision(17);
  o << "(" << size << ",[";
  for (size_t i = 0; i < indices.size(); ++i) o << (i ? "," : "") << indices[i];
  o << "],[";
  for (size_t i = 0; i < values.size(); ++i) o << (i ? "," : "") << values[i];
  o << "])";
  return o.str();
}

SparseVector SparseVector::fromString(const std::string &s) {
  // inputString.split(",\\[") must give 3 pieces (SparseVector.scala:133-136)
  const size_t p1 = s.find(",[");
  const size_t p2 = p1 == std::string::npos ? p1 : s.find(",[", p1 + 2);
  if (p1 == std::string::npos || p2 == std::string::npos || s.find(",[", p2 + 2) != std::string::npos)
    throw std::runtime_error("cannot parse " + s);
  auto strip = [](std::string t, const char *drop) {
    for (const char *d = drop; *d; ++d) t.erase(std::remove(t.begin(), t.end(), *d), t.end());
    return t;
  };
  SparseVector v;
  v.size = std::stoi(strip(s.substr(0, p1), "("));
  std::stringstream is(strip(s.substr(p1 + 2, p2 - p1 - 2), "]")), vs(strip(s.substr(p2 + 2), "])"));
  std::string tok;
  while (std::getline(is, tok, ',')) if (!tok.empty()) v.indices.push_back(std::stoi(tok));
  while (std::getline(vs, tok, ',')) if (!tok.empty()) v.values.push_back(std::stod(tok));
  if (v.indices.size() != v.values.size()) throw std::invalid_argument("requirement failed");
  return v;
}

std::pair<std::string, SparkSparseVector> CCWEBVideoLoadGenerator::lineParser(const std::string &line) {
  // line.replace("(", "").replace(")", "").replace("[", "").replace("]", "").split(",")  (CCW:11-12); String.split drops
  // trailing empty strings
  std::string t;
  for (char ch : line)
    if (ch != '(' && ch != ')' && ch != '[' && ch != ']') t.push_back(ch);
  std::vector<std::string> f;
  size_t b = 0;
  for (;;) {
    const size_t e = t.find(',', b);
    f.push_back(t.substr(b, e == std::string::npos ? e : e - b));
    if (e == std::string::npos) break;
    b = e + 1;
  }
  while (!f.empty() && f.back().empty()) f.pop_back();
  if (f.size() < 2) throw std::invalid_argument("CC_WEB_VIDEO line without id and size: " + line);
  auto to_int = [&](const std::string &s) {
    size_t used = 0;
    int v = 0;
    try { v = std::stoi(s, &used); } catch (const std::exception &) { used = std::string::npos; }
    if (used != s.size() || s.empty()) throw std::invalid_argument("not an Int: '" + s + "'");
    return v;
  };
  auto to_double = [&](const std::string &s) {
    size_t used = 0;
    double v = 0;
    try { v = std::stod(s, &used); } catch (const std::exception &) { used = std::string::npos; }
    if (used != s.size() || s.empty()) throw std::invalid_argument("not a Double: '" + s + "'");
    return v;
  };
  const int size = to_int(f[1]);  // propertyArray(1).toInt
  if (size < 0) throw std::invalid_argument("negative vector size");
  // propertyArray.takeRight(vectorSize): the last `size` fields (all of them when there are fewer -- allValues(i) then
  // fails for i past the end, CCW:17)
  if ((size_t)size > f.size()) throw std::invalid_argument("fewer than `size` values: " + line);
  std::vector<int32_t> idx;
  std::vector<double> val;
  for (int i = 0; i < size; ++i) {
    const double v = to_double(f[f.size() - (size_t)size + (size_t)i]);
    if (v != 0) {  // allValues(_) != 0
      idx.push_back(i);
      val.push_back(v);
    }
  }
  return {f[0], SparseVector(size, std::move(idx), std::move(val))};
}

std::vector<std::pair<std::string, SparkSparseVector>> CCWEBVideoLoadGenerator::generateVectors() const {
  std::ifstream in(path_);
  if (!in) throw std::runtime_error("cannot open " + path_);  // Source.fromFile: FileNotFoundException
  std::vector<std::pair<std::string, SparkSparseVector>> out;
  std::string line;
  while (std::getline(in, line)) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    out.push_back(lineParser(line));
  }
  return out;
}

namespace etl {
int32_t javaStringHashCode(const std::string &s) {
  uint32_t h = 0;
  for (unsigned char ch : s) h = 31u * h + ch;
  return (int32_t)h;
}

int32_t nonNegativeMod(int32_t x, int32_t mod) {
  const int32_t r = x % mod;  // truncated, like the JVM's %
  return r < 0 ? r + mod : r;
}

std::vector<std::string> documentTokens(const std::string &path) {
  std::ifstream in(path, std::ios::binary);
  if (!in) throw std::runtime_error("cannot open " + path);
  std::string raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  // BufferedReader.readLine: "\n", "\r" and "\r\n" end a line; a final terminator does not start another line
  std::string s;
  size_t i = 0;
  while (i < raw.size()) {
    size_t j = i;
    while (j < raw.size() && raw[j] != '\n' && raw[j] != '\r') ++j;
    s.append(raw, i, j - i);
    s.push_back(' ');
    if (j < raw.size() && raw[j] == '\r' && j + 1 < raw.size() && raw[j + 1] == '\n') ++j;
    i = j + 1;
  }
  s += "null ";
  std::vector<std::string> toks;
  size_t b = 0;
  for (;;) {
    const size_t e = s.find(' ', b);
    toks.push_back(s.substr(b, e == std::string::npos ? e : e - b));
    if (e == std::string::npos) break;
    b = e + 1;
  }
  while (!toks.empty() && toks.back().empty()) toks.pop_back();  // String.split drops trailing empty strings
  return toks;
}

SparseVector hashingTF(const std::vector<std::string> &tokens, int32_t numFeatures) {
  std::map<int32_t, double> tf;
  for (const auto &t : tokens) tf[nonNegativeMod(javaStringHashCode(t), numFeatures)] += 1.0;
  std::vector<int32_t> idx;
  std::vector<double> val;
  for (const auto &kv : tf) {
    idx.push_back(kv.first);
    val.push_back(kv.second);
  }
  return SparseVector(numFeatures, std::move(idx), std::move(val));
}

std::vector<SparseVector> tfidf(const std::vector<SparseVector> &tf, bool normalize) {
  std::map<int32_t, int64_t> df;
  for (const auto &v : tf)
    for (int32_t i : v.indices) ++df[i];
  const double m = (double)tf.size();
  std::vector<SparseVector> out;
  for (const auto &v : tf) {
    std::vector<double> w(v.values.size());
    double ss = 0;
    for (size_t k = 0; k < w.size(); ++k) {
      w[k] = v.values[k] * std::log((m + 1.0) / ((double)df[v.indices[k]] + 1.0));
      ss += w[k] * w[k];
    }
    if (normalize && ss > 0) {
      const double nrm = std::sqrt(ss);
      for (double &x : w) x /= nrm;
    }
    out.emplace_back(v.size, v.indices, std::move(w));
  }
  return out;
}
}  // namespace etl

std::string SimilarityOutput::toString() const {  // Message.scala:23-34
  std::ostringstream o;
  for (const auto &q : output) {
    o << "---------------------------------" << q.first << ":";
    for (const auto &c : q.second) o << c.first << "," << c.second << ";";
    o << "\n";
  }
  return o.str();
}

static int64_t now_ms() {
  return std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::system_clock::now().time_since_epoch()).count();
}

GpuIndexingWorker::GpuIndexingWorker(const Config &conf, ReplyTo replyTo) : conf_(conf), reply_to_(std::move(replyTo)) {
  apss_config c{};
  c.struct_size = (int32_t)sizeof(c);
  c.dim = conf.vectorDim;
  c.theta = conf.similarityThreshold;
  c.index_threshold = conf.indexThreshold;
  c.flags = conf.applyIndexThreshold ? APSS_FLAG_VALUE_PRUNE : 0u;
  c.device_id = conf.deviceId;
  c.tile_rows = conf.tileRows;
  c.head_terms = conf.headTerms;
  if (conf.devices.size() > 1 || conf.groupFlags) {
    // the term-sharded index of the node behind one object: the reference's DataPacket fan-out to its term workers
    // (WriteWorkerActor.scala:164-183, EntryProxyActor.scala:37-49) happens inside the library
    std::vector<int32_t> dev(conf.devices.begin(), conf.devices.end());
    if (dev.empty()) dev.push_back(conf.deviceId);
    const int32_t D = conf.rowRanges;
    if (D < 1 || dev.size() % (size_t)D) throw std::runtime_error("rowRanges must divide the number of devices");
    const int32_t rc = D == 1 ? apss_group_create(&c, (int32_t)dev.size(), dev.data(), conf.groupFlags, &g_)
                              : apss_group_create_grid(&c, (int32_t)dev.size() / D, D, dev.data(), conf.groupFlags, &g_);
    if (rc != APSS_OK) throw std::runtime_error(std::string("apss_group_create: ") + apss_group_last_error(nullptr));
    if (conf.topK != 0) {
      const int32_t rk = apss_group_set_top_k(g_, conf.topK);
      if (rk == APSS_E_UNSUPPORTED) {  // a grid: the worker keeps answering with every pair
        last_error_ = std::string("cpslab.allpair.gpu.topK ignored: ") + apss_group_last_error(g_);
        conf_.topK = 0;
      } else if (rk != APSS_OK) {
        const std::string msg = std::string("apss_group_set_top_k: ") + apss_group_last_error(g_);
        apss_group_destroy(g_);
        g_ = nullptr;
        throw std::runtime_error(msg);
      }
    }
    if (conf.topPairs != 0) {  // a group's list lies behind its exchange: no global cut there
      last_error_ = "cpslab.allpair.gpu.topPairs ignored: a term-sharded worker has no global top-K (apss_set_top_pairs: plain handles only)";
      conf_.topPairs = 0;
    }
    if (conf.components) {  // a group's list lies behind its exchange: no stage there
      last_error_ = "cpslab.allpair.gpu.components ignored: a term-sharded worker keeps no components (apss_set_components: plain handles only)";
      conf_.components = false;
    }
    if (conf.componentsRepairRows != 0) {
      last_error_ = "cpslab.allpair.gpu.componentsRepairRows ignored: a term-sharded worker keeps no components (apss_set_components_repair: plain handles only)";
      conf_.componentsRepairRows = 0;
    }
    return;
  }
  if (conf.devices.size() == 1) c.device_id = conf.devices[0];
  const int32_t rc = apss_create(&c, &h_);
  if (rc != APSS_OK) throw std::runtime_error(std::string("apss_create: ") + apss_last_error(nullptr));
  if (conf.topKWindowPairs != 0 && apss_set_top_k_window(h_, conf.topKWindowPairs) != APSS_OK) {
    const std::string msg = std::string("apss_set_top_k_window: ") + apss_last_error(h_);
    apss_destroy(h_);
    h_ = nullptr;
    throw std::runtime_error(msg);
  }
  if (conf.topKTileCut && apss_set_top_k_tile_cut(h_, 1) != APSS_OK) {
    const std::string msg = std::string("apss_set_top_k_tile_cut: ") + apss_last_error(h_);
    apss_destroy(h_);
    h_ = nullptr;
    throw std::runtime_error(msg);
  }
  if (conf.topK != 0 && apss_set_top_k(h_, conf.topK) != APSS_OK) {
    const std::string msg = std::string("apss_set_top_k: ") + apss_last_error(h_);
    apss_destroy(h_);
    h_ = nullptr;
    throw std::runtime_error(msg);
  }
  if (conf.topPairs != 0 && apss_set_top_pairs(h_, conf.topPairs) != APSS_OK) {
    const std::string msg = std::string("apss_set_top_pairs: ") + apss_last_error(h_);
    apss_destroy(h_);
    h_ = nullptr;
    throw std::runtime_error(msg);
  }
  if (conf.components && apss_set_components(h_, 1) != APSS_OK) {
    const std::string msg = std::string("apss_set_components: ") + apss_last_error(h_);
    apss_destroy(h_);
    h_ = nullptr;
    throw std::runtime_error(msg);
  }
  if (conf.componentsRepairRows != 0 && apss_set_components_repair(h_, conf.componentsRepairRows) != APSS_OK) {
    const std::string msg = std::string("apss_set_components_repair: ") + apss_last_error(h_);
    apss_destroy(h_);
    h_ = nullptr;
    throw std::runtime_error(msg);
  }
  if (conf.autoCompact != 0.0 && apss_set_auto_compact(h_, conf.autoCompact) != APSS_OK) {
    const std::string msg = std::string("apss_set_auto_compact: ") + apss_last_error(h_);
    apss_destroy(h_);
    h_ = nullptr;
    throw std::runtime_error(msg);
  }
}

int64_t GpuIndexingWorker::remove(const std::vector<std::string> &ids) {
  if (g_) {
    last_error_ = "remove: a term-sharded worker has no removal (cpslab.allpair.gpu.devices with one entry)";
    return -1;
  }
  std::vector<int64_t> ext;
  for (const std::string &s : ids) {
    const auto it = id_of_.find(s);
    if (it != id_of_.end()) ext.push_back(it->second);
  }
  int64_t removed = 0;
  if (apss_remove(h_, (int64_t)ext.size(), ext.data(), &removed) != APSS_OK) {
    last_error_ = std::string("apss_remove: ") + apss_last_error(h_);
    return -1;
  }
  if (conf_.components && removed > 0) {  // (every live slot under one of the ids is marked: apss_remove)
    const std::unordered_set<int64_t> gone(ext.begin(), ext.end());
    for (size_t s = 0; s < slot_id_.size(); ++s)
      if (gone.count(slot_id_[s])) slot_dead_[s] = 1;
  }
  return removed;
}

bool GpuIndexingWorker::compact() {
  if (g_) {
    last_error_ = "compact: a term-sharded worker has no removal (cpslab.allpair.gpu.devices with one entry)";
    return false;
  }
  if (apss_compact(h_) != APSS_OK) {
    last_error_ = std::string("apss_compact: ") + apss_last_error(h_);
    return false;
  }
  drop_dead_slots();
  return true;
}

int64_t GpuIndexingWorker::compactions() const {
  apss_removal_info ri{};
  ri.struct_size = (int32_t)sizeof(ri);
  return h_ && apss_removal_get(h_, &ri) == APSS_OK ? ri.compactions : 0;
}

// a compaction moved the live rows to the front, in slot order
void GpuIndexingWorker::drop_dead_slots() {
  size_t live = 0;
  for (size_t s = 0; s < slot_id_.size(); ++s)
    if (!slot_dead_[s]) slot_id_[live++] = slot_id_[s];
  slot_id_.resize(live);
  slot_dead_.assign(live, 0);
}

std::unordered_map<std::string, std::string> GpuIndexingWorker::groups() {
  std::unordered_map<std::string, std::string> out;
  if (g_ || !conf_.components) {
    last_error_ = g_ ? "groups: a term-sharded worker keeps no components (cpslab.allpair.gpu.devices with one entry)"
                     : "groups: cpslab.allpair.gpu.components is off";
    return out;
  }
  const int64_t rows = storedVectors();
  if (!slots_known_ || rows != (int64_t)slot_id_.size()) {
    last_error_ = "groups: the store holds other rows than the worker sent (a vector was not admitted)";
    return out;
  }
  std::vector<int32_t> label((size_t)rows);
  std::vector<int64_t> rep((size_t)rows);
  if (apss_components_fetch(h_, 0, rows, label.data(), rep.data()) != APSS_OK) {
    last_error_ = std::string("apss_components_fetch: ") + apss_last_error(h_);
    return out;
  }
  for (int64_t s = 0; s < rows; ++s)
    if (label[(size_t)s] >= 0) out[name_of_[(size_t)slot_id_[(size_t)s]]] = name_of_[(size_t)rep[(size_t)s]];
  return out;
}

SimilarityOutput GpuIndexingWorker::similarTo(const std::vector<std::string> &ids) {
  SimilarityOutput out;
  out.outputMoment = now_ms();
  if (g_) {
    last_error_ = "similarTo: a term-sharded worker holds slices of vectors (cpslab.allpair.gpu.devices with one entry)";
    return out;
  }
  std::vector<int64_t> ext;
  for (const std::string &s : ids) {
    const auto it = id_of_.find(s);
    if (it != id_of_.end()) ext.push_back(it->second);
  }
  int64_t n_rows = 0, n_res = 0;
  if (apss_query_stored(h_, (int64_t)ext.size(), ext.data(), &n_rows, &n_res) != APSS_OK) {
    last_error_ = std::string("apss_query_stored: ") + apss_last_error(h_);
    return out;
  }
  std::vector<int64_t> q((size_t)n_res), c((size_t)n_res);
  std::vector<float> s((size_t)n_res);
  if (n_res && apss_fetch_results(h_, 0, n_res, q.data(), c.data(), s.data()) != APSS_OK) {
    last_error_ = std::string("apss_fetch_results: ") + apss_last_error(h_);
    return out;
  }
  // every known name gets an entry, possibly empty (as handle() gives every query one; IndexingWorkerActor.scala:106-107)
  for (const int64_t id : ext) out.output[name_of_[(size_t)id]];
  for (int64_t i = 0; i < n_res; ++i) out.output[name_of_[(size_t)q[i]]][name_of_[(size_t)c[i]]] = (double)s[i];
  out.outputMoment = now_ms();
  return out;
}

int64_t GpuIndexingWorker::liveVectors() const {
  if (g_) return storedVectors();
  apss_removal_info ri{};
  ri.struct_size = (int32_t)sizeof(ri);
  return apss_removal_get(h_, &ri) == APSS_OK ? ri.rows_live : storedVectors();
}

GpuIndexingWorker::~GpuIndexingWorker() {
  if (g_) apss_group_destroy(g_);
  else apss_destroy(h_);
}

int64_t GpuIndexingWorker::storedVectors() const {
  int64_t rows = 0;
  if (g_) {
    apss_group_stats st{};
    st.struct_size = (int32_t)sizeof(st);
    if (apss_group_stats_get(g_, &st) == APSS_OK) rows = st.rows;
  } else {
    apss_size(h_, &rows, nullptr);
  }
  return rows;
}

SimilarityOutput GpuIndexingWorker::handle(const IndexData &m) {
  // flatten the batch to CSR; every vector's size must equal vectorDim (the require of CommonUtils.scala:99)
  std::vector<int64_t> rowptr{0}, ids;
  std::vector<int32_t> idx;
  std::vector<double> val;
  for (const auto &kv : m.vectors) {
    const SparseVector &v = kv.second;
    if (v.size != conf_.vectorDim)
      throw std::invalid_argument("requirement failed: vector1 size: " + std::to_string(v.size) + ", vector2 size: " +
                                  std::to_string(conf_.vectorDim));
    auto it = id_of_.find(kv.first);
    if (it == id_of_.end()) {
      it = id_of_.emplace(kv.first, (int64_t)name_of_.size()).first;
      name_of_.push_back(kv.first);
    }
    ids.push_back(it->second);
    idx.insert(idx.end(), v.indices.begin(), v.indices.end());
    val.insert(val.end(), v.values.begin(), v.values.end());
    rowptr.push_back((int64_t)idx.size());
  }
  int64_t n_res = 0;
  const int64_t n = (int64_t)ids.size();
  const bool track = conf_.components && !g_ && !stop_update_index_;  // (groups(): which id went to which slot)
  const int64_t rows_before = track ? storedVectors() : 0, compactions_before = track ? compactions() : 0;
  int32_t rc;
  if (g_)
    rc = stop_update_index_  // IndexingWorkerActor.scala:125-133
             ? apss_group_query(g_, n, rowptr.data(), idx.data(), val.data(), ids.data(), &n_res)
             : apss_group_insert_and_query(g_, n, rowptr.data(), idx.data(), val.data(), ids.data(), &n_res);
  else
    rc = stop_update_index_
             ? apss_query(h_, n, rowptr.data(), idx.data(), val.data(), ids.data(), &n_res)
             : apss_insert_and_query(h_, n, rowptr.data(), idx.data(), val.data(), ids.data(), &n_res);
  if (track) {
    const bool compacted = compactions() > compactions_before;  // (apss_set_auto_compact, before the batch was stored)
    if (compacted) drop_dead_slots();
    const int64_t expect = (compacted ? (int64_t)slot_id_.size() : rows_before) + (rc == APSS_OK ? n : 0);
    if (storedVectors() == expect && rc == APSS_OK) {
      slot_id_.insert(slot_id_.end(), ids.begin(), ids.end());
      slot_dead_.resize(slot_id_.size(), 0);
    } else if (storedVectors() != (int64_t)slot_id_.size()) {
      slots_known_ = false;
    }
  }
  if (rc != APSS_OK) throw std::runtime_error(g_ ? apss_group_last_error(g_) : apss_last_error(h_));
  std::vector<int64_t> q((size_t)n_res), c((size_t)n_res);
  std::vector<float> s((size_t)n_res);
  if (n_res && (g_ ? apss_group_fetch_results(g_, 0, n_res, q.data(), c.data(), s.data())
                   : apss_fetch_results(h_, 0, n_res, q.data(), c.data(), s.data())) != APSS_OK)
    throw std::runtime_error(g_ ? apss_group_last_error(g_) : apss_last_error(h_));
  SimilarityOutput out;
  for (const auto &kv : m.vectors) out.output[kv.first];  // every query gets an entry, possibly empty (:106-107)
  for (int64_t i = 0; i < n_res; ++i) out.output[name_of_[(size_t)q[i]]][name_of_[(size_t)c[i]]] = (double)s[i];
  out.outputMoment = now_ms();
  return out;
}

void GpuIndexingWorker::receive(const IndexData &m) {
  try {
    SimilarityOutput out = handle(m);
    if (!reply_to_) return;
    if (conf_.outputIODuration <= 0) {
      reply_to_(out);  // replyTo.get ! SimilarityOutput(...), :130
    } else {           // updateWriteBuffer, :113-120
      for (auto &q : out.output)
        for (auto &c : q.second) write_buffer_[q.first][c.first] = c.second;
    }
  } catch (const std::exception &e) {  // case e: Exception => e.printStackTrace(), :135-137: the batch's output is lost
    last_error_ = e.what();
    std::fprintf(stderr, "GpuIndexingWorker: %s\n", e.what());
  }
}

void GpuIndexingWorker::receive(const IOTicket &) {
  if (write_buffer_.empty()) return;
  SimilarityOutput out;
  out.output = write_buffer_;  // writeBuffer.clone()
  out.outputMoment = now_ms();
  write_buffer_.clear();
  if (reply_to_) reply_to_(out);
}

void GpuIndexingWorker::receive(const Test &t) {
  std::printf("receiving Test(%s) in IndexWorkerActor\n", t.content.c_str());
}

void GpuIndexingWorker::receiveTimeout() { stop_update_index_ = true; }

void Region::tell(const VectorIOMsg &m) {
  IndexData d;
  d.vectors = m.vectors;
  worker_->receive(d);
}

ClientConnection::ClientConnection(const std::vector<std::string> &remoteAddresses,
                                   std::function<std::shared_ptr<Region>(const std::string &)> resolve) {
  for (const std::string &hp : remoteAddresses) {  // ClientConnection.scala:12-21
    const size_t colon = hp.find(':');
    if (colon == std::string::npos) throw std::out_of_range("ArrayIndexOutOfBoundsException: 1");  // hostAndPort(1)
    routers_.push_back("akka.tcp://ClusterSystem@" + hp.substr(0, colon) + ":" + hp.substr(colon + 1) + "/user/regionRouter");
  }
  if (routers_.empty()) throw std::invalid_argument("bound must be positive");  // Random.nextInt(0)
  std::mt19937 rng{std::random_device{}()};
  remote_router_ = resolve(routers_[rng() % routers_.size()]);  // Random.nextInt(remoteAddresses.length), :23-24
}

void ClientConnection::insertNewVector(const std::vector<std::pair<std::string, SparkSparseVector>> &vectors) {
  VectorIOMsg m;
  m.vectors = vectors;
  if (remote_router_) remote_router_->tell(m);  // remoteRouter ! VectorIOMsg(vectors)
}

}  // namespace cpslab
