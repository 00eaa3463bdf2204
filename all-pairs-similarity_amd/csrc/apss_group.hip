// apss_group.hip -- the sharded index of one node (T term ranges x D row ranges) behind ONE object of the C ABI
// (include/apss.h, apss_group_*).
//
// What the reference does with actors -- WriteWorkerActor buckets a vector by dim % maxShardNum and flushes a DataPacket per
// shard (WriteWorkerActor.scala:164-183), EntryProxyActor fans it out to the IndexingWorkerActors by
// dim % maxIndexEntryActorNum (EntryProxyActor.scala:37-49), every worker handles IndexData alone
// (IndexingWorkerActor.scala:122-137) -- with the workers resident on the GPUs of one node: member g = one shard handle
// (apss_hip.hip) on one device, one host thread per member for the member-local phase, and the exchange of the members'
// answers (all-gather of candidate lists, all-reduce(SUM) of per-candidate partial scores) over RCCL on the members' streams.
// A grid (apss_group_create_grid, D > 1 row ranges) runs that exchange INSIDE each row range, once per phase: the row range's
// own span of the batch (insert-and-query), then one outside batch made of the other spans (query); the phases' results are
// gathered as (ext, ext, score) triples per row range.
// This file only uses the public handle ABI; it holds no index state of its own.
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include <rccl/rccl.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>

#include "../../include/apss.h"
#include "apss_lockstep.hpp"
#include "apss_topk.hpp"

namespace {

thread_local std::string g_group_create_error;

using Clock = std::chrono::steady_clock;
inline double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }
__host__ __device__ inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- RCCL, loaded on first use: libapss_hip.so itself does not depend on librccl (a single-GPU deployment, or a JVM without
// RCCL on its library path, loads and runs without it).  A process that already maps an image with soname librccl.so.1
// (PyTorch-ROCm bundles one) gets THAT image: there is never a second copy.  RTLD_LOCAL, always: promoting librccl and its
// dependencies (librocm_smi64 ...) to the global scope lets a later loader of the same libraries bind to their statics and
// destroy them twice at exit (seen with `import torch` after a group's first RCCL call: double free in rocm_smi's teardown).
struct Rccl {
  void *lib = nullptr;
  decltype(&ncclCommInitAll) CommInitAll = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  decltype(&ncclBroadcast) Broadcast = nullptr;
  decltype(&ncclAllReduce) AllReduce = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  std::string err;
};

Rccl *load_rccl() {
  static std::mutex mu;
  static Rccl r;
  std::lock_guard<std::mutex> lk(mu);
  if (r.lib) return &r;
  std::vector<std::string> names = {"librccl.so.1", "librccl.so"};
  void *lib = nullptr;
  for (const std::string &n : names)
    if ((lib = dlopen(n.c_str(), RTLD_NOW | RTLD_NOLOAD | RTLD_LOCAL))) break;
  if (!lib) {
    // beside the HIP runtime this process runs on (PyTorch's bundle, or /opt/rocm/lib), then the loader's own search path
    Dl_info info;
    if (dladdr(reinterpret_cast<void *>(&hipGetDeviceCount), &info) && info.dli_fname) {
      std::string dir(info.dli_fname);
      const size_t slash = dir.rfind('/');
      if (slash != std::string::npos) {
        dir.resize(slash + 1);
        names.insert(names.begin(), {dir + "librccl.so.1", dir + "librccl.so"});
      }
    }
    names.push_back("/opt/rocm/lib/librccl.so.1");
    for (const std::string &n : names)
      if ((lib = dlopen(n.c_str(), RTLD_NOW | RTLD_LOCAL))) break;
  }
  if (!lib) {
    r.err = std::string("librccl.so.1 not found: ") + (dlerror() ? dlerror() : "");
    return &r;
  }
#define APSS_RCCL_SYM(field, name)                                                      \
  r.field = reinterpret_cast<decltype(r.field)>(dlsym(lib, name));                     \
  if (!r.field) {                                                                       \
    r.err = std::string("librccl: missing symbol ") + name;                             \
    return &r;                                                                          \
  }
  APSS_RCCL_SYM(CommInitAll, "ncclCommInitAll")
  APSS_RCCL_SYM(CommDestroy, "ncclCommDestroy")
  APSS_RCCL_SYM(GetErrorString, "ncclGetErrorString")
  APSS_RCCL_SYM(Broadcast, "ncclBroadcast")
  APSS_RCCL_SYM(AllReduce, "ncclAllReduce")
  APSS_RCCL_SYM(GroupStart, "ncclGroupStart")
  APSS_RCCL_SYM(GroupEnd, "ncclGroupEnd")
#undef APSS_RCCL_SYM
  r.lib = lib;
  return &r;
}

using apss::Barrier;
using apss::DevBuf;
using apss::Lockstep;
using apss::When;
static_assert(APSS_OK == apss::kLockstepOk, "apss_lockstep.hpp takes 0 for success");

// ---- kernels of the exchange (everything else is the shard handles' work)
// candidate (query row of the batch, candidate slot) -> one sortable 8-B key
__global__ void k_pack_keys(const int32_t *q_row, const int32_t *c_slot, int64_t n, unsigned long long *keys) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    keys[i] = ((unsigned long long)(uint32_t)q_row[i] << 32) | (unsigned long long)(uint32_t)c_slot[i];
}

__global__ void k_unpack_keys(const unsigned long long *keys, int64_t n, int32_t *q_row, int32_t *c_slot) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    q_row[i] = (int32_t)(keys[i] >> 32);
    c_slot[i] = (int32_t)(keys[i] & 0xffffffffULL);
  }
}

// the copies exchange's reduction: sum += part (one launch per member after the first)
__global__ void k_accumulate(float *sum, const float *part, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) sum[i] += part[i];
}

// the `>= theta` prune (IndexingWorkerActor.scala:93) over the reduced scores; survivors compacted per wavefront: ballot,
// one atomic per wave, prefix popcount for the lane's place
__global__ void k_threshold_compact(const float *score, const int32_t *q_row, const int32_t *c_slot, int64_t n, float theta,
                                    int32_t *out_q, int32_t *out_c, float *out_s, unsigned long long *out_count) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t n_pad = ceil_div(n, 64) * 64;  // whole waves take every trip of the loop together
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pad; i += stride) {
    const bool keep = i < n && score[i] >= theta;
    const unsigned long long mask = __ballot(keep);
    if (mask == 0) continue;
    const int lane = threadIdx.x & 63;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(out_count, (unsigned long long)__popcll(mask));
    base = __shfl(base, 0);
    if (keep) {
      const unsigned long long at = base + (unsigned long long)__popcll(mask & ((1ULL << lane) - 1ULL));
      out_q[at] = q_row[i];
      out_c[at] = c_slot[i];
      out_s[at] = score[i];
    }
  }
}

__global__ void k_gather_ext(const int32_t *q_row, const int32_t *c_slot, const int64_t *q_ext, const int64_t *c_ext, int64_t n,
                             int64_t *out_q, int64_t *out_c) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    out_q[i] = q_ext[q_row[i]];
    out_c[i] = c_ext[c_slot[i]];
  }
}

// document frequencies of terms [lo, hi) (df[t - lo]) over a device-resident batch (the layout decision of a group fed through the
// device entry point) or over one member's stored slice (a re-layout: each member's range, the histograms side by side)
__global__ void k_df_hist(const int32_t *idx, int64_t nnz, int32_t lo, int32_t hi, unsigned int *df) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t t = idx[i];
    if (t >= lo && t < hi) atomicAdd(&df[t - lo], 1u);  // (a malformed index is the shard handle's to refuse)
  }
}

// ---- re-layout: whole rows out of the members' slices.  Slot r is row r on every member, the ranges are contiguous and in
// member order, so whole row r = member 0's slice of r, then member 1's, ... (terms stay strictly increasing).
// whole-row lengths: len[r] += the row's entries in one member's slice (one launch per member)
__global__ void k_row_len_add(const int64_t *rowptr, int64_t rows, int64_t *len) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x)
    len[r] += rowptr[r + 1] - rowptr[r];
}

// one member's slice into the whole rows: cur[r] = where the row's next entries go (starts as the whole row's offset; the
// launches run in member order on one stream and each advances it by the member's part).  A wave takes 64 consecutive rows;
// their entries are one contiguous run of the slice, which the wave copies 64 entries at a time -- coalesced 4-B loads and
// stores, every lane busy however short the rows -- and each lane finds its entry's row by a binary search over the lanes'
// row starts (shuffles).
__global__ __launch_bounds__(256) void k_merge_slice(const int64_t *rowptr, const int32_t *idx, const float *val, int64_t rows,
                                                     int64_t *cur, int32_t *out_idx, float *out_val) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r0 = wave * 64; r0 < rows; r0 += n_waves * 64) {
    const int64_t r = r0 + lane;
    const bool live = r < rows;
    const int64_t s = live ? rowptr[r] : rowptr[rows];  // (lanes past the end: empty rows at the end of the slice)
    const int64_t e = live ? rowptr[r + 1] : s;
    const int64_t d = live ? cur[r] - s : 0;  // entry k of this row goes to d + k
    const int64_t run_b = __shfl(s, 0), run_e = __shfl(e, 63);
    for (int64_t k0 = run_b; k0 < run_e; k0 += 64) {
      const int64_t k = k0 + lane;
      int j = 0;  // the last lane whose row starts at or before k (empty rows share their start with the next row)
      for (int step = 32; step; step >>= 1) {
        const int64_t sj = __shfl(s, j + step);
        if (sj <= k) j += step;
      }
      const int64_t dj = __shfl(d, j);
      if (k < run_e) {
        out_idx[dj + k] = idx[k];
        out_val[dj + k] = val[k];
      }
    }
    if (live) cur[r] += e - s;
  }
}

// ---- grids: the spans of a device-resident batch.  A phase's batch is a concatenation of contiguous row spans of the whole
// batch (one span: a row range's own rows; several: its outside batch), described by a small table passed by value.
constexpr int kMaxSpans = APSS_GROUP_MAX_MEMBERS;
struct SpanBounds {
  int32_t n;
  int64_t row[kMaxSpans + 1];
};
struct SpanTable {
  int32_t n;                       // spans, in output order (each with at least one row)
  int64_t src_row[kMaxSpans];      // first row of span s in the whole batch
  int64_t src_ent[kMaxSpans];      // ... its first entry
  int64_t out_row[kMaxSpans + 1];  // first row of span s in the output; [n] = rows of the output
  int64_t out_ent[kMaxSpans + 1];  // first entry of span s in the output; [n] = entries of the output
};

// the batch's row offsets at the span boundaries (b.row[k] <= n rows), for the one small read-back of a call
__global__ void k_span_offsets(const int64_t *rowptr, SpanBounds b, int64_t *out) {
  const int t = (int)threadIdx.x;
  if (t < b.n) out[t] = rowptr[b.row[t]];
}

// rows of the output: rebased row offsets and external ids, span after span
__global__ void k_concat_rows(const int64_t *rowptr, const int64_t *ext, SpanTable t, int64_t *out_rowptr, int64_t *out_ext) {
  const int64_t rows = t.out_row[t.n];
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= rows; r += (int64_t)gridDim.x * blockDim.x) {
    if (r == rows) {
      out_rowptr[r] = t.out_ent[t.n];
      continue;
    }
    int s = 0;
    while (s + 1 < t.n && t.out_row[s + 1] <= r) ++s;
    const int64_t src = t.src_row[s] + (r - t.out_row[s]);
    out_rowptr[r] = rowptr[src] - t.src_ent[s] + t.out_ent[s];
    out_ext[r] = ext[src];
  }
}

// entries of the output: a span's entries are one contiguous run of the whole batch
__global__ void k_concat_entries(const int32_t *idx, const float *val, SpanTable t, int32_t *out_idx, float *out_val) {
  const int64_t total = t.out_ent[t.n];
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    int s = 0;
    while (s + 1 < t.n && t.out_ent[s + 1] <= e) ++s;  // (a span of empty rows shares its offset with the next: skipped)
    const int64_t src = t.src_ent[s] + (e - t.out_ent[s]);
    out_idx[e] = idx[src];
    out_val[e] = val[src];
  }
}

// a phase's results as (query ext id, candidate ext id, score) triples, appended to the row range's list; a mirrored phase
// (the symmetry across row ranges) reports every pair in the other direction as well, n entries further on
__global__ void k_triples(const int32_t *q_row, const int32_t *c_slot, const float *score, const int64_t *q_ext, const int64_t *c_ext,
                          int64_t n, int mirrored, int64_t *out_q, int64_t *out_c, float *out_s) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t q = q_ext[q_row[i]], c = c_ext[c_slot[i]];
    const float sc = score[i];
    out_q[i] = q;
    out_c[i] = c;
    out_s[i] = sc;
    if (mirrored) {
      out_q[n + i] = c;
      out_c[n + i] = q;
      out_s[n + i] = sc;
    }
  }
}

inline unsigned grid_for(int64_t n, int threads = 256, int64_t cap = 4096) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cap, ceil_div(n, threads)));
}

}  // namespace

struct apss_group {
  // (a member's, a range's and the group's arrays stand in structs of their own: apss_group_destroy assigns each an empty one
  // with the right device current)
  struct MemberBufs {
    // exchange buffers, on this member's device
    DevBuf<unsigned long long> keys, sorted, uniq, count;
    DevBuf<char> tmp;
    DevBuf<int32_t> uq, uc;
    DevBuf<float> partial, sum, stage;
    // grids, device-pointer entry: the phases' batches cut out of the whole batch on this device ([0] own span, [1] outside)
    DevBuf<int64_t> sp_rowptr[2], sp_ext[2], sp_off;
    DevBuf<int32_t> sp_idx[2];
    DevBuf<float> sp_val[2];
  };
  struct Member : MemberBufs {
    int dev = 0;
    apss_handle *h = nullptr;
    apss::DevStream stream;
    ncclComm_t comm = nullptr;
    int64_t n_cand = 0, n_union = 0;
    double member_ms = 0, partial_ms = 0;
    int32_t rc = APSS_OK;
    std::string err;
    // the call's sums over its phases (a grid's own join and outside batch; one phase otherwise)
    int64_t visits = 0, dev_visits = 0, touched = 0, cand_sum = 0, cand_max = 0;
    double probe_ms = 0, head_ms = 0;
  };
  // one row range: its T members hold the same rows; its buffers live on its first member's device
  struct RangeBufs {
    // results of the phase in flight (exchange modes): query row of the phase's batch, candidate slot, score
    DevBuf<int32_t> res_q, res_c;
    DevBuf<float> res_s;
    // grids: the call's results as triples, phase after phase
    DevBuf<int64_t> tri_q, tri_c;
    DevBuf<float> tri_s;
  };
  struct Range : RangeBufs {
    int64_t rows = 0;
    int64_t n_phase = 0;  // pairs of the phase in flight
    int64_t n_tri = 0;    // triples of the call so far
    int64_t union_pairs = 0, gather_bytes = 0, mirrored = 0, outside_rows = 0;
    double own_ms = 0, outside_ms = 0, exchange_ms = 0;
  };
  apss_config cfg{};
  uint32_t flags = 0;
  int T = 0;  // term ranges
  int D = 1;  // row ranges; member (j, i) = row range j, term range i = m[j * T + i]
  std::vector<Member> m;
  std::vector<Range> rr;
  bool symmetric_ranges = false;  // the last query-type call used half spans and mirrored
  std::string err;
  bool created = false;         // the members' handles exist (the layout is decided)
  bool cuts_named = false;      // apss_group_set_term_cuts
  std::vector<int32_t> cuts;    // T + 1
  std::vector<int32_t> head;    // shared dense-head terms
  int exchange = APSS_EXCHANGE_NONE;
  bool distinct_devices = true;
  int64_t n_rows = 0;
  // layout history (apss_group_layout)
  int64_t layout_rows = 0;
  int64_t evaluations = 0, relayouts = 0, relayout_bytes = 0;
  double last_relayout_ms = 0, total_relayout_ms = 0;
  int relayout_fail = -1;  // APSS_DEBUG=relayout_fail=<member>: that member's insert of a re-layout fails (test hook)
  // results of the last query-type call: D = 1, exchange modes: rr[0].res_* on member 0's device; grids: the ranges' triples
  struct ExtBufs {
    DevBuf<int64_t> q, c;
  } ext;
  int64_t n_res = -1;
  bool results_in_handle = false;  // one member, no exchange: the handle's own result list
  // per-query top-k (apss_topk.hpp; D = 1 only).  One member without an exchange: its handle holds the setting and cuts its own
  // list.  Exchange modes: the pass runs on member 0's device behind k_threshold_compact, with these buffers
  int32_t top_k = 0;
  apss::TopkWork topk;
  apss_topk_info tk{};
  apss_group_stats st{};
};

namespace {

int32_t gfail(apss_group *g, int32_t rc, const std::string &msg) {
  g->err = msg;
  return rc;
}
// (a member's: its thread publishes the code, run_members reports the message)
int32_t mfail(apss_group::Member &M, int32_t rc, const std::string &msg) {
  M.err = msg;
  return rc;
}
inline int32_t hip_rc(hipError_t e) { return e == hipErrorOutOfMemory ? APSS_E_NOMEM : APSS_E_DEVICE; }

#define GHIP(g, M, expr)                                                                            \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess) {                                                                          \
      return mfail((M), hip_rc(e_), std::string(#expr) + ": " + hipGetErrorString(e_));              \
    }                                                                                                \
  } while (0)

// room for n elements in each of the arrays, on M's device: the old block freed first, the contents dropped (apss_owned.hpp,
// kGrowGroup; a list that is appended to grows with kGrowGroupKeep where it does)
template <class... A>
int32_t ensure(apss_group::Member &M, size_t n, A &...b) {
  GHIP(nullptr, M, apss::grow_all(apss::kGrowGroup, n, 0, M.stream, nullptr, b...));
  return APSS_OK;
}

// a few words of M's device into a host variable, on M's stream, which is waited for
template <class T>
int32_t read_back(apss_group::Member &M, T *host, const T *dev, size_t n = 1) {
  GHIP(nullptr, M, hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, M.stream));
  GHIP(nullptr, M, hipStreamSynchronize(M.stream));
  return APSS_OK;
}

int32_t set_member_device(apss_group::Member &M) {
  return hipSetDevice(M.dev) == hipSuccess ? APSS_OK : mfail(M, APSS_E_DEVICE, "hipSetDevice failed");
}

// fn(m, cx) for the n members of a call (member 0 on the caller's thread), the caller's device current again behind them; a
// failed call reports its lowest-numbered failed member, or `fallback`
template <class Ctx>
int32_t run_members(apss_group *g, int n, void (*fn)(int, Ctx *), Ctx *cx, const char *fallback) {
  apss::run_members(n, fn, cx);
  (void)hipSetDevice(g->m[0].dev);
  if (!cx->failed.load()) return APSS_OK;
  const apss::MemberFailure f = apss::first_failure(
      n, [&](int m) { return g->m[(size_t)m].rc; }, [&](int m) -> const std::string & { return g->m[(size_t)m].err; }, APSS_E_STATE, fallback);
  return gfail(g, f.rc, f.msg);
}

// one batch as the caller handed it in
struct Batch {
  int64_t n = 0, nnz = 0;
  // host form
  const int64_t *rowptr = nullptr;
  const int32_t *indices = nullptr;
  const double *values = nullptr;
  const int64_t *ext = nullptr;
  // device form (per member)
  const int64_t *const *d_rowptr = nullptr;
  const int32_t *const *d_indices = nullptr;
  const float *const *d_values = nullptr;
  const int64_t *const *d_ext = nullptr;
  bool on_device = false;
};

// contiguous term ranges with (nearly) equal sum of df^2 (= the posting visits of a self-join), each non-empty
std::vector<int32_t> balanced_cuts(const std::vector<uint32_t> &df, int T) {
  const int32_t dim = (int32_t)df.size();
  std::vector<double> cum((size_t)dim + 1, 0.0);
  for (int32_t t = 0; t < dim; ++t) cum[(size_t)t + 1] = cum[(size_t)t] + (double)df[(size_t)t] * (double)df[(size_t)t];
  std::vector<int32_t> cuts((size_t)T + 1, 0);
  for (int g = 1; g < T; ++g) {
    const double want = cum.back() * (double)g / (double)T;
    cuts[(size_t)g] = (int32_t)(std::lower_bound(cum.begin(), cum.end(), want) - cum.begin());
  }
  cuts[(size_t)T] = dim;
  for (int g = 1; g <= T; ++g) cuts[(size_t)g] = std::max(cuts[(size_t)g], cuts[(size_t)g - 1] + 1);
  cuts[(size_t)T] = dim;
  for (int g = T - 1; g >= 1; --g) cuts[(size_t)g] = std::min(cuts[(size_t)g], cuts[(size_t)g + 1] - 1);
  return cuts;
}

std::vector<int32_t> equal_cuts(int32_t dim, int T) {
  std::vector<int32_t> cuts((size_t)T + 1, 0);
  for (int g = 0; g <= T; ++g) cuts[(size_t)g] = (int32_t)((int64_t)dim * g / T);
  return cuts;
}

// document frequencies of the terms [lo, hi) over idx[0, nnz) on M's device, into the host array out[hi - lo]: scratch that lives as
// long as this call, one launch on M's stream, which is waited for
hipError_t df_hist(apss_group::Member &M, const int32_t *idx, int64_t nnz, int32_t lo, int32_t hi, unsigned int *out) {
  const size_t bytes = (size_t)(hi - lo) * sizeof(unsigned int);
  DevBuf<unsigned int> d_df;
  hipError_t e = d_df.grow(apss::kGrowStage, (size_t)(hi - lo), 0, nullptr, nullptr);
  if (e == hipSuccess) e = hipMemsetAsync(d_df.p, 0, bytes, M.stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_df_hist, dim3(grid_for(nnz)), dim3(256), 0, M.stream, idx, nnz, lo, hi, d_df.p);
  if ((e = hipGetLastError()) == hipSuccess) e = hipMemcpyAsync(out, d_df.p, bytes, hipMemcpyDeviceToHost, M.stream);
  return e == hipSuccess ? hipStreamSynchronize(M.stream) : e;
}

// document frequencies of a batch as the caller handed it in, added to df (on member 0's device for a device batch)
int32_t add_batch_df(apss_group *g, const Batch &b, std::vector<uint32_t> &df) {
  const int32_t dim = g->cfg.dim;
  apss_group::Member &M0 = g->m[0];
  if (!b.on_device) {
    for (int64_t i = 0; i < b.nnz; ++i) {
      const int32_t t = b.indices[i];
      if (t >= 0 && t < dim) ++df[(size_t)t];
    }
    return APSS_OK;
  }
  if (b.nnz == 0) return APSS_OK;
  if (hipSetDevice(M0.dev) != hipSuccess) return gfail(g, APSS_E_DEVICE, "hipSetDevice failed");
  std::vector<uint32_t> part((size_t)dim, 0u);
  const hipError_t e = df_hist(M0, b.d_indices[0], b.nnz, 0, dim, part.data());
  if (e != hipSuccess) return gfail(g, APSS_E_DEVICE, std::string("document frequencies: ") + hipGetErrorString(e));
  for (size_t t = 0; t < part.size(); ++t) df[t] += part[t];
  return APSS_OK;
}

// the first `count` rows of a batch into a handle (the head policy's sample)
int32_t feed_batch(apss_group *g, apss_handle *ph, const Batch &b, int64_t count) {
  if (count <= 0) return APSS_OK;
  if (!b.on_device) return apss_insert(ph, count, b.rowptr, b.indices, b.values, b.ext);
  int64_t e_end = 0;
  (void)hipSetDevice(g->m[0].dev);
  if (hipMemcpy(&e_end, b.d_rowptr[0] + count, sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess) return APSS_E_DEVICE;
  return apss_insert_dev(ph, count, e_end, b.d_rowptr[0], b.d_indices[0], b.d_values[0], b.d_ext[0]);
}

bool needs_df(const apss_group *g, bool cuts_fixed) { return g->T > 1 && (!cuts_fixed || g->cfg.head_terms == 0); }

bool head_possible(const apss_group *g) {
  return g->T > 1 && g->cfg.head_terms >= 0 && g->cfg.theta > 0.0 &&
         !(g->cfg.flags & (APSS_FLAG_EXACT_ACCUM | APSS_FLAG_FORCE_GENERAL | APSS_FLAG_FORCE_SCAN | APSS_FLAG_ADMISSION));
}

struct Layout {
  std::vector<int32_t> cuts;  // T + 1
  std::vector<int32_t> head;  // shared dense-head terms
};

// Decide a layout for n_rows rows with document frequencies df (needs_df; the head's terms are zeroed on return): the shared
// dense-head block (member 0's device runs the library's own policy on a sample of the rows, put into a plain handle by
// `feed`, which is asked which terms it took) and the term cuts -- `fixed` when named, else balanced by sum df^2.
int32_t decide_layout(apss_group *g, std::vector<uint32_t> &df, int64_t n_rows, const std::vector<int32_t> *fixed,
                      const std::function<int32_t(apss_handle *)> &feed, Layout &out) {
  const int T = g->T;
  const int32_t dim = g->cfg.dim;
  apss_group::Member &M0 = g->m[0];
  out.head.clear();
  if (head_possible(g) && n_rows > 0) {
    apss_config pc = g->cfg;
    pc.struct_size = (int32_t)sizeof(apss_config);
    pc.device_id = M0.dev;
    pc.term_lo = pc.term_hi = 0;
    pc.capacity_rows = pc.capacity_nnz = 0;
    apss_handle *ph = nullptr;
    int32_t rc = apss_create(&pc, &ph);
    if (rc != APSS_OK) return gfail(g, rc, std::string("head policy handle: ") + apss_last_error(nullptr));
    rc = feed(ph);
    int32_t nt = 0;
    if (rc == APSS_OK) rc = apss_get_head_terms(ph, 0, nullptr, &nt);
    if (rc == APSS_OK && nt > 0) {
      out.head.resize((size_t)nt);
      rc = apss_get_head_terms(ph, nt, out.head.data(), &nt);
    }
    const std::string perr = rc == APSS_OK ? "" : apss_last_error(ph);
    apss_destroy(ph);
    if (rc != APSS_OK) return gfail(g, rc, "head policy handle: " + perr);
    if (g->cfg.head_terms == 0 && out.head.size() > 256) {
      // A deep head leaves few tail terms per row, and T term ranges cut them T ways: a row with a single term in a range
      // pairs up at within-range cosine 1 with every row sharing it and the candidate rule stops being selective.  Keep the
      // head only as deep as leaves about 8 tail terms per row and member, never shallower than the 256 terms that hold the
      // long posting lists (measured on C3 with Zipf(1) terms).
      double total = 0;
      for (uint32_t f : df) total += (double)f;
      size_t k = out.head.size();
      for (;;) {
        double in_head = 0;
        for (size_t i = 0; i < k; ++i) in_head += (double)df[(size_t)out.head[i]];
        if (k <= 256 || (total - in_head) / (double)std::max<int64_t>(1, n_rows) / (double)T >= 8.0) break;
        k /= 2;
      }
      out.head.resize(std::max<size_t>(k, 256));
    }
  }
  if (fixed) {
    out.cuts = *fixed;
  } else if (T == 1) {
    out.cuts = {0, dim};
  } else if (n_rows < 1024) {
    out.cuts = equal_cuts(dim, T);  // (this few rows say nothing about the term distribution)
  } else {
    for (int32_t t : out.head) df[(size_t)t] = 0;  // the block's terms are in no member's index: balance the tail's visits
    out.cuts = balanced_cuts(df, T);
  }
  if (dim < T) return gfail(g, APSS_E_INVALID, "more members than terms");
  return APSS_OK;
}

// the group's answer is its one member's own list (no exchange): that handle applies the per-query top-k itself
inline bool topk_in_handle(const apss_group *g) { return g->T == 1 && g->D == 1 && !(g->flags & APSS_GROUP_FORCE_EXCHANGE); }

// member m's shard handle for a layout (term range m % T), on the member's stream (*out stays NULL on failure; the message
// is in err)
int32_t create_member_handle(apss_group *g, int m, const Layout &L, apss_handle **out, std::string &err) {
  const int T = g->T;
  const int i = m % T;
  apss_group::Member &M = g->m[(size_t)m];
  *out = nullptr;
  apss_config c = g->cfg;
  c.struct_size = (int32_t)sizeof(apss_config);
  c.device_id = M.dev;
  c.term_lo = T == 1 ? 0 : L.cuts[(size_t)i];
  c.term_hi = T == 1 ? 0 : L.cuts[(size_t)i + 1];
  apss_handle *h = nullptr;
  int32_t rc = apss_create(&c, &h);
  if (rc != APSS_OK) {
    err = std::string("member handle: ") + apss_last_error(nullptr);
    return rc;
  }
  if ((rc = apss_set_stream(h, (void *)M.stream, 0)) != APSS_OK) {
    err = apss_last_error(h);
  } else if (!L.head.empty() && (rc = apss_set_head_terms(h, (int32_t)L.head.size(), L.head.data(), i, T)) != APSS_OK) {
    err = std::string("member head block: ") + apss_last_error(h);
  } else if (topk_in_handle(g) && (rc = apss_set_top_k(h, g->top_k)) != APSS_OK) {
    err = std::string("member top-k: ") + apss_last_error(h);
  }
  if (rc != APSS_OK) {
    apss_destroy(h);
    return rc;
  }
  *out = h;
  return APSS_OK;
}

// Decide the layout from the first batch (the WHOLE batch, all spans of a grid: one set of cuts and one head for every row
// range), then create the members' shard handles and -- when the members of every row range have a GPU each -- the RCCL
// communicators.
int32_t create_members(apss_group *g, const Batch &b) {
  const int T = g->T;
  std::vector<uint32_t> df;
  if (needs_df(g, g->cuts_named)) {
    df.assign((size_t)g->cfg.dim, 0u);
    const int32_t rc = add_batch_df(g, b, df);
    if (rc != APSS_OK) return rc;
  }
  Layout L;
  const std::vector<int32_t> named = g->cuts;
  int32_t rc = decide_layout(g, df, b.n, g->cuts_named ? &named : nullptr,
                             [&](apss_handle *ph) { return feed_batch(g, ph, b, std::min<int64_t>(b.n, 131072)); }, L);
  if (rc != APSS_OK) return rc;
  g->cuts = L.cuts;
  g->head = L.head;
  for (int m = 0; m < T * g->D; ++m) {
    std::string err;
    if ((rc = create_member_handle(g, m, L, &g->m[(size_t)m].h, err)) != APSS_OK) return gfail(g, rc, err);
  }
  const bool exchange_needed = T > 1 || (g->flags & APSS_GROUP_FORCE_EXCHANGE);
  g->exchange = !exchange_needed ? APSS_EXCHANGE_NONE : APSS_EXCHANGE_COPIES;
  if (exchange_needed && g->distinct_devices && !(g->flags & APSS_GROUP_NO_RCCL)) {
    Rccl *r = load_rccl();
    if (!r->lib) return gfail(g, APSS_E_UNSUPPORTED, "RCCL exchange: " + r->err + " (APSS_GROUP_NO_RCCL combines the members by copies)");
    for (int j = 0; j < g->D; ++j) {  // one communicator per row range
      std::vector<ncclComm_t> comms((size_t)T, nullptr);
      std::vector<int> devs;
      for (int i = 0; i < T; ++i) devs.push_back(g->m[(size_t)(j * T + i)].dev);
      const ncclResult_t nr = r->CommInitAll(comms.data(), T, devs.data());
      if (nr != ncclSuccess) return gfail(g, APSS_E_DEVICE, std::string("ncclCommInitAll: ") + r->GetErrorString(nr));
      for (int i = 0; i < T; ++i) g->m[(size_t)(j * T + i)].comm = comms[(size_t)i];
    }
    g->exchange = APSS_EXCHANGE_RCCL;
  }
  g->layout_rows = b.n;
  g->created = true;
  return APSS_OK;
}

// ---- one member's share of a call; every member thread runs this, the barriers keep the phases in step.  A failure is
// published BEFORE the next barrier, and every thread acts on the flag as the barrier returned it: they leave (or skip a
// collective) together -- Lockstep::step (apss_lockstep.hpp) is that rule, and the only place a thread of this file waits at a
// barrier or raises the flag.  A grid has one barrier per row range (its T members are a term-sharded group of their own and never
// wait for another row range) and ONE failure flag for all T x D threads.

// a phase's batch as ONE member reads it (host form: values; device form, on the member's device: d_values)
struct MemberBatch {
  int64_t n = 0, nnz = 0;
  const int64_t *rowptr = nullptr;
  const int32_t *indices = nullptr;
  const double *values = nullptr;
  const float *d_values = nullptr;
  const int64_t *ext = nullptr;
  bool on_device = false;
};

// a CSR cut out of a host batch
struct HostCsr {
  std::vector<int64_t> rowptr, ext;
  std::vector<int32_t> idx;
  std::vector<double> val;
};

// what one row range does in a call
struct RangePlan {
  int span = 0;              // the span of the batch this row range stores
  std::vector<int> outside;  // the spans of its outside batch, in span order
  bool mirrored = false;     // the outside phase's pairs are reported in both directions
  int64_t out_rows = 0;
  HostCsr own, out;          // host-pointer entry points: sliced by the caller's thread before the members start
};

struct CallCtx {
  apss_group *g;
  int mode;  // 0 insert, 1 query (frozen index), 2 insert-and-query
  Batch b;
  std::deque<Barrier> bar;       // per row range
  std::vector<int64_t> span_lo;  // grids: span k = rows [span_lo[k], span_lo[k + 1]) of the batch
  std::vector<RangePlan> plan;   // grids: per row range
  std::atomic<int> failed{0};
};

MemberBatch whole_batch(const Batch &b, int m) {
  MemberBatch mb;
  mb.n = b.n;
  mb.nnz = b.nnz;
  mb.on_device = b.on_device;
  if (!b.on_device) {
    mb.rowptr = b.rowptr;
    mb.indices = b.indices;
    mb.values = b.values;
    mb.ext = b.ext;
  } else if (b.n > 0) {
    mb.rowptr = b.d_rowptr[m];
    mb.indices = b.d_indices[m];
    mb.d_values = b.d_values[m];
    mb.ext = b.d_ext[m];
  }
  return mb;
}

MemberBatch host_csr_batch(const HostCsr &c) {
  MemberBatch mb;
  mb.n = (int64_t)c.ext.size();
  mb.nnz = (int64_t)c.idx.size();
  mb.rowptr = c.rowptr.data();
  mb.indices = c.idx.data();
  mb.values = c.val.data();
  mb.ext = c.ext.data();
  return mb;
}

// rows [lo, hi) of a host batch, appended to a CSR
void append_span(HostCsr &c, const Batch &b, int64_t lo, int64_t hi) {
  if (c.rowptr.empty()) c.rowptr.push_back(0);
  const int64_t shift = (int64_t)c.idx.size() - b.rowptr[lo];
  for (int64_t r = lo; r < hi; ++r) c.rowptr.push_back(b.rowptr[r + 1] + shift);
  c.ext.insert(c.ext.end(), b.ext + lo, b.ext + hi);
  if (b.rowptr[hi] > b.rowptr[lo]) {
    c.idx.insert(c.idx.end(), b.indices + b.rowptr[lo], b.indices + b.rowptr[hi]);
    c.val.insert(c.val.end(), b.values + b.rowptr[lo], b.values + b.rowptr[hi]);
  }
}

// grids, device-pointer entry: this member's copies of its row range's span (slot 0) and outside batch (slot 1), cut out of
// the whole batch resident on its device.  Only the batch's row offsets at the span boundaries come back to the host.
int32_t member_slice(apss_group::Member &M, const CallCtx &cx, const MemberBatch &whole, const RangePlan &P, MemberBatch out[2]) {
  const int D = cx.g->D;
  SpanBounds sb{};
  sb.n = D + 1;
  for (int k = 0; k <= D; ++k) sb.row[k] = cx.span_lo[(size_t)k];
  int32_t rc;
  if ((rc = ensure(M, (size_t)kMaxSpans + 1, M.sp_off)) != APSS_OK) return rc;
  hipLaunchKernelGGL(k_span_offsets, dim3(1), dim3(128), 0, M.stream, whole.rowptr, sb, M.sp_off.p);
  GHIP(nullptr, M, hipGetLastError());
  int64_t ent[kMaxSpans + 1];
  if ((rc = read_back(M, ent, M.sp_off.p, (size_t)(D + 1))) != APSS_OK) return rc;
  bool sane = ent[0] == 0 && ent[D] == whole.nnz;
  for (int k = 0; k < D; ++k) sane = sane && ent[k] <= ent[k + 1];
  // (the gathers below read entries [ent[k], ent[k + 1]) of arrays that are nnz long)
  if (!sane) return mfail(M, APSS_E_INVALID, "d_rowptr is not the row offsets of a batch of nnz entries");
  for (int slot = 0; slot < 2; ++slot) {
    SpanTable t{};
    std::vector<int> one(1, P.span);
    for (int k : slot == 0 ? one : P.outside) {
      const int64_t lo = cx.span_lo[(size_t)k], hi = cx.span_lo[(size_t)k + 1];
      if (hi == lo) continue;
      t.src_row[t.n] = lo;
      t.src_ent[t.n] = ent[k];
      t.out_row[t.n + 1] = t.out_row[t.n] + (hi - lo);
      t.out_ent[t.n + 1] = t.out_ent[t.n] + (ent[k + 1] - ent[k]);
      ++t.n;
    }
    MemberBatch &o = out[slot];
    o = MemberBatch{};
    o.on_device = true;
    if (t.n == 0) continue;
    o.n = t.out_row[t.n];
    o.nnz = t.out_ent[t.n];
    if ((rc = ensure(M, (size_t)o.n + 1, M.sp_rowptr[slot])) != APSS_OK) return rc;
    if ((rc = ensure(M, (size_t)o.n, M.sp_ext[slot])) != APSS_OK) return rc;
    if ((rc = ensure(M, (size_t)std::max<int64_t>(1, o.nnz), M.sp_idx[slot], M.sp_val[slot])) != APSS_OK) return rc;
    hipLaunchKernelGGL(k_concat_rows, dim3(grid_for(o.n + 1)), dim3(256), 0, M.stream, whole.rowptr, whole.ext, t, M.sp_rowptr[slot].p,
                       M.sp_ext[slot].p);
    GHIP(nullptr, M, hipGetLastError());
    if (o.nnz > 0) {
      hipLaunchKernelGGL(k_concat_entries, dim3(grid_for(o.nnz)), dim3(256), 0, M.stream, whole.indices, whole.d_values, t,
                         M.sp_idx[slot].p, M.sp_val[slot].p);
      GHIP(nullptr, M, hipGetLastError());
    }
    o.rowptr = M.sp_rowptr[slot].p;
    o.indices = M.sp_idx[slot].p;
    o.d_values = M.sp_val[slot].p;
    o.ext = M.sp_ext[slot].p;
  }
  return APSS_OK;
}

// step 1: the handle call of a phase (mode as CallCtx::mode), and what it adds to the member's sums of the call.  A
// mirrored phase found each pair once and reports it twice: the reference's two-directional probe visits twice as much.
int32_t member_phase1(apss_group::Member &M, int mode, const MemberBatch &b, bool mirrored) {
  const auto t0 = Clock::now();
  int64_t n_res = 0;
  int32_t rc;
  if (!b.on_device) {
    if (mode == 0) rc = apss_insert(M.h, b.n, b.rowptr, b.indices, b.values, b.ext);
    else if (mode == 1) rc = apss_query(M.h, b.n, b.rowptr, b.indices, b.values, b.ext, &n_res);
    else rc = apss_insert_and_query(M.h, b.n, b.rowptr, b.indices, b.values, b.ext, &n_res);
  } else if (mode == 1) {
    rc = apss_query_dev(M.h, b.n, b.nnz, b.rowptr, b.indices, b.d_values, b.ext, &n_res);
  } else {
    rc = apss_insert_and_query_dev(M.h, b.n, b.nnz, b.rowptr, b.indices, b.d_values, b.ext, &n_res);
  }
  if (rc != APSS_OK) M.err = apss_last_error(M.h);
  M.n_cand = n_res;
  if (rc == APSS_OK && mode != 0) {
    apss_stats ms{};
    ms.struct_size = (int32_t)sizeof(apss_stats);
    (void)apss_stats_get(M.h, &ms);
    M.visits += (mirrored ? 2 : 1) * ms.posting_visits;
    M.dev_visits += ms.device_posting_visits;
    M.touched += ms.candidate_pairs;
    M.cand_sum += n_res;
    M.cand_max = std::max(M.cand_max, n_res);
    M.probe_ms += ms.probe_ms;
    M.head_ms += ms.head_ms;
  }
  M.member_ms += ms_since(t0);
  return rc;
}

int32_t member_pack(apss_group::Member &M, int64_t total, int64_t my_off) {
  int32_t rc;
  if ((rc = ensure(M, (size_t)total, M.keys, M.sorted, M.uniq)) != APSS_OK) return rc;
  if ((rc = ensure(M, 4, M.count)) != APSS_OK) return rc;
  if (M.n_cand > 0) {
    const int32_t *dq = nullptr, *dc = nullptr;
    const float *ds = nullptr;
    int64_t n = 0;
    if ((rc = apss_results_dev(M.h, &dq, &dc, &ds, &n)) != APSS_OK) return mfail(M, rc, apss_last_error(M.h));
    hipLaunchKernelGGL(k_pack_keys, dim3(grid_for(M.n_cand)), dim3(256), 0, M.stream, dq, dc, M.n_cand, M.keys.p + my_off);
    GHIP(nullptr, M, hipGetLastError());
  }
  GHIP(nullptr, M, hipStreamSynchronize(M.stream));  // (the copies exchange lets the peers read this list)
  return APSS_OK;
}

int32_t member_union(apss_group::Member &M, int64_t total, int key_bits) {
  size_t a = 0, bsz = 0;
  GHIP(nullptr, M, rocprim::radix_sort_keys(nullptr, a, M.keys.p, M.sorted.p, (size_t)total, 0, (unsigned)key_bits, M.stream));
  GHIP(nullptr, M, rocprim::unique(nullptr, bsz, M.sorted.p, M.uniq.p, M.count.p, (size_t)total, rocprim::equal_to<unsigned long long>(), M.stream));
  int32_t rc;
  if ((rc = ensure(M, std::max(a, bsz) + 256, M.tmp)) != APSS_OK) return rc;
  GHIP(nullptr, M, rocprim::radix_sort_keys((void *)M.tmp.p, a, M.keys.p, M.sorted.p, (size_t)total, 0, (unsigned)key_bits, M.stream));
  GHIP(nullptr, M, rocprim::unique((void *)M.tmp.p, bsz, M.sorted.p, M.uniq.p, M.count.p, (size_t)total, rocprim::equal_to<unsigned long long>(), M.stream));
  unsigned long long nu = 0;
  if ((rc = read_back(M, &nu, M.count.p)) != APSS_OK) return rc;
  M.n_union = (int64_t)nu;
  if ((rc = ensure(M, (size_t)std::max<int64_t>(1, M.n_union), M.uq, M.uc, M.partial, M.sum)) != APSS_OK) return rc;
  if (M.n_union > 0) {
    hipLaunchKernelGGL(k_unpack_keys, dim3(grid_for(M.n_union)), dim3(256), 0, M.stream, (const unsigned long long *)M.uniq.p, M.n_union, M.uq.p, M.uc.p);
    GHIP(nullptr, M, hipGetLastError());
  }
  return APSS_OK;
}

// the phase's results on the row range's first member -- (query row, candidate slot, score), n of them, on M's device -- into
// the row range's list of triples (grids); the query side's ids are the handle's view of its last query batch
int32_t append_triples(apss_group::Member &M, apss_group::Range &R, const int32_t *q_row, const int32_t *c_slot, const float *score,
                       int64_t n, bool mirrored) {
  if (n == 0) return APSS_OK;
  const int64_t add = mirrored ? 2 * n : n;
  const int64_t *d_store = nullptr, *d_query = nullptr;
  int32_t rc = apss_ext_ids_dev(M.h, &d_store, &d_query);
  if (rc != APSS_OK || !d_store || !d_query) return mfail(M, APSS_E_STATE, "the member's external ids are gone");
  GHIP(nullptr, M, apss::grow_all(apss::kGrowGroupKeep, (size_t)(R.n_tri + add), (size_t)R.n_tri, M.stream, nullptr, R.tri_q, R.tri_c, R.tri_s));
  hipLaunchKernelGGL(k_triples, dim3(grid_for(n)), dim3(256), 0, M.stream, q_row, c_slot, score, d_query, d_store, n, mirrored ? 1 : 0,
                     R.tri_q.p + R.n_tri, R.tri_c.p + R.n_tri, R.tri_s.p + R.n_tri);
  GHIP(nullptr, M, hipGetLastError());
  GHIP(nullptr, M, hipStreamSynchronize(M.stream));  // (the next phase's handle call replaces the views read here)
  R.n_tri += add;
  if (mirrored) R.mirrored += n;
  return APSS_OK;
}

// ---- one phase of a call, as one member sees it: the stages below take this context, member_phase sequences them
struct Phase {
  apss_group *g;
  apss_group::Member &M, *peers;  // M = peers[i] of the row range's T members, by term range
  apss_group::Range &R;
  int T, i, mode;                 // (mode as CallCtx::mode)
  const MemberBatch &b;           // the phase's batch
  bool mirrored;
  Lockstep &ls;
  apss::ExchangeOffsets x;        // member k's candidates sit at x.off[k] of every member's key buffer
  int32_t (*gather)(Phase &) = nullptr, (*reduce)(Phase &) = nullptr;  // the exchange's transport (g->exchange)
  const float *total_score = nullptr;                                  // the reduced scores, once `reduce` has run
  Clock::time_point tx;                                                // the exchange began
};

// all-gather of the candidate lists, in place: member k's list sits at off[k] in every member's buffer
int32_t gather_rccl(Phase &P) {
  apss_group::Member &M = P.M;
  Rccl *r = load_rccl();
  ncclResult_t nr = r->GroupStart();
  for (int k = 0; k < P.T && nr == ncclSuccess; ++k) {
    const int64_t nk = P.peers[k].n_cand;
    if (nk > 0) nr = r->Broadcast(M.keys.p + P.x.off[(size_t)k], M.keys.p + P.x.off[(size_t)k], (size_t)nk, ncclUint64, k, M.comm, M.stream);
  }
  const ncclResult_t ne = r->GroupEnd();
  if (nr == ncclSuccess) nr = ne;
  if (nr != ncclSuccess) return mfail(M, APSS_E_DEVICE, std::string("RCCL all-gather of candidate lists: ") + r->GetErrorString(nr));
  return APSS_OK;
}

int32_t gather_copies(Phase &P) {
  apss_group::Member &M = P.M;
  int32_t rc = APSS_OK;
  for (int k = 0; k < P.T && rc == APSS_OK; ++k) {
    const int64_t nk = P.peers[k].n_cand;
    if (k == P.i || nk == 0) continue;
    const hipError_t e = hipMemcpyAsync(M.keys.p + P.x.off[(size_t)k], P.peers[k].keys.p + P.x.off[(size_t)k], (size_t)nk * sizeof(unsigned long long),
                                        hipMemcpyDefault, M.stream);
    if (e != hipSuccess) rc = mfail(M, APSS_E_DEVICE, std::string("candidate list copy: ") + hipGetErrorString(e));
  }
  return rc;
}

// B3: gather, then the sorted union (the same list in the same order on every member), then this member's exact partial score
// of every pair
int32_t phase_gather_union_partials(Phase &P) {
  apss_group::Member &M = P.M;
  int32_t rc = P.gather(P);
  // (query rows are rows of the PHASE's batch: a span or an outside batch)
  if (rc == APSS_OK) rc = member_union(M, P.x.total, apss::exchange_key_bits(P.b.n));
  if (rc == APSS_OK && M.n_union > 0) {
    const auto tp = Clock::now();
    rc = apss_partial_scores_dev(M.h, M.n_union, M.uq.p, M.uc.p, M.partial.p);  // (synchronises the member's stream)
    if (rc != APSS_OK) M.err = apss_last_error(M.h);
    M.partial_ms += ms_since(tp);
  }
  return rc;
}

// B3b: the members agree on the union's size.  It cannot fail -- the same sort of the same keys -- and is checked because a
// collective of unequal counts hangs: the decision to run the collective is this barrier's, the same on every member.
int32_t phase_agree(Phase &P) {
  return P.peers[0].n_union == P.M.n_union ? APSS_OK : mfail(P.M, APSS_E_STATE, "members disagree on the candidate union");
}

// all-reduce(SUM) of the partial scores: every member of the RCCL exchange holds the sums ...
int32_t reduce_rccl(Phase &P) {
  apss_group::Member &M = P.M;
  Rccl *r = load_rccl();
  const ncclResult_t nr = r->AllReduce(M.partial.p, M.sum.p, (size_t)M.n_union, ncclFloat, ncclSum, M.comm, M.stream);
  if (nr != ncclSuccess) return mfail(M, APSS_E_DEVICE, std::string("RCCL all-reduce of partial scores: ") + r->GetErrorString(nr));
  P.total_score = M.sum.p;
  return APSS_OK;
}

// ... the copies exchange sums on the row range's first member only, which reads its peers' vectors
int32_t reduce_copies(Phase &P) {
  apss_group::Member &M = P.M;
  if (P.i != 0) return APSS_OK;
  const int64_t nu = M.n_union;
  hipError_t e = hipMemcpyAsync(M.sum.p, M.partial.p, (size_t)nu * sizeof(float), hipMemcpyDeviceToDevice, M.stream);
  for (int k = 1; k < P.T && e == hipSuccess; ++k) {
    const float *src = P.peers[k].partial.p;
    if (P.peers[k].dev != M.dev) {  // (another device: bring the vector over first)
      if (ensure(M, (size_t)nu, M.stage) != APSS_OK) {
        e = hipErrorOutOfMemory;
        break;
      }
      e = hipMemcpyAsync(M.stage.p, src, (size_t)nu * sizeof(float), hipMemcpyDefault, M.stream);
      src = M.stage.p;
    }
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_accumulate, dim3(grid_for(nu)), dim3(256), 0, M.stream, M.sum.p, src, nu);
      e = hipGetLastError();
    }
  }
  if (e != hipSuccess) return mfail(M, hip_rc(e), std::string("partial score reduction: ") + hipGetErrorString(e));
  P.total_score = M.sum.p;
  return APSS_OK;
}

// The row range's FINAL LIST of a phase, finished on the range's first member -- whichever way it was produced: one member
// per row range, whose handle's answer is final as it stands, or an exchange, whose reduced scores meet the `>= theta` prune
// (k_threshold_compact), the count's read-back and, on a plain group, the per-query cut.  Either way the list then stands as
// (query row, candidate slot, score), n of them, on M's device: THIS is where a list stage of the group hooks in (removal,
// stored queries, a global top-K, components: apss_group has none of them yet).  A grid appends it to the range's triples.
int32_t range_final_list(Phase &P) {
  apss_group *g = P.g;
  apss_group::Member &M = P.M;
  apss_group::Range &R = P.R;
  const int32_t *q = nullptr, *c = nullptr;
  const float *s = nullptr;
  int64_t n = 0;
  int32_t rc;
  if (g->exchange == APSS_EXCHANGE_NONE) {
    R.n_phase = M.n_cand;
    if (g->D == 1 || M.n_cand == 0) return APSS_OK;  // (a plain group's list stays in its handle)
    if ((rc = apss_results_dev(M.h, &q, &c, &s, &n)) != APSS_OK) return mfail(M, rc, apss_last_error(M.h));
  } else {
    const int64_t nu = M.n_union;
    if ((rc = ensure(M, (size_t)std::max<int64_t>(1, nu), R.res_q, R.res_c, R.res_s)) != APSS_OK) return rc;
    GHIP(nullptr, M, hipMemsetAsync(M.count.p, 0, sizeof(unsigned long long), M.stream));
    if (nu > 0) {
      hipLaunchKernelGGL(k_threshold_compact, dim3(grid_for(nu)), dim3(256), 0, M.stream, P.total_score, (const int32_t *)M.uq.p,
                         (const int32_t *)M.uc.p, nu, (float)g->cfg.theta, R.res_q.p, R.res_c.p, R.res_s.p, M.count.p);
      GHIP(nullptr, M, hipGetLastError());
    }
    unsigned long long nres = 0;
    if ((rc = read_back(M, &nres, M.count.p)) != APSS_OK) return rc;
    R.n_phase = (int64_t)nres;
    R.union_pairs += nu;
    g->tk = apss_topk_info{};
    g->tk.pairs_over_theta = g->tk.kept = R.n_phase;
    if (g->top_k > 0 && g->D == 1) {  // the per-query cut of the group's final list (the members are term shards: no k of their own)
      const int64_t *d_store = nullptr, *d_query = nullptr;
      int64_t store_rows = 0;
      if (apss_ext_ids_dev(M.h, &d_store, &d_query) != APSS_OK || apss_size(M.h, &store_rows, nullptr) != APSS_OK || (nres > 0 && !d_store))
        return mfail(M, APSS_E_STATE, "per-query top-k: the member's external ids are gone");
      const hipError_t e = apss::topk_run(g->topk, M.stream, R.res_q.p, R.res_c.p, R.res_s.p, R.n_phase, P.b.n, d_store, store_rows, g->top_k, &g->tk);
      if (e != hipSuccess) return mfail(M, hip_rc(e), std::string("per-query top-k: ") + hipGetErrorString(e));
      if (R.n_phase > 0) {  // (kept <= n_phase: the selected list fits the buffers it replaces)
        const size_t kept = (size_t)g->tk.kept;
        GHIP(nullptr, M, hipMemcpyAsync(R.res_q.p, g->topk.out_q.p, kept * sizeof(int32_t), hipMemcpyDeviceToDevice, M.stream));
        GHIP(nullptr, M, hipMemcpyAsync(R.res_c.p, g->topk.out_c.p, kept * sizeof(int32_t), hipMemcpyDeviceToDevice, M.stream));
        GHIP(nullptr, M, hipMemcpyAsync(R.res_s.p, g->topk.out_s.p, kept * sizeof(float), hipMemcpyDeviceToDevice, M.stream));
        GHIP(nullptr, M, hipStreamSynchronize(M.stream));
        R.n_phase = g->tk.kept;
      }
    }
    q = R.res_q.p, c = R.res_c.p, s = R.res_s.p, n = R.n_phase;
  }
  return g->D > 1 ? append_triples(M, R, q, c, s, n, P.mirrored) : APSS_OK;
}

// B4: reduce, then the range's final list on the first member, or the wait for the stream on the others
int32_t phase_reduce_and_finish(Phase &P) {
  apss_group::Member &M = P.M;
  P.total_score = M.partial.p;  // (an empty union: nothing to reduce, and nothing to read)
  int32_t rc = M.n_union > 0 ? P.reduce(P) : APSS_OK;
  if (rc != APSS_OK) return rc;
  if (P.i == 0) {
    rc = range_final_list(P);
    P.R.exchange_ms += ms_since(P.tx);
  } else if (hipStreamSynchronize(M.stream) != hipSuccess) {
    rc = mfail(M, APSS_E_DEVICE, "stream synchronisation failed after the exchange");
  }
  return rc;
}

// One phase of a call for member m = (row range j, term range i): the handle call on the phase's batch, the exchange among the T
// members of the row range, the range's final list.  A plain group's call is one phase; a grid's insert-and-query is two (its
// own span, then the outside batch as a query).  This function only sequences: a line is a step of the lock-step rule behind
// one of the barriers B1 .. B4, or an exit that the members of the row range take together.  false: the call has failed.
bool member_phase(int m, CallCtx &cx, Lockstep &ls, int mode, const MemberBatch &b, bool mirrored) {
  apss_group *g = cx.g;
  const int T = g->T, j = m / T, i = m % T;
  Phase P{g, g->m[(size_t)m], &g->m[(size_t)(j * T)], g->rr[(size_t)j], T, i, mode, b, mirrored, ls};
  if (g->exchange == APSS_EXCHANGE_RCCL) P.gather = gather_rccl, P.reduce = reduce_rccl;
  else P.gather = gather_copies, P.reduce = reduce_copies;
  P.M.n_cand = P.M.n_union = 0;
  if (i == 0) P.R.n_phase = 0;
  // ---- B1: every member's candidate count (or failure) is known
  if (!ls.step(When::kUnlessFailed, [&] { return member_phase1(P.M, mode, b, mirrored); })) return false;
  if (mode == 0) return true;
  // ---- (no exchange) B2: one member per row range, its answer is final
  if (g->exchange == APSS_EXCHANGE_NONE) return ls.step(When::kAlways, [&] { return range_final_list(P); });
  P.tx = Clock::now();
  P.x = apss::exchange_offsets(T, i, [&](int k) { return P.peers[k].n_cand; });
  if (P.x.total == 0) return true;  // nothing to exchange: every member leaves together
  if (i == 0) P.R.gather_bytes += 8 * (P.x.total - P.x.least);
  // ---- B2: every list is packed (the copies exchange lets the peers read it)
  if (!ls.step(When::kAlways, [&] { return member_pack(P.M, P.x.total, P.x.mine); })) return false;
  // ---- B3: every member's partial scores are complete
  if (!ls.step(When::kAlways, [&] { return phase_gather_union_partials(P); })) return false;
  // ---- B3b: the members agree on the union (a barrier of its own: a collective of unequal counts must never start)
  if (!ls.step(When::kAlways, [&] { return phase_agree(P); })) return false;
  // ---- B4: the first member has read every peer's partial scores (copies exchange) before anyone goes on
  return ls.step(When::kAlways, [&] { return phase_reduce_and_finish(P); });
}

void member_main(int m, CallCtx *pcx) {
  CallCtx &cx = *pcx;
  apss_group *g = cx.g;
  apss_group::Member &M = g->m[(size_t)m];
  const int j = m / g->T, i = m % g->T;
  M.rc = APSS_OK;
  M.err.clear();
  M.n_cand = M.n_union = 0;
  M.member_ms = M.partial_ms = M.probe_ms = M.head_ms = 0;
  M.visits = M.dev_visits = M.touched = M.cand_sum = M.cand_max = 0;
  Lockstep ls(&cx.bar[(size_t)j], &cx.failed, &M.rc);
  ls.run(When::kAlways, [&] { return set_member_device(M); });
  const MemberBatch whole = whole_batch(cx.b, m);
  if (g->D == 1) {  // T x 1: every member holds its slice of every row, one phase
    (void)member_phase(m, cx, ls, cx.mode, whole, false);
    return;
  }
  apss_group::Range &R = g->rr[(size_t)j];
  const RangePlan &P = cx.plan[(size_t)j];
  if (cx.mode == 1) {  // frozen index: every row range that holds rows is asked the whole batch
    if (R.rows > 0) (void)member_phase(m, cx, ls, 1, whole, false);
    return;
  }
  if (cx.b.n == 0) return;  // (an empty batch: no span, no outside batch, and no row offsets to read)
  MemberBatch ph[2];  // [0] the row range's own span, [1] its outside batch
  if (cx.b.on_device) {  // (a failure is published before the row range's next barrier, B1 of the first phase below)
    ls.run(When::kUnlessFailed, [&] { return member_slice(M, cx, whole, P, ph); });
  } else {
    ph[0] = host_csr_batch(P.own);
    ph[1] = host_csr_batch(P.out);
  }
  // (which phases run follows from the plan alone, so the T members of a row range run the same ones)
  const int64_t own_n = cx.span_lo[(size_t)P.span + 1] - cx.span_lo[(size_t)P.span];
  if (own_n > 0) {  // an empty span: the row range skips the handle call
    const auto t0 = Clock::now();
    const bool ok = member_phase(m, cx, ls, cx.mode, ph[0], false);
    if (i == 0) R.own_ms = ms_since(t0);
    if (!ok) return;
  }
  if (cx.mode == 2 && P.out_rows > 0 && R.rows + own_n > 0) {
    const auto t0 = Clock::now();
    (void)member_phase(m, cx, ls, 1, ph[1], P.mirrored);
    if (i == 0) R.outside_ms = ms_since(t0), R.outside_rows = P.out_rows;
  }
}

// ---- re-layout (apss_group_relayout, APSS_GROUP_ADAPT_LAYOUT): decide a layout from the store (+ the incoming batch), build
// new member handles from whole rows reassembled out of the old members' slices, swap only when every member succeeded.

// whole rows of the store on one device, assembled by the first member on it and read in place by the others there
struct WholeRows {
  DevBuf<int64_t> rowptr, len, cur;
  DevBuf<int32_t> idx;
  DevBuf<float> val;
  int64_t nnz = 0;
  struct Staged {  // the copy of another device's slice
    DevBuf<int64_t> rp;
    DevBuf<int32_t> ix;
    DevBuf<float> vl;
  };
  std::vector<Staged> staged;
  DevBuf<char> scan_tmp;
};

struct RelayoutCtx {
  apss_group *g = nullptr;
  const Batch *b = nullptr;             // the incoming batch of the call that triggered it (NULL: apss_group_relayout)
  const std::vector<int32_t> *fixed = nullptr;  // cuts to take (named, or given to apss_group_relayout)
  Barrier *bar = nullptr;
  std::atomic<int> failed{0};
  int64_t rows = 0;                     // stored rows (every member holds a slice of each)
  bool decide_df = false;
  std::vector<uint32_t> df;             // of the store: member i fills its range [cuts[i], cuts[i + 1])
  std::vector<int> builder;             // per member: the member that assembles whole rows on its device
  std::vector<WholeRows> whole;         // per member (used at the builders' indices)
  std::atomic<int64_t> bytes{0};
  Layout next;
  bool rebuild = false;
  std::vector<apss_handle *> fresh;
};

// b[n], at least 16 bytes (an empty store still has arrays to point at); a re-layout's arrays are made once, at their size
template <class T>
hipError_t dev_alloc(DevBuf<T> &b, size_t n) {
  return b.grow(apss::kGrowStage, std::max<size_t>(n, 16 / sizeof(T)), 0, nullptr, nullptr);
}

// document frequencies of member i's stored slice: its range of the store's terms (on the member's stream)
int32_t member_df(apss_group *g, int m, const int32_t *cuts, uint32_t *df_range) {
  apss_group::Member &M = g->m[(size_t)m];
  const int i = m % g->T;
  const int32_t lo = g->T == 1 ? 0 : cuts[i], hi = g->T == 1 ? g->cfg.dim : cuts[i + 1];
  const int64_t *rp = nullptr;
  const int32_t *ix = nullptr;
  const float *vl = nullptr;
  int64_t rows = 0, nnz = 0;
  (void)apss_get_store_dev(M.h, &rp, &ix, &vl, &rows, &nnz);
  std::memset(df_range, 0, (size_t)(hi - lo) * sizeof(uint32_t));
  if (nnz == 0) return APSS_OK;
  GHIP(nullptr, M, df_hist(M, ix, nnz, lo, hi, df_range));
  return APSS_OK;
}

// whole rows on member i's device (i is the builder there): lengths, exclusive scan, then every member's slice in member order
int32_t assemble_whole(RelayoutCtx &cx, int i) {
  apss_group *g = cx.g;
  apss_group::Member &M = g->m[(size_t)i];
  WholeRows &w = cx.whole[(size_t)i];
  const int64_t rows = cx.rows;
  GHIP(nullptr, M, dev_alloc(w.rowptr, (size_t)(rows + 1)));
  GHIP(nullptr, M, dev_alloc(w.len, (size_t)(rows + 1)));
  GHIP(nullptr, M, dev_alloc(w.cur, (size_t)(rows + 1)));
  GHIP(nullptr, M, hipMemsetAsync(w.len.p, 0, (size_t)(rows + 1) * sizeof(int64_t), M.stream));
  struct Slice {
    const int64_t *rp;
    const int32_t *ix;
    const float *vl;
  };
  std::vector<Slice> sl((size_t)g->T);
  for (int k = 0; k < g->T; ++k) {
    const apss_group::Member &P = g->m[(size_t)k];
    Slice &s = sl[(size_t)k];
    int64_t r = 0, z = 0;
    (void)apss_get_store_dev(P.h, &s.rp, &s.ix, &s.vl, &r, &z);
    if (r != rows || !s.rp)
      return mfail(M, APSS_E_STATE, "member " + std::to_string(k) + " holds " + std::to_string(r) + " rows, member 0 " + std::to_string(rows));
    if (P.dev != M.dev) {  // another device's slice: brought over first (peer copy, or staged by the runtime)
      w.staged.emplace_back();
      WholeRows::Staged &c = w.staged.back();
      GHIP(nullptr, M, dev_alloc(c.rp, (size_t)(rows + 1)));
      GHIP(nullptr, M, dev_alloc(c.ix, (size_t)z));
      GHIP(nullptr, M, dev_alloc(c.vl, (size_t)z));
      GHIP(nullptr, M, hipMemcpyAsync(c.rp.p, s.rp, (size_t)(rows + 1) * sizeof(int64_t), hipMemcpyDefault, M.stream));
      if (z > 0) {
        GHIP(nullptr, M, hipMemcpyAsync(c.ix.p, s.ix, (size_t)z * sizeof(int32_t), hipMemcpyDefault, M.stream));
        GHIP(nullptr, M, hipMemcpyAsync(c.vl.p, s.vl, (size_t)z * sizeof(float), hipMemcpyDefault, M.stream));
      }
      cx.bytes += (rows + 1) * (int64_t)sizeof(int64_t) + z * (int64_t)(sizeof(int32_t) + sizeof(float));
      s = Slice{c.rp.p, c.ix.p, c.vl.p};
    }
    hipLaunchKernelGGL(k_row_len_add, dim3(grid_for(rows)), dim3(256), 0, M.stream, s.rp, rows, w.len.p);
    GHIP(nullptr, M, hipGetLastError());
  }
  size_t tmp_bytes = 0;
  GHIP(nullptr, M, rocprim::exclusive_scan(nullptr, tmp_bytes, w.len.p, w.rowptr.p, (int64_t)0, (size_t)(rows + 1), rocprim::plus<int64_t>(), M.stream));
  GHIP(nullptr, M, dev_alloc(w.scan_tmp, tmp_bytes));
  GHIP(nullptr, M, rocprim::exclusive_scan((void *)w.scan_tmp.p, tmp_bytes, w.len.p, w.rowptr.p, (int64_t)0, (size_t)(rows + 1), rocprim::plus<int64_t>(), M.stream));
  GHIP(nullptr, M, hipMemcpyAsync(&w.nnz, w.rowptr.p + rows, sizeof(int64_t), hipMemcpyDeviceToHost, M.stream));
  GHIP(nullptr, M, hipMemcpyAsync(w.cur.p, w.rowptr.p, (size_t)rows * sizeof(int64_t), hipMemcpyDeviceToDevice, M.stream));
  GHIP(nullptr, M, hipStreamSynchronize(M.stream));
  GHIP(nullptr, M, dev_alloc(w.idx, (size_t)w.nnz));
  GHIP(nullptr, M, dev_alloc(w.val, (size_t)w.nnz));
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div(rows, 256), 8192));  // 4 waves x 64 rows
  for (int k = 0; k < g->T; ++k) {
    const Slice &s = sl[(size_t)k];
    hipLaunchKernelGGL(k_merge_slice, dim3(blocks), dim3(256), 0, M.stream, s.rp, s.ix, s.vl, rows, w.cur.p, w.idx.p, w.val.p);
    GHIP(nullptr, M, hipGetLastError());
  }
  GHIP(nullptr, M, hipStreamSynchronize(M.stream));  // (the other members on this device read the rows on their own streams)
  return APSS_OK;
}

// phase B: member 0 decides (the head policy runs on its device over whole rows)
int32_t relayout_decide(RelayoutCtx &cx) {
  apss_group *g = cx.g;
  apss_group::Member &M = g->m[0];
  const WholeRows &w = cx.whole[(size_t)cx.builder[0]];
  const int64_t batch_n = cx.b ? cx.b->n : 0;
  auto feed = [&](apss_handle *ph) -> int32_t {
    const int64_t s_rows = std::min<int64_t>(cx.rows, 131072);
    if (s_rows > 0) {
      int64_t s_nnz = 0;
      if (hipMemcpy(&s_nnz, w.rowptr.p + s_rows, sizeof(int64_t), hipMemcpyDeviceToHost) != hipSuccess) return APSS_E_DEVICE;
      const int64_t *d_ext = nullptr;
      (void)apss_ext_ids_dev(M.h, &d_ext, nullptr);
      const int32_t rc = apss_insert_stored_dev(ph, s_rows, s_nnz, w.rowptr.p, w.idx.p, w.val.p, d_ext);
      if (rc != APSS_OK) return rc;
    }
    return cx.b ? feed_batch(g, ph, *cx.b, std::min<int64_t>(batch_n, 131072 - s_rows)) : APSS_OK;
  };
  int32_t rc = APSS_OK;
  if (cx.decide_df && cx.b) rc = add_batch_df(g, *cx.b, cx.df);
  if (rc == APSS_OK) rc = decide_layout(g, cx.df, cx.rows + batch_n, cx.fixed, feed, cx.next);
  if (rc != APSS_OK) M.err = g->err;
  else cx.rebuild = cx.next.cuts != g->cuts || cx.next.head != g->head;
  return rc;
}

// phase C: a new handle for this member in the new layout, filled with the whole rows of its device
int32_t relayout_refill(RelayoutCtx &cx, int i) {
  apss_group *g = cx.g;
  apss_group::Member &M = g->m[(size_t)i];
  std::string err;
  int32_t rc = create_member_handle(g, i, cx.next, &cx.fresh[(size_t)i], err);
  if (rc == APSS_OK && cx.rows > 0) {
    const WholeRows &w = cx.whole[(size_t)cx.builder[(size_t)i]];
    const int64_t *d_ext = nullptr;
    (void)apss_ext_ids_dev(M.h, &d_ext, nullptr);
    const bool inject = g->relayout_fail == i;  // (the test hook: the handle's own argument check refuses the call)
    rc = apss_insert_stored_dev(cx.fresh[(size_t)i], inject ? -1 : cx.rows, w.nnz, w.rowptr.p, w.idx.p, w.val.p, d_ext);
    if (rc != APSS_OK) err = std::string(inject ? "APSS_DEBUG relayout_fail: " : "") + apss_last_error(cx.fresh[(size_t)i]);
    else if (hipStreamSynchronize(M.stream) != hipSuccess) rc = APSS_E_DEVICE, err = "stream synchronisation failed after the re-insert";
  }
  if (rc != APSS_OK) M.err = "re-layout: " + err;
  return rc;
}

// One member's share of a re-layout: three steps of the lock-step rule (apss_lockstep.hpp) behind the barriers R1 .. R3.
// This function only sequences.
void relayout_main(int i, RelayoutCtx *pcx) {
  RelayoutCtx &cx = *pcx;
  apss_group *g = cx.g;
  apss_group::Member &M = g->m[(size_t)i];
  M.rc = APSS_OK;
  M.err.clear();
  Lockstep ls(cx.bar, &cx.failed, &M.rc);
  ls.run(When::kAlways, [&] { return set_member_device(M); });
  // ---- phase A: this member's document frequencies; the builder of each device assembles the whole rows there
  ls.run(When::kUnlessFailed, [&] { return cx.decide_df ? member_df(g, i, g->cuts.data(), cx.df.data() + (g->T == 1 ? 0 : g->cuts[(size_t)i])) : APSS_OK; });
  const bool swap =
      // ---- R1: document frequencies and whole rows are complete
      ls.step(When::kUnlessFailed, [&] { return cx.rows > 0 && cx.builder[(size_t)i] == i ? assemble_whole(cx, i) : APSS_OK; }) &&
      // ---- R2: the decision is known
      ls.step(When::kAlways, [&] { return i == 0 ? relayout_decide(cx) : APSS_OK; }) && cx.rebuild &&
      // ---- R3: every new member is filled (or one failed): swap together, or not at all
      ls.step(When::kAlways, [&] { return relayout_refill(cx, i); });
  if (cx.builder[(size_t)i] == i) cx.whole[(size_t)i] = WholeRows{};  // (whichever barrier the re-layout ended at)
  if (swap) {
    apss_destroy(M.h);
    M.h = cx.fresh[(size_t)i];
  } else if (cx.fresh[(size_t)i]) {
    apss_destroy(cx.fresh[(size_t)i]);
  }
  cx.fresh[(size_t)i] = nullptr;
}

bool layout_can_change(const apss_group *g, bool cuts_given) { return g->T > 1 && (!(g->cuts_named || cuts_given) || head_possible(g)); }

int64_t next_eval_rows(const apss_group *g) {
  if (!(g->flags & APSS_GROUP_ADAPT_LAYOUT) || !g->created || !layout_can_change(g, false)) return 0;
  return std::max<int64_t>(1024, 2 * g->layout_rows);
}

// decide again on the store (+ b) and rebuild the store when the layout changes; cuts: taken as given (NULL: named or decided)
int32_t relayout(apss_group *g, const std::vector<int32_t> *cuts, const Batch *b) {
  const auto t0 = Clock::now();
  const int T = g->T;
  RelayoutCtx cx;
  cx.g = g;
  cx.b = b;
  cx.fixed = cuts ? cuts : (g->cuts_named ? &g->cuts : nullptr);
  (void)apss_size(g->m[0].h, &cx.rows, nullptr);
  const int64_t decided_on = cx.rows + (b ? b->n : 0);
  if (layout_can_change(g, cuts != nullptr) || (cuts && *cuts != g->cuts)) {
    cx.decide_df = needs_df(g, cx.fixed != nullptr);
    if (cx.decide_df) cx.df.assign((size_t)g->cfg.dim, 0u);
    cx.builder.assign((size_t)T, 0);
    for (int i = 0; i < T; ++i) {
      int k = 0;
      while (g->m[(size_t)k].dev != g->m[(size_t)i].dev) ++k;
      cx.builder[(size_t)i] = k;
    }
    cx.whole.resize((size_t)T);
    cx.fresh.assign((size_t)T, nullptr);
    Barrier bar(T, &cx.failed);
    cx.bar = &bar;
    const int32_t rc = run_members(g, T, relayout_main, &cx, "a member failed during the re-layout");
    if (rc != APSS_OK) return rc;
    if (cx.rebuild) {
      g->cuts = cx.next.cuts;
      g->head = cx.next.head;
      ++g->relayouts;
      g->relayout_bytes += cx.bytes.load();
      g->n_res = -1;  // (the old handles held the last results)
      g->results_in_handle = false;
    }
  }
  ++g->evaluations;
  g->layout_rows = decided_on;
  g->last_relayout_ms = ms_since(t0);
  g->total_relayout_ms += g->last_relayout_ms;
  return APSS_OK;
}

// span k of a batch of n rows cut D ways: [ceil(n k / D), ceil(n (k + 1) / D)) -- the longer spans first, so a single row is span 0
std::vector<int64_t> span_bounds(int64_t n, int D) {
  std::vector<int64_t> lo((size_t)D + 1, 0);
  for (int k = 0; k <= D; ++k) lo[(size_t)k] = ceil_div(n * k, D);
  return lo;
}

// grids: which span every row range stores and which spans it meets as its outside batch (include/apss.h, GRIDS)
void plan_ranges(apss_group *g, CallCtx &cx) {
  const int D = g->D;
  cx.span_lo = span_bounds(cx.b.n, D);
  cx.plan.assign((size_t)D, RangePlan{});
  if (cx.mode == 1) return;  // (a query of the frozen index: the whole batch to every row range)
  int first = 0;
  bool empty = true;
  for (int j = 0; j < D; ++j) {
    if (g->rr[(size_t)j].rows < g->rr[(size_t)first].rows) first = j;
    empty = empty && g->rr[(size_t)j].rows == 0;
  }
  // a whole-store join may use the symmetry across the row ranges; onto a store, half spans would lose the pairs of a skipped
  // span's rows with this range's STORED rows
  const bool symmetric = cx.mode == 2 && empty && !(g->flags & APSS_GROUP_NO_SYMMETRIC_RANGES) && !(g->cfg.flags & APSS_FLAG_NO_SYMMETRY);
  if (cx.mode == 2) g->symmetric_ranges = symmetric;
  for (int j = 0; j < D; ++j) {
    RangePlan &P = cx.plan[(size_t)j];
    P.span = ((j - first) % D + D) % D;
    if (cx.mode == 2) {
      if (symmetric) {  // (first = 0 here: span k is row range k) the (D - 1) / 2 ranges before j, cyclically ...
        for (int d = 1; d <= (D - 1) / 2; ++d) P.outside.push_back(((j - d) % D + D) % D);
        const int k = (j + D / 2) % D;  // ... and for even D the opposite range, taken by the lower-numbered of the two
        if (D % 2 == 0 && j < k) P.outside.push_back(k);
        std::sort(P.outside.begin(), P.outside.end());
        P.mirrored = true;
      } else {
        for (int k = 0; k < D; ++k)
          if (k != P.span) P.outside.push_back(k);
      }
      for (int k : P.outside) P.out_rows += cx.span_lo[(size_t)k + 1] - cx.span_lo[(size_t)k];
    }
    if (!cx.b.on_device) {  // the host-pointer entry points slice here, once per row range
      append_span(P.own, cx.b, cx.span_lo[(size_t)P.span], cx.span_lo[(size_t)P.span + 1]);
      for (int k : P.outside)
        if (cx.span_lo[(size_t)k + 1] > cx.span_lo[(size_t)k]) append_span(P.out, cx.b, cx.span_lo[(size_t)k], cx.span_lo[(size_t)k + 1]);
      if (P.out.rowptr.empty()) P.out.rowptr.push_back(0);
    }
  }
}

int32_t run_call(apss_group *g, int mode, const Batch &b, int64_t *n_results) {
  if (n_results) *n_results = 0;
  g->err.clear();
  if (b.n < 0 || b.nnz < 0) return gfail(g, APSS_E_INVALID, "negative size");
  g->n_res = -1;
  g->results_in_handle = false;
  const int T = g->T, D = g->D, n_members = T * D;
  for (apss_group::Range &R : g->rr) {
    R.n_phase = R.n_tri = 0;
    R.union_pairs = R.gather_bytes = R.mirrored = R.outside_rows = 0;
    R.own_ms = R.outside_ms = R.exchange_ms = 0;
  }
  if (!g->created) {
    if (mode == 1 || b.n == 0) {  // nothing is indexed yet: an empty answer, no layout decided
      g->n_res = mode == 0 ? -1 : 0;
      return APSS_OK;
    }
    const int32_t rc = create_members(g, b);
    if (rc != APSS_OK) {
      for (apss_group::Member &M : g->m) {
        if (M.h) apss_destroy(M.h);
        M.h = nullptr;
      }
      return rc;
    }
  } else if (mode != 1 && b.n > 0) {
    // APSS_GROUP_ADAPT_LAYOUT: the store doubled since the layout was decided -- decide again on the store plus this batch,
    // rebuild, and let the batch land in the new layout
    const int64_t at = next_eval_rows(g);
    if (at > 0 && g->n_rows + b.n >= at) {
      const int32_t rc = relayout(g, nullptr, &b);
      if (rc != APSS_OK) return rc;
    }
  }
  const auto t0 = Clock::now();
  CallCtx cx;
  cx.g = g;
  cx.mode = mode;
  cx.b = b;
  if (D > 1) plan_ranges(g, cx);
  for (int j = 0; j < D; ++j) cx.bar.emplace_back(T, &cx.failed);
  const int32_t rc = run_members(g, n_members, member_main, &cx, "a member failed");
  if (rc != APSS_OK) {
    g->n_res = -1;
    return rc;
  }
  if (mode != 1) {
    g->n_rows = 0;
    for (int j = 0; j < D; ++j) {
      int64_t rows = 0;
      (void)apss_size(g->m[(size_t)(j * T)].h, &rows, nullptr);
      g->rr[(size_t)j].rows = rows;
      g->n_rows += rows;
    }
  }
  // statistics of the call
  apss_group_stats &st = g->st;
  const int32_t keep_size = st.struct_size;
  st = apss_group_stats{};
  st.struct_size = keep_size;
  st.n_members = n_members;
  st.exchange = g->exchange;
  st.head_terms = (int32_t)g->head.size();
  st.rows = g->n_rows;
  for (int i = 0; i <= T && i <= APSS_GROUP_MAX_MEMBERS; ++i) st.term_cuts[i] = g->cuts[(size_t)i];
  int64_t least = INT64_MAX;
  for (int m = 0; m < n_members; ++m) {
    apss_group::Member &M = g->m[(size_t)m];
    apss_stats ms{};
    ms.struct_size = (int32_t)sizeof(apss_stats);
    (void)apss_stats_get(M.h, &ms);
    st.nnz += ms.nnz;
    if (mode != 0) {
      st.posting_visits += M.visits;
      st.device_posting_visits += M.dev_visits;
      st.member_touched_pairs += M.touched;
      st.candidates_sum += M.cand_sum;
      st.candidates_max = std::max(st.candidates_max, M.cand_max);
      st.probe_ms_max = std::max(st.probe_ms_max, M.probe_ms);
      st.head_ms_max = std::max(st.head_ms_max, M.head_ms);
      least = std::min(least, M.cand_sum);
    }
    st.build_ms_max = std::max(st.build_ms_max, ms.build_ms);
    st.member_ms_max = std::max(st.member_ms_max, M.member_ms);
    st.partial_ms_max = std::max(st.partial_ms_max, M.partial_ms);
  }
  if (mode != 0) {
    if (D > 1) {  // the row ranges' triples, one list after the other
      g->n_res = 0;
      for (const apss_group::Range &R : g->rr) {
        g->n_res += R.n_tri;
        st.union_pairs += g->exchange == APSS_EXCHANGE_NONE ? R.n_tri - R.mirrored : R.union_pairs;
        st.all_gather_bytes += R.gather_bytes;
        st.exchange_ms = std::max(st.exchange_ms, R.exchange_ms);
      }
      if (g->exchange != APSS_EXCHANGE_NONE) st.all_reduce_bytes = 4 * st.union_pairs;
    } else if (g->exchange == APSS_EXCHANGE_NONE) {
      g->results_in_handle = true;
      g->n_res = g->m[0].n_cand;
      st.union_pairs = g->n_res;
    } else {
      g->n_res = g->rr[0].n_phase;
      st.union_pairs = g->m[0].n_union;
      st.all_gather_bytes = 8 * (st.candidates_sum - least);
      st.all_reduce_bytes = 4 * st.union_pairs;
      st.exchange_ms = g->rr[0].exchange_ms;
    }
    st.result_pairs = g->n_res;
    if (n_results) *n_results = g->n_res;
  }
  if (mode == 1) g->symmetric_ranges = false;
  st.total_ms = ms_since(t0);
  return APSS_OK;
}

int32_t validate_host(apss_group *g, int64_t n, const int64_t *rowptr, const int32_t *indices, const double *values, const int64_t *ext) {
  if (n < 0) return gfail(g, APSS_E_INVALID, "negative row count");
  if (n == 0) return APSS_OK;
  if (!rowptr || !ext) return gfail(g, APSS_E_INVALID, "null rowptr / ext_ids");
  if (rowptr[0] != 0) return gfail(g, APSS_E_INVALID, "rowptr[0] must be 0");
  for (int64_t i = 0; i < n; ++i)
    if (rowptr[i + 1] < rowptr[i]) return gfail(g, APSS_E_INVALID, "rowptr must be non-decreasing");
  if (rowptr[n] > 0 && (!indices || !values)) return gfail(g, APSS_E_INVALID, "null indices / values");
  return APSS_OK;
}

Batch host_batch(int64_t n, const int64_t *rowptr, const int32_t *indices, const double *values, const int64_t *ext) {
  Batch b;
  b.n = n;
  b.nnz = n > 0 ? rowptr[n] : 0;
  b.rowptr = rowptr;
  b.indices = indices;
  b.values = values;
  b.ext = ext;
  return b;
}

}  // namespace

extern "C" {

int32_t apss_group_create(const apss_config *cfg, int32_t n_members, const int32_t *device_ids, uint32_t group_flags, apss_group **out) {
  return apss_group_create_grid(cfg, n_members, 1, device_ids, group_flags, out);
}

int32_t apss_group_create_grid(const apss_config *cfg, int32_t n_term_ranges, int32_t n_row_ranges, const int32_t *device_ids,
                               uint32_t group_flags, apss_group **out) {
  if (!cfg || !out || !device_ids) {
    g_group_create_error = "null argument";
    return APSS_E_INVALID;
  }
  *out = nullptr;
  if (cfg->struct_size != (int32_t)sizeof(apss_config)) {
    g_group_create_error = "apss_config.struct_size mismatch";
    return APSS_E_INVALID;
  }
  if (n_term_ranges < 1 || n_row_ranges < 1 || (int64_t)n_term_ranges * n_row_ranges > APSS_GROUP_MAX_MEMBERS) {
    g_group_create_error = n_row_ranges == 1 ? "n_members must be in [1, 64]" : "term ranges x row ranges must be in [1, 64], each at least 1";
    return APSS_E_INVALID;
  }
  const int32_t n_members = n_term_ranges * n_row_ranges;
  if (cfg->dim <= 0 || !std::isfinite(cfg->theta)) {
    g_group_create_error = "dim must be > 0 and theta finite";
    return APSS_E_INVALID;
  }
  if (n_row_ranges > 1 && (group_flags & APSS_GROUP_ADAPT_LAYOUT)) {
    g_group_create_error = "APSS_GROUP_ADAPT_LAYOUT is not supported with more than one row range (name the cuts: apss_group_set_term_cuts)";
    return APSS_E_UNSUPPORTED;
  }
  if (n_term_ranges > 1 && !(cfg->theta > 0.0)) {
    g_group_create_error = "term-range shards need theta > 0 (candidate test p_g >= theta*|q_g|*|c_g|)";
    return APSS_E_UNSUPPORTED;
  }
  int ndev = 0;
  const hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    g_group_create_error = std::string("no usable HIP device (there is no CPU fallback): ") + (e != hipSuccess ? hipGetErrorString(e) : "none found");
    return APSS_E_DEVICE;
  }
  apss_group *g = new (std::nothrow) apss_group();
  if (!g) return APSS_E_NOMEM;
  g->cfg = *cfg;
  g->flags = group_flags;
  g->T = n_term_ranges;
  g->D = n_row_ranges;
  g->m.resize((size_t)n_members);
  g->rr.resize((size_t)n_row_ranges);
  g->st.struct_size = (int32_t)sizeof(apss_group_stats);
  if (const char *dbg = getenv("APSS_DEBUG")) {  // (the group's only token; the handles skip it)
    const std::string s = std::string(",") + dbg;
    const size_t at = s.find(",relayout_fail=");
    if (at != std::string::npos) g->relayout_fail = atoi(s.c_str() + at + 15);
  }
  for (int i = 0; i < n_members; ++i) {
    const int d = device_ids[i];
    if (d < 0 || d >= ndev) {
      g_group_create_error = "device ordinal out of range";
      apss_group_destroy(g);
      return APSS_E_DEVICE;
    }
    for (int k = i - i % n_term_ranges; k < i; ++k)  // (the exchange runs among the members of ONE row range)
      if (g->m[(size_t)k].dev == d) g->distinct_devices = false;
    g->m[(size_t)i].dev = d;
    if (hipSetDevice(d) != hipSuccess || g->m[(size_t)i].stream.make() != hipSuccess) {
      g_group_create_error = "HIP stream creation failed";
      apss_group_destroy(g);
      return APSS_E_DEVICE;
    }
  }
  *out = g;
  return APSS_OK;
}

void apss_group_destroy(apss_group *g) {
  if (!g) return;
  Rccl *r = g->exchange == APSS_EXCHANGE_RCCL ? load_rccl() : nullptr;
  for (apss_group::Member &M : g->m) {
    (void)hipSetDevice(M.dev);
    if (M.stream.made()) (void)hipStreamSynchronize(M.stream);
    if (M.comm && r && r->lib) (void)r->CommDestroy(M.comm);
    if (M.h) apss_destroy(M.h);
    static_cast<apss_group::MemberBufs &>(M) = {};
  }
  if (!g->m.empty()) {
    (void)hipSetDevice(g->m[0].dev);
    g->topk = {};
  }
  for (size_t j = 0; j < g->rr.size() && j * (size_t)g->T < g->m.size(); ++j) {
    (void)hipSetDevice(g->m[j * (size_t)g->T].dev);
    static_cast<apss_group::RangeBufs &>(g->rr[j]) = {};
  }
  if (!g->m.empty()) (void)hipSetDevice(g->m[0].dev);
  g->ext = {};
  for (apss_group::Member &M : g->m) {
    (void)hipSetDevice(M.dev);
    M.stream = {};
  }
  delete g;
}

const char *apss_group_last_error(const apss_group *g) { return g ? g->err.c_str() : g_group_create_error.c_str(); }

int32_t apss_group_set_term_cuts(apss_group *g, const int32_t *cuts) {
  if (!g || !cuts) return APSS_E_INVALID;
  if (g->created) return gfail(g, APSS_E_STATE, "apss_group_set_term_cuts: the members exist already (name the cuts before the first insert)");
  if (cuts[0] != 0 || cuts[g->T] != g->cfg.dim) return gfail(g, APSS_E_INVALID, "apss_group_set_term_cuts: cuts[0] = 0 and cuts[n_members] = dim");
  for (int i = 0; i < g->T; ++i)
    if (cuts[i] >= cuts[i + 1]) return gfail(g, APSS_E_INVALID, "apss_group_set_term_cuts: cuts must be strictly increasing");
  g->cuts.assign(cuts, cuts + g->T + 1);
  g->cuts_named = true;
  return APSS_OK;
}

int32_t apss_group_insert(apss_group *g, int64_t n, const int64_t *rowptr, const int32_t *indices, const double *values,
                          const int64_t *ext_ids) {
  if (!g) return APSS_E_INVALID;
  int32_t rc = validate_host(g, n, rowptr, indices, values, ext_ids);
  if (rc != APSS_OK) return rc;
  if (n == 0) return APSS_OK;
  return run_call(g, 0, host_batch(n, rowptr, indices, values, ext_ids), nullptr);
}

int32_t apss_group_query(apss_group *g, int64_t n, const int64_t *rowptr, const int32_t *indices, const double *values,
                         const int64_t *ext_ids, int64_t *n_results) {
  if (!g) return APSS_E_INVALID;
  int32_t rc = validate_host(g, n, rowptr, indices, values, ext_ids);
  if (rc != APSS_OK) return rc;
  return run_call(g, 1, host_batch(n, rowptr, indices, values, ext_ids), n_results);
}

int32_t apss_group_insert_and_query(apss_group *g, int64_t n, const int64_t *rowptr, const int32_t *indices, const double *values,
                                    const int64_t *ext_ids, int64_t *n_results) {
  if (!g) return APSS_E_INVALID;
  int32_t rc = validate_host(g, n, rowptr, indices, values, ext_ids);
  if (rc != APSS_OK) return rc;
  return run_call(g, 2, host_batch(n, rowptr, indices, values, ext_ids), n_results);
}

int32_t apss_group_insert_and_query_dev(apss_group *g, int64_t n, int64_t nnz, const int64_t *const *d_rowptr,
                                        const int32_t *const *d_indices, const float *const *d_values,
                                        const int64_t *const *d_ext_ids, int64_t *n_results) {
  if (!g) return APSS_E_INVALID;
  if (n < 0 || nnz < 0) return gfail(g, APSS_E_INVALID, "negative size");
  if (n > 0) {
    if (!d_rowptr || !d_indices || !d_values || !d_ext_ids) return gfail(g, APSS_E_INVALID, "null pointer table");
    for (int i = 0; i < g->T * g->D; ++i)
      if (!d_rowptr[i] || !d_ext_ids[i] || (nnz > 0 && (!d_indices[i] || !d_values[i]))) return gfail(g, APSS_E_INVALID, "null device pointer");
  }
  Batch b;
  b.n = n;
  b.nnz = nnz;
  b.d_rowptr = d_rowptr;
  b.d_indices = d_indices;
  b.d_values = d_values;
  b.d_ext = d_ext_ids;
  b.on_device = true;
  return run_call(g, 2, b, n_results);
}

int32_t apss_group_clear(apss_group *g) {
  if (!g) return APSS_E_INVALID;
  g->n_res = -1;
  g->results_in_handle = false;
  g->n_rows = 0;
  for (apss_group::Range &R : g->rr) R.rows = R.n_tri = R.n_phase = 0;
  for (int i = 0; i < g->T * g->D; ++i) {
    apss_group::Member &M = g->m[(size_t)i];
    if (!M.h) continue;
    const int32_t rc = apss_clear(M.h);
    if (rc != APSS_OK) return gfail(g, rc, "member " + std::to_string(i) + ": " + apss_last_error(M.h));
  }
  return APSS_OK;
}

int32_t apss_group_relayout(apss_group *g, const int32_t *cuts) {
  if (!g) return APSS_E_INVALID;
  g->err.clear();
  if (g->D > 1) return gfail(g, APSS_E_UNSUPPORTED, "apss_group_relayout: not supported on a grid with more than one row range");
  if (!g->created || g->n_rows == 0) return gfail(g, APSS_E_STATE, "apss_group_relayout: the group holds no rows");
  std::vector<int32_t> given;
  if (cuts) {
    if (cuts[0] != 0 || cuts[g->T] != g->cfg.dim) return gfail(g, APSS_E_INVALID, "apss_group_relayout: cuts[0] = 0 and cuts[n_members] = dim");
    for (int i = 0; i < g->T; ++i)
      if (cuts[i] >= cuts[i + 1]) return gfail(g, APSS_E_INVALID, "apss_group_relayout: cuts must be strictly increasing");
    given.assign(cuts, cuts + g->T + 1);
  }
  return relayout(g, cuts ? &given : nullptr, nullptr);
}

int32_t apss_group_layout_get(apss_group *g, apss_group_layout *out) {
  if (!g || !out) return APSS_E_INVALID;
  const int32_t caller = out->struct_size;
  if (caller < (int32_t)(2 * sizeof(int32_t)) || caller > (1 << 16))
    return gfail(g, APSS_E_INVALID, "apss_group_layout.struct_size must be set to sizeof(apss_group_layout) before the call");
  apss_group_layout L{};
  L.n_members = g->T * g->D;
  L.layout_rows = g->layout_rows;
  L.next_eval_rows = next_eval_rows(g);
  L.evaluations = g->evaluations;
  L.relayouts = g->relayouts;
  L.last_relayout_ms = g->last_relayout_ms;
  L.total_relayout_ms = g->total_relayout_ms;
  L.relayout_bytes = g->relayout_bytes;
  L.head_terms = (int32_t)g->head.size();
  for (size_t i = 0; i < g->cuts.size() && i <= APSS_GROUP_MAX_MEMBERS; ++i) L.term_cuts[i] = g->cuts[i];
  if (g->created) {
    // sum of df^2 over each member's stored tail terms (its range without the head's): a df pass over every member's slice
    std::vector<uint32_t> df((size_t)g->cfg.dim, 0u);
    std::vector<char> in_head((size_t)g->cfg.dim, 0);
    for (int32_t t : g->head) in_head[(size_t)t] = 1;
    for (int m = 0; m < g->T * g->D; ++m) {  // (a grid: member (j, i)'s own rows, at dfsq[j * T + i])
      const int i = m % g->T;
      apss_group::Member &M = g->m[(size_t)m];
      const int32_t lo = g->T == 1 ? 0 : g->cuts[(size_t)i], hi = g->T == 1 ? g->cfg.dim : g->cuts[(size_t)i + 1];
      int32_t rc = hipSetDevice(M.dev) == hipSuccess ? APSS_OK : APSS_E_DEVICE;
      if (rc == APSS_OK) rc = member_df(g, m, g->cuts.data(), df.data() + lo);
      if (rc != APSS_OK) return gfail(g, rc, "member " + std::to_string(m) + ": " + M.err);
      double sq = 0;
      for (int32_t t = lo; t < hi; ++t)
        if (!in_head[(size_t)t]) sq += (double)df[(size_t)t] * (double)df[(size_t)t];
      L.dfsq[m] = sq;
    }
  }
  const int32_t n = std::min<int32_t>(caller, (int32_t)sizeof(apss_group_layout));
  L.struct_size = n;
  std::memcpy(out, &L, (size_t)n);
  return APSS_OK;
}

int32_t apss_group_result_count(const apss_group *g, int64_t *n_results) {
  if (!g || !n_results) return APSS_E_INVALID;
  if (g->n_res < 0) return APSS_E_STATE;
  *n_results = g->n_res;
  return APSS_OK;
}

int32_t apss_group_fetch_results(apss_group *g, int64_t offset, int64_t count, int64_t *out_q, int64_t *out_c, float *out_score) {
  if (!g) return APSS_E_INVALID;
  if (g->n_res < 0) return gfail(g, APSS_E_STATE, "no query has run on this group since the last insert");
  if (offset < 0 || count < 0 || offset + count > g->n_res) return gfail(g, APSS_E_INVALID, "fetch range out of bounds");
  if (count == 0) return APSS_OK;
  if (!out_q || !out_c || !out_score) return gfail(g, APSS_E_INVALID, "null output buffer");
  if (g->D > 1) {  // the row ranges' triples, one list after the other
    int64_t base = 0;
    for (int j = 0; j < g->D; ++j) {
      const apss_group::Range &R = g->rr[(size_t)j];
      const int64_t lo = std::max(offset, base), hi = std::min(offset + count, base + R.n_tri);
      if (lo < hi) {
        apss_group::Member &Mj = g->m[(size_t)(j * g->T)];
        const size_t n = (size_t)(hi - lo);
        auto copy = [&]() -> int32_t {
          GHIP(nullptr, Mj, hipSetDevice(Mj.dev));
          GHIP(nullptr, Mj, hipMemcpyAsync(out_q + (lo - offset), R.tri_q.p + (lo - base), n * sizeof(int64_t), hipMemcpyDeviceToHost, Mj.stream));
          GHIP(nullptr, Mj, hipMemcpyAsync(out_c + (lo - offset), R.tri_c.p + (lo - base), n * sizeof(int64_t), hipMemcpyDeviceToHost, Mj.stream));
          GHIP(nullptr, Mj, hipMemcpyAsync(out_score + (lo - offset), R.tri_s.p + (lo - base), n * sizeof(float), hipMemcpyDeviceToHost, Mj.stream));
          GHIP(nullptr, Mj, hipStreamSynchronize(Mj.stream));
          return APSS_OK;
        };
        const int32_t rc = copy();
        if (rc != APSS_OK) return gfail(g, rc, Mj.err);
      }
      base += R.n_tri;
    }
    (void)hipSetDevice(g->m[0].dev);
    return APSS_OK;
  }
  apss_group::Member &M = g->m[0];
  if (g->results_in_handle) {
    const int32_t rc = apss_fetch_results(M.h, offset, count, out_q, out_c, out_score);
    if (rc != APSS_OK) g->err = apss_last_error(M.h);
    return rc;
  }
  auto body = [&]() -> int32_t {
    GHIP(nullptr, M, hipSetDevice(M.dev));
    const int64_t *d_store = nullptr, *d_query = nullptr;
    int32_t rc = apss_ext_ids_dev(M.h, &d_store, &d_query);
    if (rc != APSS_OK || !d_store || !d_query) {
      M.err = "the members' external ids are gone (an insert since the last query-type call)";
      return APSS_E_STATE;
    }
    if ((rc = ensure(M, (size_t)count, g->ext.q, g->ext.c)) != APSS_OK) return rc;
    hipLaunchKernelGGL(k_gather_ext, dim3((unsigned)ceil_div(count, 256)), dim3(256), 0, M.stream, (const int32_t *)g->rr[0].res_q.p + offset,
                       (const int32_t *)g->rr[0].res_c.p + offset, d_query, d_store, count, g->ext.q.p, g->ext.c.p);
    GHIP(nullptr, M, hipGetLastError());
    GHIP(nullptr, M, hipMemcpyAsync(out_q, g->ext.q.p, (size_t)count * sizeof(int64_t), hipMemcpyDeviceToHost, M.stream));
    GHIP(nullptr, M, hipMemcpyAsync(out_c, g->ext.c.p, (size_t)count * sizeof(int64_t), hipMemcpyDeviceToHost, M.stream));
    GHIP(nullptr, M, hipMemcpyAsync(out_score, g->rr[0].res_s.p + offset, (size_t)count * sizeof(float), hipMemcpyDeviceToHost, M.stream));
    GHIP(nullptr, M, hipStreamSynchronize(M.stream));
    return APSS_OK;
  };
  const int32_t rc = body();
  if (rc != APSS_OK) g->err = M.err;
  return rc;
}

int32_t apss_group_set_top_k(apss_group *g, int32_t k) {
  if (!g) return APSS_E_INVALID;
  // (a refusal is also left where apss_group_last_error(NULL) finds it: a wrapper that applies k right after the create and
  // destroys the group when it is refused reports it as a failed create)
  if (k < 0 || k > APSS_TOP_K_MAX) return gfail(g, APSS_E_INVALID, g_group_create_error = "apss_group_set_top_k: k must be in [0, 1024] (0: off)");
  if (k > 0 && g->D > 1)
    return gfail(g, APSS_E_UNSUPPORTED, g_group_create_error = "apss_group_set_top_k: a grid keeps its results as triples per row range on different "
                                                               "devices; per-query top-k is not available with more than one row range");
  if (g->created && topk_in_handle(g)) {
    const int32_t rc = apss_set_top_k(g->m[0].h, k);
    if (rc != APSS_OK) return gfail(g, rc, apss_last_error(g->m[0].h));
  }
  g->top_k = k;
  return APSS_OK;
}

int32_t apss_group_topk_get(apss_group *g, apss_topk_info *out) {
  if (!g || !out) return APSS_E_INVALID;
  const int32_t caller = out->struct_size;
  if (caller < (int32_t)(2 * sizeof(int32_t)) || caller > (1 << 16))
    return gfail(g, APSS_E_INVALID, "apss_topk_info.struct_size must be set to sizeof(apss_topk_info) before the call");
  if (g->results_in_handle) {
    const int32_t rc = apss_topk_get(g->m[0].h, out);
    if (rc != APSS_OK) g->err = apss_last_error(g->m[0].h);
    return rc;
  }
  apss_topk_info t = g->tk;
  if (g->D > 1 || g->n_res < 0) t = apss_topk_info{};
  if (g->D > 1 && g->n_res >= 0) t.pairs_over_theta = t.kept = g->n_res;
  const int32_t n = std::min<int32_t>(caller, (int32_t)sizeof(apss_topk_info));
  t.struct_size = n;
  std::memcpy(out, &t, (size_t)n);
  return APSS_OK;
}

int32_t apss_group_stats_get(apss_group *g, apss_group_stats *out) {
  if (!g || !out) return APSS_E_INVALID;
  const int32_t caller = out->struct_size;
  if (caller < (int32_t)(2 * sizeof(int32_t)) || caller > (1 << 16))
    return gfail(g, APSS_E_INVALID, "apss_group_stats.struct_size must be set to sizeof(apss_group_stats) before the call");
  const int32_t n = std::min<int32_t>(caller, (int32_t)sizeof(apss_group_stats));
  g->st.n_members = g->T * g->D;
  g->st.struct_size = n;
  std::memcpy(out, &g->st, (size_t)n);
  return APSS_OK;
}

int32_t apss_group_grid_get(apss_group *g, apss_group_grid *out) {
  if (!g || !out) return APSS_E_INVALID;
  const int32_t caller = out->struct_size;
  if (caller < (int32_t)(2 * sizeof(int32_t)) || caller > (1 << 16))
    return gfail(g, APSS_E_INVALID, "apss_group_grid.struct_size must be set to sizeof(apss_group_grid) before the call");
  apss_group_grid G{};
  G.n_term_ranges = g->T;
  G.n_row_ranges = g->D;
  G.symmetric_ranges = g->symmetric_ranges ? 1 : 0;
  for (int j = 0; j < g->D; ++j) {
    const apss_group::Range &R = g->rr[(size_t)j];
    G.rows_in_range[j] = R.rows;
    G.outside_rows_max = std::max(G.outside_rows_max, R.outside_rows);
    G.mirrored_pairs += R.mirrored;
    G.own_ms_max = std::max(G.own_ms_max, R.own_ms);
    G.outside_ms_max = std::max(G.outside_ms_max, R.outside_ms);
  }
  const int32_t n = std::min<int32_t>(caller, (int32_t)sizeof(apss_group_grid));
  G.struct_size = n;
  std::memcpy(out, &G, (size_t)n);
  return APSS_OK;
}

int32_t apss_group_member_stats(apss_group *g, int32_t member, apss_stats *out) {
  if (!g || !out) return APSS_E_INVALID;
  if (member < 0 || member >= g->T * g->D) return gfail(g, APSS_E_INVALID, "no such member");
  if (!g->m[(size_t)member].h) return gfail(g, APSS_E_STATE, "the members are created by the group's first insert");
  const int32_t rc = apss_stats_get(g->m[(size_t)member].h, out);
  if (rc != APSS_OK) g->err = apss_last_error(g->m[(size_t)member].h);
  return rc;
}

}  // extern "C"
