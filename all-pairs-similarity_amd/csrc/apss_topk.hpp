// apss_topk.hpp -- per-query top-k over the final list of a query-type call (include/apss.h: apss_set_top_k).
//
// In: the call's final list (query row of the batch, candidate slot, fp32 score), n pairs in no particular order, and the
// store's external ids.  Out: for every query row its first k pairs in the order (score descending, candidate external id
// ascending, candidate slot ascending; -0.0f counts as +0.0f), grouped by query row ascending, in rank order inside a row.
//
// Four launches, all on the caller's stream:
//   k_topk_count    pairs per query row.  The list is not grouped, so a workgroup aggregates its 1024 entries in an LDS hash
//                   table keyed by query row and adds once per distinct row to the global counters.
//   k_topk_scan     one workgroup: exclusive scans of count (segment starts) and of min(count, k) (output starts), the kept
//                   total, the rows cut and the longest segment; resets the counters, which become the scatter's cursors.
//                   (A probe that cut its rounds -- apss_set_top_k_tile_cut -- hands in the rows' UNCUT counts as a second input:
//                   the rows cut and the longest segment are then theirs, what the call found and not what the probe emitted.)
//   k_topk_scatter  (candidate slot, score) of every pair into its row's segment; the same LDS table hands out a workgroup's
//                   places in a segment with one global atomic per distinct row.
//   k_topk_select   one workgroup per query row.  A segment of up to 1024 pairs is sorted whole in LDS.  A longer one is cut
//                   by radix select over the 128-bit key (score key, external id, slot), 8 bits per pass with an LDS
//                   histogram, streaming the segment from global memory per pass and stopping at the first digit that
//                   separates the k-th pair from the (k+1)-th (external ids are gathered only for pairs that tie the score
//                   of the boundary); the k kept pairs are collected in LDS and sorted there.
// This header is included by both translation units (the handle's pass, the group's pass behind its exchange): everything
// lives in an unnamed namespace.
#ifndef APSS_TOPK_HPP
#define APSS_TOPK_HPP

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/apss.h"
#include "apss_stage.hpp"
#include "apss_topk_key.hpp"

namespace apss {
namespace {

constexpr int kTopkThreads = 256;
constexpr int kTopkItems = 4;                          // list entries per thread of k_topk_count / k_topk_scatter (one 16-B load)
constexpr int kTopkBlock = kTopkThreads * kTopkItems;  // entries per workgroup
constexpr int kTopkSlots = 2 * kTopkBlock;             // LDS hash slots: never more than half full
constexpr int kTopkSort = APSS_TOP_K_MAX;              // pairs sorted in LDS by one workgroup of k_topk_select
constexpr int kTopkScanThreads = 1024;
constexpr int kTopkLaunches = 4;
enum { kTopkKept = 0, kTopkCut = 1, kTopkLongest = 2, kTopkTotal = 3, kTopkInfoWords = 4 };

static_assert((kTopkSort & (kTopkSort - 1)) == 0, "the LDS sort wants a power of two");

__device__ inline int topk_slot_of(int32_t q, int32_t *keys) {
  unsigned s = ((unsigned)q * 2654435761u) >> 21;  // 11 bits: kTopkSlots
  static_assert(kTopkSlots == 2048, "hash width");
  for (;;) {
    const int32_t old = atomicCAS(&keys[s], -1, q);
    if (old == -1 || old == q) return (int)s;
    s = (s + 1) & (kTopkSlots - 1);
  }
}

// the thread's (up to) four consecutive entries; rows outside [0, nq) (there are none in a valid list) become -1
__device__ inline void topk_load_rows(const int32_t *__restrict__ q, int64_t i0, int64_t n, int32_t nq, int32_t (&r)[kTopkItems]) {
  if (i0 + kTopkItems <= n) {
    const int4 v = *reinterpret_cast<const int4 *>(q + i0);
    r[0] = v.x;
    r[1] = v.y;
    r[2] = v.z;
    r[3] = v.w;
  } else {
    for (int j = 0; j < kTopkItems; ++j) r[j] = i0 + j < n ? q[i0 + j] : -1;
  }
  for (int j = 0; j < kTopkItems; ++j)
    if (r[j] < 0 || r[j] >= nq) r[j] = -1;
}

__global__ __launch_bounds__(kTopkThreads) void k_topk_count(const int32_t *__restrict__ q, int64_t n, int32_t nq,
                                                             unsigned int *__restrict__ cnt) {
  __shared__ int32_t keys[kTopkSlots];
  __shared__ unsigned int vals[kTopkSlots];
  for (int s = threadIdx.x; s < kTopkSlots; s += kTopkThreads) {
    keys[s] = -1;
    vals[s] = 0u;
  }
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * kTopkBlock + (int64_t)threadIdx.x * kTopkItems;
  if (i0 < n) {
    int32_t r[kTopkItems];
    topk_load_rows(q, i0, n, nq, r);
    for (int j = 0; j < kTopkItems;) {  // neighbours of one row go in as one add
      int e = j + 1;
      while (e < kTopkItems && r[e] == r[j]) ++e;
      if (r[j] >= 0) atomicAdd(&vals[topk_slot_of(r[j], keys)], (unsigned)(e - j));
      j = e;
    }
  }
  __syncthreads();
  for (int s = threadIdx.x; s < kTopkSlots; s += kTopkThreads)
    if (keys[s] >= 0) atomicAdd(&cnt[keys[s]], vals[s]);
}

// cnt[nq] -> seg_start[nq + 1], out_start[nq + 1], info[kTopkInfoWords]; cnt is zeroed (the scatter's cursors)
// uncut (or null): the rows' counts before a cut inside the probe; min(count, k) is the same for both
__global__ __launch_bounds__(kTopkScanThreads) void k_topk_scan(unsigned int *__restrict__ cnt, int32_t nq, int32_t k,
                                                                int64_t *__restrict__ seg_start, int64_t *__restrict__ out_start,
                                                                unsigned long long *__restrict__ info,
                                                                const unsigned int *__restrict__ uncut) {
  __shared__ unsigned long long sa[kTopkScanThreads], sb[kTopkScanThreads];
  __shared__ unsigned int s_cut, s_long;
  const int t = threadIdx.x;
  if (t == 0) s_cut = s_long = 0u;
  const int64_t per = ((int64_t)nq + kTopkScanThreads - 1) / kTopkScanThreads;
  const int64_t lo = std::min<int64_t>((int64_t)t * per, nq), hi = std::min<int64_t>(lo + per, nq);
  unsigned long long a = 0, b = 0;
  unsigned int cut = 0, longest = 0;
  for (int64_t i = lo; i < hi; ++i) {
    const unsigned int c = cnt[i];
    a += c;
    b += c < (unsigned)k ? c : (unsigned)k;
    const unsigned int u = uncut ? uncut[i] : c;
    cut += u > (unsigned)k ? 1u : 0u;
    longest = u > longest ? u : longest;
  }
  sa[t] = a;
  sb[t] = b;
  __syncthreads();
  for (int off = 1; off < kTopkScanThreads; off <<= 1) {
    const unsigned long long ua = t >= off ? sa[t - off] : 0ull, ub = t >= off ? sb[t - off] : 0ull;
    __syncthreads();
    sa[t] += ua;
    sb[t] += ub;
    __syncthreads();
  }
  if (cut) atomicAdd(&s_cut, cut);
  if (longest) atomicMax(&s_long, longest);
  unsigned long long ea = sa[t] - a, eb = sb[t] - b;
  for (int64_t i = lo; i < hi; ++i) {
    const unsigned int c = cnt[i];
    seg_start[i] = (int64_t)ea;
    out_start[i] = (int64_t)eb;
    ea += c;
    eb += c < (unsigned)k ? c : (unsigned)k;
    cnt[i] = 0u;
  }
  __syncthreads();
  if (t == kTopkScanThreads - 1) {
    seg_start[nq] = (int64_t)sa[t];
    out_start[nq] = (int64_t)sb[t];
    info[kTopkKept] = sb[t];
    info[kTopkCut] = s_cut;
    info[kTopkLongest] = s_long;
    info[kTopkTotal] = sa[t];
  }
}

__global__ __launch_bounds__(kTopkThreads) void k_topk_scatter(const int32_t *__restrict__ q, const int32_t *__restrict__ c,
                                                               const float *__restrict__ s, int64_t n, int32_t nq,
                                                               const int64_t *__restrict__ seg_start, unsigned int *__restrict__ cursor,
                                                               int32_t *__restrict__ seg_c, float *__restrict__ seg_s) {
  __shared__ int32_t keys[kTopkSlots];
  __shared__ unsigned int vals[kTopkSlots];
  __shared__ unsigned int base[kTopkSlots];
  for (int i = threadIdx.x; i < kTopkSlots; i += kTopkThreads) {
    keys[i] = -1;
    vals[i] = 0u;
  }
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * kTopkBlock + (int64_t)threadIdx.x * kTopkItems;
  int32_t r[kTopkItems];
  int slot[kTopkItems];
  unsigned int rank[kTopkItems];
  for (int j = 0; j < kTopkItems; ++j) r[j] = -1;
  if (i0 < n) {
    topk_load_rows(q, i0, n, nq, r);
    for (int j = 0; j < kTopkItems;) {
      int e = j + 1;
      while (e < kTopkItems && r[e] == r[j]) ++e;
      if (r[j] >= 0) {
        const int sl = topk_slot_of(r[j], keys);
        const unsigned int first = atomicAdd(&vals[sl], (unsigned)(e - j));
        for (int u = j; u < e; ++u) {
          slot[u] = sl;
          rank[u] = first + (unsigned)(u - j);
        }
      }
      j = e;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kTopkSlots; i += kTopkThreads)
    if (keys[i] >= 0) base[i] = atomicAdd(&cursor[keys[i]], vals[i]);
  __syncthreads();
  for (int j = 0; j < kTopkItems; ++j) {
    if (r[j] < 0) continue;
    const int64_t pos = seg_start[r[j]] + (int64_t)base[slot[j]] + (int64_t)rank[j];
    if (pos >= seg_start[r[j] + 1]) continue;  // (cannot happen: the count pass read the same list)
    seg_c[pos] = c[i0 + j];
    seg_s[pos] = s[i0 + j];
  }
}

// the 128-bit sort key of a pair, ascending = rank order: (inverted score key, external id, slot)
struct TopkKey {
  unsigned long long hi, lo;
};
__device__ inline unsigned long long topk_ext_bits(const int64_t *__restrict__ c_ext, int32_t c, int64_t n_store) {
  const int64_t e = (c >= 0 && c < n_store) ? c_ext[c] : 0;
  return (unsigned long long)e ^ 0x8000000000000000ull;  // signed order as unsigned
}
__device__ inline TopkKey topk_make_key(uint32_t ik, unsigned long long e, int32_t c) {
  TopkKey k;
  k.hi = ((unsigned long long)ik << 32) | (e >> 32);
  k.lo = (e << 32) | (unsigned long long)(uint32_t)c;
  return k;
}
__device__ inline bool topk_less(unsigned long long ahi, unsigned long long alo, unsigned long long bhi, unsigned long long blo) {
  return ahi < bhi || (ahi == bhi && alo < blo);
}

// one add per wave when every matching lane of the wave holds the same digit (the leading digits of scores in [theta, 1])
__device__ inline void topk_hist_add(unsigned int *hist, bool match, uint32_t dig) {
  const unsigned long long m = __ballot(match);
  if (m == 0ull) return;
  const int leader = __ffsll((long long)m) - 1;
  const uint32_t first = (uint32_t)__shfl((int)dig, leader);
  if (__all(!match || dig == first)) {
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[first], (unsigned)__popcll(m));
  } else if (match) {
    atomicAdd(&hist[dig], 1u);
  }
}

__global__ __launch_bounds__(kTopkThreads) void k_topk_select(const int64_t *__restrict__ seg_start, const int64_t *__restrict__ out_start,
                                                              const int32_t *__restrict__ seg_c, const float *__restrict__ seg_s,
                                                              const int64_t *__restrict__ c_ext, int64_t n_store, int32_t k,
                                                              int32_t *__restrict__ out_q, int32_t *__restrict__ out_c,
                                                              float *__restrict__ out_s) {
  __shared__ unsigned long long khi[kTopkSort], klo[kTopkSort];
  __shared__ unsigned int hist[256];
  __shared__ unsigned int wsum[kTopkThreads / 64];
  __shared__ unsigned int sel_digit, sel_less, sel_count, n_kept, n_tied;
  const int32_t q = (int32_t)blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t base = seg_start[q];
  const int64_t n = seg_start[q + 1] - base;
  if (n <= 0) return;
  int m;  // pairs in LDS
  if (n <= kTopkSort) {
    m = (int)n;
    for (int i = tid; i < m; i += kTopkThreads) {
      const int32_t c = seg_c[base + i];
      const TopkKey key = topk_make_key(~topk_key(seg_s[base + i]), topk_ext_bits(c_ext, c, n_store), c);
      khi[i] = key.hi;
      klo[i] = key.lo;
    }
  } else {
    // ---- radix select: the k smallest keys of n > kTopkSort >= k.  T = the digits found so far (of the k-th smallest key)
    uint32_t t_ik = 0u, t_c = 0u;
    unsigned long long t_e = 0ull;
    unsigned int remaining = (unsigned)k;  // how many of the pairs matching T's digits are wanted
    int digits = 0;
    for (int d = 0; d < 16; ++d) {
      hist[tid] = 0u;
      __syncthreads();
      for (int64_t j0 = 0; j0 < n; j0 += kTopkThreads) {
        const int64_t j = j0 + tid;
        bool match = false;
        uint32_t dig = 0u;
        if (j < n) {
          const uint32_t ik = ~topk_key(seg_s[base + j]);
          if (d < 4) {
            const int sh = 24 - 8 * d;
            match = d == 0 || (ik >> (sh + 8)) == (t_ik >> (sh + 8));
            dig = (ik >> sh) & 255u;
          } else if (ik == t_ik) {
            const int32_t c = seg_c[base + j];
            const unsigned long long e = topk_ext_bits(c_ext, c, n_store);
            if (d < 12) {
              const int sh = 56 - 8 * (d - 4);
              match = d == 4 || (e >> (sh + 8)) == (t_e >> (sh + 8));
              dig = (uint32_t)(e >> sh) & 255u;
            } else {
              const int sh = 24 - 8 * (d - 12);
              match = e == t_e && (d == 12 || ((uint32_t)c >> (sh + 8)) == (t_c >> (sh + 8)));
              dig = ((uint32_t)c >> sh) & 255u;
            }
          }
        }
        topk_hist_add(hist, match, dig);
      }
      __syncthreads();
      // inclusive scan of the 256 buckets: in each wave by shuffles, then across the four waves
      const unsigned int mine = hist[tid];
      unsigned int inc = mine;
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned int up = (unsigned)__shfl_up((int)inc, off);
        if ((tid & 63) >= off) inc += up;
      }
      if ((tid & 63) == 63) wsum[tid >> 6] = inc;
      __syncthreads();
      for (int w = 0; w < (tid >> 6); ++w) inc += wsum[w];
      if (inc >= remaining && inc - mine < remaining) {  // exactly one bucket holds the pair of rank `remaining`
        sel_digit = (unsigned)tid;
        sel_less = inc - mine;
        sel_count = mine;
      }
      __syncthreads();
      const uint32_t dg = sel_digit;
      remaining -= sel_less;
      if (d < 4) t_ik |= dg << (24 - 8 * d);
      else if (d < 12) t_e |= (unsigned long long)dg << (56 - 8 * (d - 4));
      else t_c |= dg << (24 - 8 * (d - 12));
      digits = d + 1;
      const unsigned int in_bucket = sel_count;
      __syncthreads();  // (sel_* and hist are rewritten by the next pass)
      if (in_bucket == remaining) break;  // every pair that matches T so far is kept: no further digit is needed
    }
    // ---- collect: pairs whose first `digits` digits are below T's, and `remaining` of those that equal them
    if (tid == 0) n_kept = n_tied = 0u;
    __syncthreads();
    for (int64_t j = tid; j < n; j += kTopkThreads) {
      const uint32_t ik = ~topk_key(seg_s[base + j]);
      bool less = false, eq = false, have = false;
      int32_t c = 0;
      unsigned long long e = 0ull;
      if (digits <= 4) {
        const int sh = 32 - 8 * digits;
        less = (ik >> sh) < (t_ik >> sh);
        eq = (ik >> sh) == (t_ik >> sh);
      } else if (ik < t_ik) {
        less = true;
      } else if (ik == t_ik) {
        c = seg_c[base + j];
        e = topk_ext_bits(c_ext, c, n_store);
        have = true;
        if (digits <= 12) {
          const int sh = 64 - 8 * (digits - 4);
          less = (e >> sh) < (t_e >> sh);
          eq = (e >> sh) == (t_e >> sh);
        } else if (e < t_e) {
          less = true;
        } else if (e == t_e) {
          const int sh = 32 - 8 * (digits - 12);
          less = ((uint32_t)c >> sh) < (t_c >> sh);
          eq = ((uint32_t)c >> sh) == (t_c >> sh);
        }
      }
      if (!less && !(eq && atomicAdd(&n_tied, 1u) < remaining)) continue;
      const unsigned int pos = atomicAdd(&n_kept, 1u);
      if (pos >= (unsigned)kTopkSort) continue;  // (cannot happen: exactly k are kept)
      if (!have) {
        c = seg_c[base + j];
        e = topk_ext_bits(c_ext, c, n_store);
      }
      const TopkKey key = topk_make_key(ik, e, c);
      khi[pos] = key.hi;
      klo[pos] = key.lo;
    }
    __syncthreads();
    m = (int)std::min<unsigned int>(n_kept, (unsigned)kTopkSort);
  }
  // ---- rank order: bitonic sort of the m pairs, padded to a power of two with keys that sort last
  int p = 2;
  while (p < m) p <<= 1;
  for (int i = m + tid; i < p; i += kTopkThreads) khi[i] = klo[i] = ~0ull;
  __syncthreads();
  for (int kk = 2; kk <= p; kk <<= 1) {
    for (int jj = kk >> 1; jj > 0; jj >>= 1) {
      for (int i = tid; i < p; i += kTopkThreads) {
        const int o = i ^ jj;
        if (o > i) {
          const unsigned long long ahi = khi[i], alo = klo[i], bhi = khi[o], blo = klo[o];
          const bool up = (i & kk) == 0;
          if (topk_less(bhi, blo, ahi, alo) == up) {
            khi[i] = bhi;
            klo[i] = blo;
            khi[o] = ahi;
            klo[o] = alo;
          }
        }
      }
      __syncthreads();
    }
  }
  const int keep = m < k ? m : k;
  const int64_t ob = out_start[q];
  for (int i = tid; i < keep; i += kTopkThreads) {
    out_q[ob + i] = q;
    out_c[ob + i] = (int32_t)(uint32_t)klo[i];
    out_s[ob + i] = topk_key_inv(~(uint32_t)(khi[i] >> 32));
  }
}

// ---- host side: the pass's buffers (owned by a handle, or by a group for the list behind its exchange) and its launches
struct TopkWork {
  DevBuf<unsigned int> cnt;
  DevBuf<int64_t> seg_start, out_start;
  DevBuf<unsigned long long> info;
  DevBuf<int32_t> seg_c, out_q, out_c;
  DevBuf<float> seg_s, out_s;
  StageMem mem;
};

// Runs the pass over (q, c, s)[0, n) on `stream` and waits for it (the one host read: the four info words).  The new list is
// w.out_*[0, info->kept).  n == 0: nothing is launched.  info: k, pairs_over_theta, kept, queries_cut, longest_segment,
// select_ms, select_launches are filled.  uncut (or null) / uncut_total: the rows' pair counts and their sum before a cut inside the
// probe thinned the list; pairs_over_theta, queries_cut and longest_segment then speak of those (k_topk_scan's second input: the
// launches stay four).
inline hipError_t topk_run(TopkWork &w, hipStream_t stream, const int32_t *q, const int32_t *c, const float *s, int64_t n, int64_t nq,
                           const int64_t *c_ext, int64_t n_store, int32_t k, apss_topk_info *info, const unsigned int *uncut = nullptr,
                           int64_t uncut_total = 0) {
  info->k = k;
  info->pairs_over_theta = uncut ? uncut_total : n;
  info->kept = info->queries_cut = info->longest_segment = 0;
  info->select_ms = 0.0;
  info->select_launches = 0;
  if (n <= 0 || nq <= 0) return hipSuccess;
  hipError_t e;
  if (!w.info.p && (e = w.mem.grow((size_t)kTopkInfoWords, w.info)) != hipSuccess) return e;
  // (arrays that grow together share a capacity; the one grown last says whether all of them have it)
  if ((size_t)nq + 1 > w.out_start.cap) {
    const size_t cap = std::max<size_t>((size_t)nq + 1, w.out_start.cap + w.out_start.cap / 2);
    if ((e = w.mem.grow(cap, w.cnt, w.seg_start, w.out_start)) != hipSuccess) return e;
  }
  if ((size_t)n > w.seg_s.cap && (e = w.mem.grow((size_t)n + (size_t)n / 8 + 1024, w.seg_c, w.seg_s)) != hipSuccess) return e;
  const size_t out_need = (size_t)std::min<int64_t>(n, nq * (int64_t)k);
  if (out_need > w.out_s.cap && (e = w.mem.grow(out_need + out_need / 8 + 1024, w.out_q, w.out_c, w.out_s)) != hipSuccess) return e;
  const unsigned blocks = (unsigned)((n + kTopkBlock - 1) / kTopkBlock);
  if ((e = hipMemsetAsync(w.cnt.p, 0, ((size_t)nq + 1) * sizeof(unsigned int), stream)) != hipSuccess) return e;
  if ((e = begin_timed(stream, w.mem.e0)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_topk_count, dim3(blocks), dim3(kTopkThreads), 0, stream, q, n, (int32_t)nq, w.cnt.p);
  hipLaunchKernelGGL(k_topk_scan, dim3(1), dim3(kTopkScanThreads), 0, stream, w.cnt.p, (int32_t)nq, k, w.seg_start.p, w.out_start.p, w.info.p,
                     uncut);
  hipLaunchKernelGGL(k_topk_scatter, dim3(blocks), dim3(kTopkThreads), 0, stream, q, c, s, n, (int32_t)nq,
                     (const int64_t *)w.seg_start.p, w.cnt.p, w.seg_c.p, w.seg_s.p);
  hipLaunchKernelGGL(k_topk_select, dim3((unsigned)nq), dim3(kTopkThreads), 0, stream, (const int64_t *)w.seg_start.p,
                     (const int64_t *)w.out_start.p, (const int32_t *)w.seg_c.p, (const float *)w.seg_s.p, c_ext, n_store, k, w.out_q.p, w.out_c.p,
                     w.out_s.p);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  unsigned long long words[kTopkInfoWords] = {0, 0, 0, 0};
  float ms = 0.f;
  if ((e = end_timed_read(stream, w.mem.e0, w.mem.e1, {{words, w.info.p, sizeof(words)}}, &ms)) != hipSuccess) return e;
  info->kept = (int64_t)words[kTopkKept];
  info->queries_cut = (int64_t)words[kTopkCut];
  info->longest_segment = (int64_t)words[kTopkLongest];
  info->select_ms = ms;
  info->select_launches = kTopkLaunches;
  return hipSuccess;
}

}  // namespace
}  // namespace apss

#endif  // APSS_TOPK_HPP
