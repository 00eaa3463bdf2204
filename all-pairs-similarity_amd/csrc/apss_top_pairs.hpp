// apss_top_pairs.hpp -- the GLOBAL top-K over the final list of a query-type call (include/apss.h: apss_set_top_pairs).
//
// In: the call's final list (query row of the batch, candidate slot, fp32 score), n pairs in no particular order, the batch's and
// the store's external ids.  Out: the first min(K, n) pairs of the list in the total order (score descending with -0.0f as +0.0f,
// query external id, candidate external id, query row, candidate slot -- all ascending), in rank order.
//
// The list is read where it lies; nothing of its length is written but, at worst, one 32-bit index per pair that TIES the K-th score.
//   k_tp_hist         radix select over the 32-bit inverted score key, 8 bits per pass, four passes: a workgroup keeps one LDS
//                     histogram over its grid-stride share of the scores (16-B loads, one LDS add per wave where a wave's matching
//                     lanes share a digit -- tp_hist_add) and adds each non-empty bin once to the pass's global histogram.
//   k_tp_pick         one workgroup: scans a 256-bin histogram, finds the bin of the wanted rank, extends the prefix and lowers the
//                     remaining rank IN DEVICE MEMORY (no host read between passes).  After the fourth pass: the threshold key T,
//                     G = pairs above it (< K), E = pairs that share it.
//   k_tp_collect      one pass over the scores: the index of every pair above T into the selection, of every pair AT T into the tie
//                     list (or into the selection too, when all E are kept); a wave takes its places in the workgroup's LDS stage
//                     with ballots and one LDS add, the workgroup its places in the output with one global add per stage.
//   k_tp_tie_hist     radix select of the K - G first ties by (query id, candidate id, query row, slot): the same passes over the
//   (+ k_tp_pick)     tie list, ids gathered for tied pairs only; the passes stop counting once a digit separates.
//   k_tp_tie_collect  the kept ties' indices behind the G in the selection.
//   k_tp_keys         rank order of the min(K, n) selected pairs: four stable rocprim radix sorts, least significant field
//   k_tp_write        first ((row, slot); candidate id; query id; score key), each over keys gathered through the permutation
//                     so far; then the pairs are written out in that order.
// Two host waits: one reads (G, E) and sizes the tie list, one ends the stage.  n <= K goes straight to the rank order.
#ifndef APSS_TOP_PAIRS_HPP
#define APSS_TOP_PAIRS_HPP

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/apss.h"
#include "apss_stage.hpp"
#include "apss_topk.hpp"
#include "apss_topk_key.hpp"

namespace apss {
namespace {

constexpr int kTpThreads = 256;
constexpr int kTpWave = 64;
constexpr int kTpItems = 4;                        // scores per lane and trip (one 16-B load)
constexpr int kTpBlock = kTpThreads * kTpItems;    // list entries per workgroup and trip
constexpr int kTpBins = 256;                       // 8-bit digits
constexpr int kTpScorePasses = 4;
constexpr int kTpTieDigitsMax = 24;                // 64 + 64 + 64 bits of (query id, candidate id, row and slot)
constexpr int64_t kTpGridCap = 2048;               // workgroups of the grid-stride kernels (APSS_DEBUG=tp_grid=N: N)
constexpr int64_t kTpTrips = 4;                    // ... and a workgroup of the passes over the list takes this many trips before there
                                                   // are more of them: every workgroup ends in adds to a few hot words (the leading
                                                   // digit's bins, the cursors), which answer about 90 adds a microsecond
// the stage's words in device memory
enum {
  kTpT = 0,          // the inverted score key of the K-th pair, digit by digit
  kTpTie0 = 1,       // [3] the tie key of the last kept tie, digit by digit
  kTpRemaining = 4,  // the wanted rank among the pairs that match the digits so far (1-based)
  kTpDone = 5,       // tie passes: a digit separated, every pair matching the digits so far is kept
  kTpDigits = 6,     // tie digits found
  kTpAbove = 7,      // G
  kTpTied = 8,       // E
  kTpSelCursor = 9,
  kTpTieCursor = 10,
  kTpTieTaken = 11,  // ties equal to the whole tie prefix that took a place
  kTpWords = 16
};

__device__ inline void tp_load_scores(const float *__restrict__ s, int64_t i0, int64_t n, bool wide, float (&v)[kTpItems]) {
  if (wide && i0 + kTpItems <= n) {
    const float4 f = *reinterpret_cast<const float4 *>(s + i0);
    v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
  } else {
    for (int j = 0; j < kTpItems; ++j) v[j] = i0 + j < n ? s[i0 + j] : 0.f;
  }
}

// One LDS add per distinct digit of the wave, for its first kTpAddRounds digits (topk_hist_add's idea, carried past the case of
// ONE digit: at theta = 0 a wave's leading digits are two or three exponents, and 64 lanes on three LDS words serialise); lanes
// whose digit is still waiting after that add for themselves.
constexpr int kTpAddRounds = 4;
__device__ inline void tp_hist_add(unsigned int *hist, bool match, uint32_t dig) {
  unsigned long long m = __ballot(match);
  for (int r = 0; r < kTpAddRounds && m != 0ull; ++r) {  // (m is the same in every lane)
    const int leader = __ffsll((long long)m) - 1;
    const uint32_t d = (uint32_t)__shfl((int)dig, leader);
    const unsigned long long same = __ballot(match && dig == d);
    if ((int)(threadIdx.x % kTpWave) == leader) atomicAdd(&hist[d], (unsigned)__popcll(same));
    if (dig == d) match = false;
    m &= ~same;
  }
  if (match) atomicAdd(&hist[dig], 1u);
}

// pass p of the score select: the digit `24 - 8p` of the inverted key, over the pairs that match the prefix found so far
__global__ __launch_bounds__(kTpThreads) void k_tp_hist(const float *__restrict__ s, int64_t n, const unsigned long long *__restrict__ state,
                                                        int pass, unsigned long long *__restrict__ ghist) {
  __shared__ unsigned int hist[kTpBins];
  hist[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t prefix = (uint32_t)state[kTpT];
  const int sh = 24 - 8 * pass;
  const bool wide = (reinterpret_cast<uintptr_t>(s) & 15u) == 0;
  for (int64_t base = (int64_t)blockIdx.x * kTpBlock; base < n; base += (int64_t)gridDim.x * kTpBlock) {  // (block-uniform: ballots inside)
    const int64_t i0 = base + (int64_t)threadIdx.x * kTpItems;
    float v[kTpItems];
    tp_load_scores(s, i0, n, wide, v);
    for (int j = 0; j < kTpItems; ++j) {
      const uint32_t ik = ~topk_key(v[j]);
      const bool match = i0 + j < n && (pass == 0 || (ik >> (sh + 8)) == (prefix >> (sh + 8)));
      tp_hist_add(hist, match, (ik >> sh) & 255u);
    }
  }
  __syncthreads();
  const unsigned int mine = hist[threadIdx.x];
  if (mine) atomicAdd(&ghist[threadIdx.x], (unsigned long long)mine);
}

// One workgroup.  word / shift: where the digit goes (state[word] |= digit << shift).  last_score: the fourth score pass (leaves G
// and E, k = K).  tie: a tie pass (honours and sets kTpDone, counts kTpDigits).
__global__ __launch_bounds__(kTpBins) void k_tp_pick(const unsigned long long *__restrict__ ghist, unsigned long long *__restrict__ state,
                                                     int word, int shift, int last_score, int tie, unsigned long long k) {
  __shared__ unsigned long long sc[kTpBins];
  const int t = threadIdx.x;
  if (tie && state[kTpDone]) return;  // (read by every thread before anyone writes: the one write is behind the barriers below)
  const unsigned long long remaining = state[kTpRemaining];
  const unsigned long long mine = ghist[t];
  sc[t] = mine;
  __syncthreads();
  for (int off = 1; off < kTpBins; off <<= 1) {
    const unsigned long long up = t >= off ? sc[t - off] : 0ull;
    __syncthreads();
    sc[t] += up;
    __syncthreads();
  }
  const unsigned long long inc = sc[t];
  if (inc >= remaining && inc - mine < remaining) {  // exactly one bin holds the pair of rank `remaining`
    const unsigned long long left = remaining - (inc - mine);
    state[word] |= (unsigned long long)t << shift;
    state[kTpRemaining] = left;
    if (last_score) {
      state[kTpAbove] = k - left;
      state[kTpTied] = mine;
    }
    if (tie) {
      state[kTpDigits] += 1ull;
      if (mine == left) state[kTpDone] = 1ull;
    }
  }
}

// k_tp_collect stages what a workgroup selects in LDS and takes its places behind a global cursor once per kTpStage - kTpBlock
// indices or more (with K << n: once, at its end).  One cursor word answers about 90 returning adds a microsecond: a wave's add per
// trip, ten thousand of them on a list of 2.7 M pairs, was the whole kernel's time.
constexpr int kTpStage = 2 * kTpBlock;

// a wave's places in a stage: votes[j] = the lanes whose item j goes in; returns the first place (every lane), 0 if none go
__device__ inline unsigned int tp_wave_places(unsigned int *fill, const unsigned long long (&votes)[kTpItems], int lane) {
  int total = 0;
  for (int j = 0; j < kTpItems; ++j) total += __popcll(votes[j]);
  if (total == 0) return 0u;  // (wave-uniform)
  unsigned int at = 0u;
  if (lane == 0) at = atomicAdd(fill, (unsigned)total);
  return (unsigned)__shfl((int)at, 0);
}

// stage[0, *fill) -> out[cursor ...) (out[cap]); every thread of the workgroup calls it
__device__ inline void tp_flush(const uint32_t *stage, unsigned int *fill, unsigned long long *base, unsigned long long *cursor,
                                uint32_t *__restrict__ out, unsigned long long cap) {
  const unsigned int n = *fill;
  if (threadIdx.x == 0 && n) *base = atomicAdd(cursor, (unsigned long long)n);
  __syncthreads();
  for (unsigned int i = threadIdx.x; i < n; i += kTpThreads) {
    const unsigned long long o = *base + i;
    if (o < cap) out[o] = stage[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) *fill = 0u;
  __syncthreads();
}

// sel[sel_cap] <- indices of the pairs above T (and, ties_all, at T); tie[tie_cap] <- indices of the pairs at T (unless ties_all)
__global__ __launch_bounds__(kTpThreads) void k_tp_collect(const float *__restrict__ s, int64_t n, unsigned long long *__restrict__ state,
                                                           uint32_t *__restrict__ sel, unsigned long long sel_cap, uint32_t *__restrict__ tie,
                                                           unsigned long long tie_cap, int ties_all) {
  __shared__ uint32_t stage[2][kTpStage];
  __shared__ unsigned int fill[2];
  __shared__ unsigned long long base[2];
  if (threadIdx.x < 2) fill[threadIdx.x] = 0u;
  const uint32_t T = (uint32_t)state[kTpT];
  const int lane = threadIdx.x % kTpWave;
  const unsigned long long below = (1ull << lane) - 1ull;
  const bool wide = (reinterpret_cast<uintptr_t>(s) & 15u) == 0;
  for (int64_t i00 = (int64_t)blockIdx.x * kTpBlock; i00 < n; i00 += (int64_t)gridDim.x * kTpBlock) {  // (block-uniform)
    __syncthreads();  // the last trip's appends are in ...
    const unsigned int f0 = fill[0], f1 = fill[1];
    __syncthreads();  // ... and read by every thread before this trip's begin: the two decisions are the workgroup's
    if (f0 + kTpBlock > kTpStage) tp_flush(stage[0], &fill[0], &base[0], &state[kTpSelCursor], sel, sel_cap);
    if (f1 + kTpBlock > kTpStage) tp_flush(stage[1], &fill[1], &base[1], &state[kTpTieCursor], tie, tie_cap);
    const int64_t i0 = i00 + (int64_t)threadIdx.x * kTpItems;
    float v[kTpItems];
    tp_load_scores(s, i0, n, wide, v);
    bool up[kTpItems], eq[kTpItems];
    unsigned long long vu[kTpItems], ve[kTpItems];
    for (int j = 0; j < kTpItems; ++j) {
      const uint32_t ik = ~topk_key(v[j]);
      const bool in = i0 + j < n;
      eq[j] = in && ik == T;
      up[j] = in && (ik < T || (ties_all && eq[j]));
      if (ties_all) eq[j] = false;
      vu[j] = __ballot(up[j]);
      ve[j] = __ballot(eq[j]);
    }
    unsigned int at = tp_wave_places(&fill[0], vu, lane);
    for (int j = 0; j < kTpItems; ++j) {
      const unsigned int o = at + (unsigned)__popcll(vu[j] & below);
      if (up[j] && o < (unsigned)kTpStage) stage[0][o] = (uint32_t)(i0 + j);
      at += (unsigned)__popcll(vu[j]);
    }
    at = tp_wave_places(&fill[1], ve, lane);
    for (int j = 0; j < kTpItems; ++j) {
      const unsigned int o = at + (unsigned)__popcll(ve[j] & below);
      if (eq[j] && o < (unsigned)kTpStage) stage[1][o] = (uint32_t)(i0 + j);
      at += (unsigned)__popcll(ve[j]);
    }
  }
  __syncthreads();
  tp_flush(stage[0], &fill[0], &base[0], &state[kTpSelCursor], sel, sel_cap);
  tp_flush(stage[1], &fill[1], &base[1], &state[kTpTieCursor], tie, tie_cap);
}

// the list, the ids behind it and the packing of (row, slot): what the tie and rank kernels gather from
struct TpList {
  const int32_t *q, *c;
  const float *s;
  int64_t n;  // pairs of the list
  const int64_t *q_ext, *c_ext;
  int64_t nq, n_store;
  int slot_bits;  // (row << slot_bits) | slot is a pair's last field
  int pos_bits;   // row bits + slot bits (<= 62)
};

__device__ inline unsigned long long tp_q_bits(const TpList &l, int32_t q) {
  const int64_t e = (q >= 0 && q < l.nq) ? l.q_ext[q] : 0;
  return (unsigned long long)e ^ 0x8000000000000000ull;  // signed order as unsigned
}
__device__ inline unsigned long long tp_pos_bits(const TpList &l, int32_t q, int32_t c) {
  return ((unsigned long long)(uint32_t)q << l.slot_bits) | (unsigned long long)(uint32_t)c;
}
// the tie key of pair i: (query id, candidate id, (row, slot) left-aligned), ascending = rank order
// (an index the stage wrote is below n; one it did not write -- a count that disagrees, reported by the host -- reads pair 0)
__device__ inline uint32_t tp_pair(const TpList &l, uint32_t i) { return (int64_t)i < l.n ? i : 0u; }
__device__ inline void tp_tie_key(const TpList &l, uint32_t i, unsigned long long (&w)[3]) {
  i = tp_pair(l, i);
  const int32_t q = l.q[i], c = l.c[i];
  w[0] = tp_q_bits(l, q);
  w[1] = topk_ext_bits(l.c_ext, c, l.n_store);
  w[2] = tp_pos_bits(l, q, c) << (64 - l.pos_bits);
}
// the first nd 8-bit digits of w against T's: -1 below, 0 equal, 1 above
__device__ inline int tp_tie_cmp(const unsigned long long (&w)[3], const unsigned long long (&T)[3], int nd) {
  for (int x = 0; x < 3; ++x) {
    const int dw = nd - 8 * x;
    if (dw <= 0) return 0;
    const int sh = dw >= 8 ? 0 : 64 - 8 * dw;
    const unsigned long long a = w[x] >> sh, b = T[x] >> sh;
    if (a != b) return a < b ? -1 : 1;
  }
  return 0;
}

// tie pass d: digit d of the tie key over the tied pairs that match the d digits found so far
__global__ __launch_bounds__(kTpThreads) void k_tp_tie_hist(const uint32_t *__restrict__ tie, int64_t n_tie, const TpList l,
                                                            const unsigned long long *__restrict__ state, int d,
                                                            unsigned long long *__restrict__ ghist) {
  __shared__ unsigned int hist[kTpBins];
  if (state[kTpDone]) return;  // (uniform)
  hist[threadIdx.x] = 0u;
  __syncthreads();
  const unsigned long long T[3] = {state[kTpTie0], state[kTpTie0 + 1], state[kTpTie0 + 2]};
  const int sh = 56 - 8 * (d % 8);
  for (int64_t base = (int64_t)blockIdx.x * kTpThreads; base < n_tie; base += (int64_t)gridDim.x * kTpThreads) {  // (block-uniform)
    const int64_t i = base + threadIdx.x;
    bool match = false;
    uint32_t dig = 0u;
    if (i < n_tie) {
      unsigned long long w[3];
      tp_tie_key(l, tie[i], w);
      match = tp_tie_cmp(w, T, d) == 0;
      dig = (uint32_t)(w[d / 8] >> sh) & 255u;
    }
    tp_hist_add(hist, match, dig);
  }
  __syncthreads();
  const unsigned int mine = hist[threadIdx.x];
  if (mine) atomicAdd(&ghist[threadIdx.x], (unsigned long long)mine);
}

// the ties below the tie key found, and `remaining` of those that equal its digits, behind the pairs above T in the selection
__global__ __launch_bounds__(kTpThreads) void k_tp_tie_collect(const uint32_t *__restrict__ tie, int64_t n_tie, const TpList l,
                                                               unsigned long long *__restrict__ state, uint32_t *__restrict__ sel,
                                                               unsigned long long sel_cap) {
  const unsigned long long T[3] = {state[kTpTie0], state[kTpTie0 + 1], state[kTpTie0 + 2]};
  const int nd = (int)state[kTpDigits];
  const unsigned long long remaining = state[kTpRemaining];
  const int lane = threadIdx.x % kTpWave;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int64_t base = (int64_t)blockIdx.x * kTpThreads; base < n_tie; base += (int64_t)gridDim.x * kTpThreads) {  // (block-uniform)
    const int64_t i = base + threadIdx.x;
    uint32_t idx = 0u;
    int cmp = 1;
    if (i < n_tie) {
      idx = tie[i];
      unsigned long long w[3];
      tp_tie_key(l, idx, w);
      cmp = tp_tie_cmp(w, T, nd);
    }
    // pairs equal to every digit found: the first `remaining` that ask (all of them, unless whole keys repeat)
    const unsigned long long ve = __ballot(cmp == 0);
    unsigned long long first = 0ull;
    if (ve) {
      if (lane == 0) first = atomicAdd(&state[kTpTieTaken], (unsigned long long)__popcll(ve));
      first = __shfl(first, 0);
    }
    const bool keep = cmp < 0 || (cmp == 0 && first + (unsigned long long)__popcll(ve & below) < remaining);
    const unsigned long long vk = __ballot(keep);
    if (vk == 0ull) continue;  // (wave-uniform)
    unsigned long long at = 0ull;
    if (lane == 0) at = atomicAdd(&state[kTpSelCursor], (unsigned long long)__popcll(vk));
    at = __shfl(at, 0) + (unsigned long long)__popcll(vk & below);
    if (keep && at < sel_cap) sel[at] = idx;
  }
}

// The sort key of one field for the m selected pairs, gathered through `perm` (pair indices in the order so far).
// level 0: (row, slot) -- perm_in is the selection (null: the whole list, pair j, which perm_out then gets); 1: candidate id;
// 2: query id; 3: the inverted score key (32 bits, in keys32).
__global__ __launch_bounds__(kTpThreads) void k_tp_keys(int level, const uint32_t *__restrict__ perm_in, int64_t m, const TpList l,
                                                        unsigned long long *__restrict__ keys, uint32_t *__restrict__ keys32,
                                                        uint32_t *__restrict__ perm_out) {
  for (int64_t j = (int64_t)blockIdx.x * kTpThreads + threadIdx.x; j < m; j += (int64_t)gridDim.x * kTpThreads) {
    const uint32_t i = tp_pair(l, perm_in ? perm_in[j] : (uint32_t)j);
    if (level == 0) {
      keys[j] = tp_pos_bits(l, l.q[i], l.c[i]);
      if (!perm_in) perm_out[j] = i;  // (the selection already lies there)
    } else if (level == 1) {
      keys[j] = topk_ext_bits(l.c_ext, l.c[i], l.n_store);
    } else if (level == 2) {
      keys[j] = tp_q_bits(l, l.q[i]);
    } else {
      keys32[j] = ~topk_key(l.s[i]);
    }
  }
}

__global__ __launch_bounds__(kTpThreads) void k_tp_write(const uint32_t *__restrict__ perm, int64_t m, const TpList l,
                                                         int32_t *__restrict__ out_q, int32_t *__restrict__ out_c, float *__restrict__ out_s) {
  for (int64_t j = (int64_t)blockIdx.x * kTpThreads + threadIdx.x; j < m; j += (int64_t)gridDim.x * kTpThreads) {
    const uint32_t i = tp_pair(l, perm[j]);
    out_q[j] = l.q[i];
    out_c[j] = l.c[i];
    out_s[j] = topk_key_inv(topk_key(l.s[i]));  // (the same bits, but +0.0f for -0.0f)
  }
}

// ---- host side: the stage's buffers (owned by a handle) and its launches
struct TpWork {
  DevBuf<unsigned long long> state;  // [kTpWords]
  DevBuf<unsigned long long> hist;   // [(kTpScorePasses + kTpTieDigitsMax) * kTpBins]
  DevBuf<uint32_t> tie;              // one index per pair at the K-th score, when a tie select runs
  DevBuf<unsigned long long> key_a, key_b;  // [out_s.cap each, as the next four] a field's keys before / after its sort
  DevBuf<uint32_t> perm_a, perm_b;          // the selection / the permutation
  DevBuf<int32_t> out_q, out_c;             // the stage's output
  DevBuf<float> out_s;
  DevBuf<char> tmp;  // rocprim's scratch
  StageMem mem;
};

inline int tp_bits(int64_t n) {  // bits that hold 0 .. n - 1 (at least 1)
  int b = 1;
  while (b < 63 && (1LL << b) < n) ++b;
  return b;
}

// Runs the stage over (q, c, s)[0, n), 0 < n < 2^32, on `stream` and waits for it.  The new list is w.out_*[0, info->kept).
// grid_cap: the most workgroups of a grid-stride kernel.  words: kTpWords host words for the two reads (pinned, or the caller's
// stack).  info: pairs_in, kept, above, tied, tied_kept, kth_score, launches, select_ms are filled.  *bad (a message): the stage's
// own counts disagree (hipErrorUnknown is returned).
inline hipError_t tp_run(TpWork &w, hipStream_t stream, const int32_t *q, const int32_t *c, const float *s, int64_t n, const int64_t *q_ext,
                         int64_t nq, const int64_t *c_ext, int64_t n_store, int64_t K, int64_t grid_cap, unsigned long long *words,
                         apss_top_pairs_info *info, const char **bad) {
  hipError_t e;
  const int64_t m = std::min<int64_t>(K, n);
  const bool cut = n > K;
  constexpr size_t kHistWords = (size_t)(kTpScorePasses + kTpTieDigitsMax) * kTpBins;
  if (!w.state.p) {
    if ((e = w.mem.grow((size_t)kTpWords, w.state)) != hipSuccess) return e;
    if ((e = w.mem.grow(kHistWords, w.hist)) != hipSuccess) return e;
  }
  TpList l{};
  l.q = q, l.c = c, l.s = s, l.n = n, l.q_ext = q_ext, l.c_ext = c_ext, l.nq = nq, l.n_store = n_store;
  l.slot_bits = tp_bits(n_store);
  l.pos_bits = l.slot_bits + tp_bits(nq);
  // the rank order's buffers, and the scratch of its widest sort
  size_t tmp_pos = 0, tmp64 = 0, tmp32 = 0;
  if ((e = rocprim::radix_sort_pairs(nullptr, tmp_pos, w.key_a.p, w.key_b.p, w.perm_a.p, w.perm_b.p, (size_t)m, 0, (unsigned)l.pos_bits, stream)) != hipSuccess)
    return e;
  if ((e = rocprim::radix_sort_pairs(nullptr, tmp64, w.key_a.p, w.key_b.p, w.perm_a.p, w.perm_b.p, (size_t)m, 0, 64, stream)) != hipSuccess) return e;
  if ((e = rocprim::radix_sort_pairs(nullptr, tmp32, (uint32_t *)nullptr, (uint32_t *)nullptr, w.perm_a.p, w.perm_b.p, (size_t)m, 0, 32, stream)) != hipSuccess)
    return e;
  const size_t tmp_need = std::max(tmp_pos, std::max(tmp64, tmp32)) + 256;
  if ((e = w.mem.grow(tmp_need, w.tmp)) != hipSuccess) return e;
  if ((size_t)m > w.out_s.cap) {  // (the array grown last says whether all seven have the room)
    const size_t cap = std::min<size_t>((size_t)APSS_TOP_PAIRS_MAX, std::max<size_t>((size_t)m + (size_t)m / 8, 1024));
    if ((e = w.mem.grow(cap, w.key_a, w.key_b, w.perm_a, w.perm_b, w.out_q, w.out_c, w.out_s)) != hipSuccess) return e;
  }
  const auto grid = [&](int64_t items, int64_t per) { return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((items + per - 1) / per, grid_cap))); };
  if ((e = begin_timed(stream, w.mem.e0)) != hipSuccess) return e;
  int64_t above = 0, tied = 0;
  const uint32_t *selection = nullptr;  // (n <= K: the whole list)
  if (cut) {
    // ---- 1. the K-th score key
    for (int k = 0; k < kTpWords; ++k) words[k] = 0ull;
    words[kTpRemaining] = (unsigned long long)K;
    if ((e = hipMemcpyAsync(w.state.p, words, kTpWords * sizeof(unsigned long long), hipMemcpyHostToDevice, stream)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(w.hist.p, 0, kHistWords * sizeof(unsigned long long), stream)) != hipSuccess) return e;
    // (words is read by the copy when the stream gets there; it is next written after the wait below)
    for (int p = 0; p < kTpScorePasses; ++p) {
      unsigned long long *gh = w.hist.p + (size_t)p * kTpBins;
      hipLaunchKernelGGL(k_tp_hist, grid(n, kTpTrips * kTpBlock), dim3(kTpThreads), 0, stream, s, n, (const unsigned long long *)w.state.p, p, gh);
      hipLaunchKernelGGL(k_tp_pick, dim3(1), dim3(kTpBins), 0, stream, (const unsigned long long *)gh, w.state.p, (int)kTpT, 24 - 8 * p,
                         p == kTpScorePasses - 1 ? 1 : 0, 0, (unsigned long long)K);
      info->launches += 2;
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(words, w.state.p, kTpWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;  // the first wait: (G, E) size the tie list
    above = (int64_t)words[kTpAbove];
    tied = (int64_t)words[kTpTied];
    if (above < 0 || above >= K || tied <= 0 || above + tied < K || above + tied > n) {
      *bad = "the score select's counts disagree with the list";
      return hipErrorUnknown;
    }
    const uint32_t T = (uint32_t)words[kTpT];
    const int64_t want = K - above;  // ties kept
    const bool ties_all = want == tied;
    if (!ties_all && (size_t)tied > w.tie.cap && (e = w.mem.grow((size_t)tied + (size_t)tied / 8 + 1024, w.tie)) != hipSuccess) return e;
    // ---- 2. collect
    hipLaunchKernelGGL(k_tp_collect, grid(n, kTpTrips * kTpBlock), dim3(kTpThreads), 0, stream, s, n, w.state.p, w.perm_a.p, (unsigned long long)m, w.tie.p,
                       (unsigned long long)(ties_all ? 0 : tied), ties_all ? 1 : 0);
    ++info->launches;
    // ---- 3. ties: `remaining` is already the wanted rank among them
    if (!ties_all) {
      const int digits = 16 + (l.pos_bits + 7) / 8;
      for (int d = 0; d < digits; ++d) {
        unsigned long long *gh = w.hist.p + (size_t)(kTpScorePasses + d) * kTpBins;
        hipLaunchKernelGGL(k_tp_tie_hist, grid(tied, kTpThreads), dim3(kTpThreads), 0, stream, (const uint32_t *)w.tie.p, tied, l,
                           (const unsigned long long *)w.state.p, d, gh);
        hipLaunchKernelGGL(k_tp_pick, dim3(1), dim3(kTpBins), 0, stream, (const unsigned long long *)gh, w.state.p, kTpTie0 + d / 8,
                           56 - 8 * (d % 8), 0, 1, 0ull);
        info->launches += 2;
      }
      hipLaunchKernelGGL(k_tp_tie_collect, grid(tied, kTpThreads), dim3(kTpThreads), 0, stream, (const uint32_t *)w.tie.p, tied, l, w.state.p,
                         w.perm_a.p, (unsigned long long)m);
      ++info->launches;
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
    selection = w.perm_a.p;
    info->above = above;
    info->tied = tied;
    info->tied_kept = want;
    info->kth_score = (double)topk_key_inv(~T);
  }
  // ---- 4. rank order: stable sorts, least significant field first
  uint32_t *pa = w.perm_a.p, *pb = w.perm_b.p;
  for (int level = 0; level < 4; ++level) {
    hipLaunchKernelGGL(k_tp_keys, grid(m, kTpThreads), dim3(kTpThreads), 0, stream, level, level == 0 ? selection : (const uint32_t *)pa, m, l,
                       w.key_a.p, reinterpret_cast<uint32_t *>(w.key_a.p), pa);
    ++info->launches;
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t tmp_bytes = w.tmp.cap;
    if (level == 3)
      e = rocprim::radix_sort_pairs((void *)w.tmp.p, tmp_bytes, reinterpret_cast<uint32_t *>(w.key_a.p), reinterpret_cast<uint32_t *>(w.key_b.p), pa, pb,
                                    (size_t)m, 0, 32, stream);
    else
      e = rocprim::radix_sort_pairs((void *)w.tmp.p, tmp_bytes, w.key_a.p, w.key_b.p, pa, pb, (size_t)m, 0, level == 0 ? (unsigned)l.pos_bits : 64u, stream);
    if (e != hipSuccess) return e;
    std::swap(pa, pb);
  }
  hipLaunchKernelGGL(k_tp_write, grid(m, kTpThreads), dim3(kTpThreads), 0, stream, (const uint32_t *)pa, m, l, w.out_q.p, w.out_c.p, w.out_s.p);
  ++info->launches;
  if ((e = hipGetLastError()) != hipSuccess) return e;
  float ms = 0.f;  // (the second wait ends the stage)
  if ((e = end_timed_read(stream, w.mem.e0, w.mem.e1, {{words, w.state.p, cut ? kTpWords * sizeof(unsigned long long) : 0}}, &ms)) != hipSuccess) return e;
  if (cut && (int64_t)words[kTpSelCursor] != K) {
    *bad = "the selection does not hold K pairs";
    return hipErrorUnknown;
  }
  info->select_ms = ms;
  info->kept = m;
  return hipSuccess;
}

}  // namespace
}  // namespace apss

#endif  // APSS_TOP_PAIRS_HPP
