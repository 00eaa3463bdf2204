// apss_window.hpp -- per-query top-k in bounded memory (include/apss.h: apss_set_top_k_window; DESIGN.md 5e "Windows").
//
// A query-type call with k > 0 and a window budget joins and cuts WINDOWS of consecutive query rows.  What sizes a window is a
// bound on the pairs its uncut list can hold: b(q) = min(sum of df_t over the terms t of row q, stored rows), df_t = stored rows
// holding term t.  Every reported pair shares a term, and a candidate is counted once for each term it shares, so b(q) is at
// least the number of distinct candidates of row q.
//
//   k_win_df      exact term counts over the store's entries.  A stored row holds a term at most once, so df is a histogram of
//                 idx[0, nnz): a workgroup aggregates its 1024 entries in an LDS hash table keyed by term (the table of
//                 k_topk_count) and adds once per distinct term to the global counters -- a frequent term costs a workgroup one
//                 global atomic, not one per posting.
//   k_win_bound   one wave per query row: gathers df[idx], sums in 64 bits, clamps at the stored rows, writes int32 b[nq]; for a
//                 stored batch of a handle with a dense-head block also whether the row has tail-view / head entries (the
//                 self-touch corrections of the statistics, per window).
//   k_win_append  a window's kept (slot, score) to the call's output arrays at the running offset, query row + r0.
#ifndef APSS_WINDOW_HPP
#define APSS_WINDOW_HPP

#include <hip/hip_runtime.h>

#include <cstdint>

#include "apss_topk.hpp"

namespace apss {
namespace {

constexpr int kWinThreads = 256;
constexpr int kWinWave = 64;

__global__ __launch_bounds__(kTopkThreads) void k_win_df(const int32_t *__restrict__ idx, int64_t nnz, int32_t dim,
                                                         unsigned int *__restrict__ df) {
  __shared__ int32_t keys[kTopkSlots];
  __shared__ unsigned int vals[kTopkSlots];
  for (int s = threadIdx.x; s < kTopkSlots; s += kTopkThreads) {
    keys[s] = -1;
    vals[s] = 0u;
  }
  __syncthreads();
  const int64_t i0 = (int64_t)blockIdx.x * kTopkBlock + (int64_t)threadIdx.x * kTopkItems;
  if (i0 < nnz) {
    int32_t t[kTopkItems];
    topk_load_rows(idx, i0, nnz, dim, t);  // (terms outside [0, dim) -- there are none in a validated store -- become -1)
    for (int j = 0; j < kTopkItems; ++j)
      if (t[j] >= 0) atomicAdd(&vals[topk_slot_of(t[j], keys)], 1u);
  }
  __syncthreads();
  for (int s = threadIdx.x; s < kTopkSlots; s += kTopkThreads)
    if (keys[s] >= 0) atomicAdd(&df[keys[s]], vals[s]);
}

// q_rowptr: the batch's row offsets into q_idx (absolute for rows of the store).  sv_rowptr (may be null): the same rows' offsets
// in the tail view of a handle with a dense-head block; then ne[q] = (tail-view entries ? 1 : 0) | (head entries ? 2 : 0).
__global__ __launch_bounds__(kWinThreads) void k_win_bound(const int64_t *__restrict__ q_rowptr, const int32_t *__restrict__ q_idx,
                                                           int64_t nq, const unsigned int *__restrict__ df, int32_t dim,
                                                           int64_t stored_rows, const int64_t *__restrict__ sv_rowptr,
                                                           int32_t *__restrict__ b, int32_t *__restrict__ ne) {
  const int64_t q = ((int64_t)blockIdx.x * kWinThreads + threadIdx.x) / kWinWave;
  const int lane = threadIdx.x % kWinWave;
  if (q >= nq) return;
  const int64_t lo = q_rowptr[q], hi = q_rowptr[q + 1];
  unsigned long long sum = 0ull;
  for (int64_t i = lo + lane; i < hi; i += kWinWave) {
    const int32_t t = q_idx[i];
    if (t >= 0 && t < dim) sum += df[t];
  }
  sum = wave_sum(sum);
  if (lane == 0) {
    b[q] = (int32_t)(sum < (unsigned long long)stored_rows ? sum : (unsigned long long)stored_rows);
    if (sv_rowptr) {
      const int64_t sv = sv_rowptr[q + 1] - sv_rowptr[q];
      ne[q] = (sv > 0 ? 1 : 0) | (hi - lo > sv ? 2 : 0);
    }
  }
}

__global__ __launch_bounds__(kWinThreads) void k_win_append(const int32_t *__restrict__ in_q, const int32_t *__restrict__ in_c,
                                                            const float *__restrict__ in_s, int64_t n, int32_t r0,
                                                            int32_t *__restrict__ out_q, int32_t *__restrict__ out_c,
                                                            float *__restrict__ out_s) {
  for (int64_t i = (int64_t)blockIdx.x * kWinThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kWinThreads) {
    out_q[i] = in_q[i] + r0;
    out_c[i] = in_c[i];
    out_s[i] = in_s[i];
  }
}

}  // namespace
}  // namespace apss

#endif  // APSS_WINDOW_HPP
