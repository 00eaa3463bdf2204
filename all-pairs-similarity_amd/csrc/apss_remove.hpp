// apss_remove.hpp -- removal of stored vectors (include/apss.h: apss_remove, apss_compact).
//
// A removed row keeps its slot until a compaction: one MARK byte per slot says whether the row is dead.  The probe kernels never
// read it -- every path of a query-type call ends in one final (query row, slot, score) list, and that list is filtered once.
//
//   k_rm_mark     ONE pass over the store's external ids per call: the removal list is sorted first (rocprim radix sort), every
//                 thread loads two ids with one 16-B load, looks each up by binary search and writes the mark with an ordinary
//                 byte store.  The rows newly marked are summed per wave (shuffles), per workgroup (LDS): one global add each.
//   k_rm_drop     stream compaction of the final list into another pair list (never in place: with unordered places a
//                 workgroup's writes would overtake another's unread input).  A lane holds four consecutive pairs (16-B loads);
//                 a wave takes its places with four ballots + popcounts and ONE returning global add.  Not stable across waves.
//   k_rm_rows     compaction, step 1: per slot the live flag and the live row's entry count (the handle's scan turns both into
//                 destinations).
//   k_rm_gather   compaction, step 2: one wave per live row copies its offset, external id and entries to their destinations.
#ifndef APSS_REMOVE_HPP
#define APSS_REMOVE_HPP

#include <hip/hip_runtime.h>

#include <cstdint>

#include "apss_stage.hpp"

namespace apss {
namespace {

constexpr int kRmThreads = 256;
constexpr int kRmWave = 64;
constexpr int kRmItems = 4;  // pairs per lane of k_rm_drop

// is `key` in the ascending list ids[0, n)?  (n > 0)
__device__ inline bool rm_listed(const int64_t *__restrict__ ids, int64_t n, int64_t lo_id, int64_t hi_id, int64_t key) {
  return sorted_find(ids, n, lo_id, hi_id, key) >= 0;
}

// ext[rows]: the store's external ids (16-B aligned); ids[n_ids]: the removal list, ascending, n_ids > 0; dead[rows]
__global__ __launch_bounds__(kRmThreads) void k_rm_mark(const int64_t *__restrict__ ext, int64_t rows, const int64_t *__restrict__ ids,
                                                        int64_t n_ids, uint8_t *__restrict__ dead, unsigned long long *__restrict__ newly) {
  __shared__ unsigned int part[kRmThreads / kRmWave];
  const int64_t lo_id = ids[0], hi_id = ids[n_ids - 1];
  unsigned int mine = 0;
  const int64_t n2 = (rows + 1) / 2;
  for (int64_t p = (int64_t)blockIdx.x * kRmThreads + threadIdx.x; p < n2; p += (int64_t)gridDim.x * kRmThreads) {
    const int64_t r = 2 * p;
    const bool two = r + 1 < rows;
    int64_t e0, e1;
    load_two_ids(ext, r, two, e0, e1);
    if (!dead[r] && rm_listed(ids, n_ids, lo_id, hi_id, e0)) {
      dead[r] = 1;
      ++mine;
    }
    if (two && !dead[r + 1] && rm_listed(ids, n_ids, lo_id, hi_id, e1)) {
      dead[r + 1] = 1;
      ++mine;
    }
  }
  mine = wave_sum(mine);
  if (threadIdx.x % kRmWave == 0) part[threadIdx.x / kRmWave] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int sum = 0;
    for (int w = 0; w < kRmThreads / kRmWave; ++w) sum += part[w];
    if (sum) atomicAdd(newly, (unsigned long long)sum);
  }
}

struct RmDropArgs {
  const int32_t *in_q, *in_c;
  const float *in_s;
  int64_t n;
  const uint8_t *dead;   // [rows]
  int64_t rows;
  int64_t q_slot_first;  // the query batch is the stored rows from this slot on (< 0: an outside batch)
  int32_t *out_q, *out_c;
  float *out_s;
  unsigned long long *kept;  // [1], zero before the launch
};

__global__ __launch_bounds__(kRmThreads) void k_rm_drop(const RmDropArgs a) {
  const int lane = threadIdx.x % kRmWave;
  const int64_t wave = ((int64_t)blockIdx.x * kRmThreads + threadIdx.x) / kRmWave;
  const int64_t n_waves = (int64_t)gridDim.x * (kRmThreads / kRmWave);
  constexpr int64_t kSpan = (int64_t)kRmWave * kRmItems;
  const unsigned long long below = (1ull << lane) - 1ull;
  // (the lists start at their arrays' first element, which the device allocation aligns; a caller that ever hands in an offset view reads by element)
  const bool wide = ((reinterpret_cast<uintptr_t>(a.in_q) | reinterpret_cast<uintptr_t>(a.in_c) | reinterpret_cast<uintptr_t>(a.in_s)) & 15u) == 0;
  for (int64_t base = wave * kSpan; base < a.n; base += n_waves * kSpan) {  // (wave-uniform: every lane takes part in the ballots)
    const int64_t i0 = base + (int64_t)lane * kRmItems;
    int32_t q[kRmItems], c[kRmItems];
    float s[kRmItems];
    if (wide && i0 + kRmItems <= a.n) {
      const int4 vq = *reinterpret_cast<const int4 *>(a.in_q + i0), vc = *reinterpret_cast<const int4 *>(a.in_c + i0);
      const float4 vs = *reinterpret_cast<const float4 *>(a.in_s + i0);
      q[0] = vq.x, q[1] = vq.y, q[2] = vq.z, q[3] = vq.w;
      c[0] = vc.x, c[1] = vc.y, c[2] = vc.z, c[3] = vc.w;
      s[0] = vs.x, s[1] = vs.y, s[2] = vs.z, s[3] = vs.w;
    } else {
      for (int j = 0; j < kRmItems; ++j) {
        const bool in = i0 + j < a.n;
        q[j] = in ? a.in_q[i0 + j] : 0;
        c[j] = in ? a.in_c[i0 + j] : 0;
        s[j] = in ? a.in_s[i0 + j] : 0.f;
      }
    }
    bool keep[kRmItems];
    unsigned long long votes[kRmItems];
    int total = 0;
    for (int j = 0; j < kRmItems; ++j) {
      bool live = i0 + j < a.n;
      if (live) {
        const int64_t cs = c[j], qs = a.q_slot_first + q[j];
        if (cs >= 0 && cs < a.rows && a.dead[cs]) live = false;
        if (a.q_slot_first >= 0 && qs < a.rows && a.dead[qs]) live = false;
      }
      keep[j] = live;
      votes[j] = __ballot(live);
      total += __popcll(votes[j]);
    }
    if (total == 0) continue;
    unsigned long long at = 0;
    if (lane == 0) at = atomicAdd(a.kept, (unsigned long long)total);
    at = __shfl(at, 0);
    for (int j = 0; j < kRmItems; ++j) {
      if (keep[j]) {
        const unsigned long long o = at + (unsigned long long)__popcll(votes[j] & below);
        a.out_q[o] = q[j];
        a.out_c[o] = c[j];
        a.out_s[o] = s[j];
      }
      at += (unsigned long long)__popcll(votes[j]);
    }
  }
}

// keep[r] = the row is live, cnt[r] = its entries if it is (rowptr: the store's absolute offsets)
__global__ __launch_bounds__(kRmThreads) void k_rm_rows(const uint8_t *__restrict__ dead, const int64_t *__restrict__ rowptr, int64_t rows,
                                                        int64_t *__restrict__ keep, int64_t *__restrict__ cnt) {
  for (int64_t r = (int64_t)blockIdx.x * kRmThreads + threadIdx.x; r < rows; r += (int64_t)gridDim.x * kRmThreads) {
    const bool live = !dead[r];
    keep[r] = live ? 1 : 0;
    cnt[r] = live ? rowptr[r + 1] - rowptr[r] : 0;
  }
}

struct RmGatherArgs {
  const uint8_t *dead;
  const int64_t *rowptr, *ext;  // the store
  const int32_t *idx;
  const float *val;
  int64_t rows;
  const int64_t *row_dst, *nnz_dst;  // [rows + 1] exclusive scans of k_rm_rows' keep / cnt
  int64_t *o_rowptr, *o_ext;         // [live rows + 1] batch-relative offsets, [live rows]
  int32_t *o_idx;
  float *o_val;
};

__global__ __launch_bounds__(kRmThreads) void k_rm_gather(const RmGatherArgs a) {
  const int64_t r = ((int64_t)blockIdx.x * kRmThreads + threadIdx.x) / kRmWave;
  const int lane = threadIdx.x % kRmWave;
  if (r >= a.rows) return;
  if (r == a.rows - 1 && lane == 0) a.o_rowptr[a.row_dst[a.rows]] = a.nnz_dst[a.rows];
  if (a.dead[r]) return;
  const int64_t lo = a.rowptr[r], len = a.rowptr[r + 1] - lo, d = a.row_dst[r], o = a.nnz_dst[r];
  if (lane == 0) {
    a.o_rowptr[d] = o;
    a.o_ext[d] = a.ext[r];
  }
  for (int64_t i = lane; i < len; i += kRmWave) {
    a.o_idx[o + i] = a.idx[lo + i];
    a.o_val[o + i] = a.val[lo + i];
  }
}

}  // namespace
}  // namespace apss

#endif  // APSS_REMOVE_HPP
