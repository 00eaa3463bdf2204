// apss_query_stored.hpp -- a query batch made of STORED rows, named by external id (include/apss.h: apss_query_stored).
//
// The id list is sorted first (rocprim radix sort, as apss_remove's); then
//
//   k_qs_select   ONE pass over the store's external ids: every thread loads two ids with one 16-B load, looks each up in the sorted
//                 list by binary search and writes, per slot, the keep flag and the entry count the handle's scan turns into
//                 destinations.  A marked row (apss_remove) is not selected; with nothing marked the mark pointer is null and
//                 nothing of the map is read.  A hit sets the FOUND byte at the id's first position in the sorted list with an
//                 ordinary byte store (racing writers all write 1).
//   k_qs_ids      one pass over the sorted list: distinct ids, and distinct ids without a found byte.  Summed per wave (shuffles),
//                 per workgroup (LDS): one global add per workgroup and counter.
//   k_qs_slots    every selected slot to its rank: the compact slot list the gather's grid is sized by.
//   k_qs_gather   one wave per SELECTED row (not per stored row): offset, external id and entries straight into the query staging,
//                 and in the same pass the batch summaries the probe plans with -- the longest row, the largest squared norm,
//                 whether any weight is negative, the non-empty rows -- in the flag words of the ingest kernels.
#ifndef APSS_QUERY_STORED_HPP
#define APSS_QUERY_STORED_HPP

#include <hip/hip_runtime.h>

#include <cstdint>

#include "apss_stage.hpp"

namespace apss {
namespace {

constexpr int kQsThreads = 256;
constexpr int kQsWave = 64;
constexpr int kQsNormLanes = 16;  // lanes that sum a row's squares: kGroup of the ingest kernels, whose bits the sum must keep

struct QsSelectArgs {
  const int64_t *ext;     // [rows] the store's external ids (16-B aligned)
  const int64_t *rowptr;  // [rows + 1] the store's absolute offsets
  int64_t rows;
  const uint8_t *dead;    // [rows] marks, or null: nothing is marked
  const int64_t *ids;     // [n_ids] the named ids, ascending, n_ids > 0
  int64_t n_ids;
  uint8_t *found;         // [n_ids] zero before the launch
  int64_t *keep, *cnt;    // [rows] (16-B aligned)
};

__global__ __launch_bounds__(kQsThreads) void k_qs_select(const QsSelectArgs a) {
  const int64_t lo_id = a.ids[0], hi_id = a.ids[a.n_ids - 1];
  const int64_t n2 = (a.rows + 1) / 2;
  for (int64_t p = (int64_t)blockIdx.x * kQsThreads + threadIdx.x; p < n2; p += (int64_t)gridDim.x * kQsThreads) {
    const int64_t r = 2 * p;
    const bool two = r + 1 < a.rows;
    int64_t e0, e1;
    load_two_ids(a.ext, r, two, e0, e1);
    const int64_t p0 = a.dead && a.dead[r] ? -1 : sorted_find(a.ids, a.n_ids, lo_id, hi_id, e0);
    const int64_t p1 = !two || (a.dead && a.dead[r + 1]) ? -1 : sorted_find(a.ids, a.n_ids, lo_id, hi_id, e1);
    longlong2 k, c;
    k.x = p0 >= 0 ? 1 : 0;
    k.y = p1 >= 0 ? 1 : 0;
    c.x = c.y = 0;
    if (p0 >= 0) {
      a.found[p0] = 1;
      c.x = a.rowptr[r + 1] - a.rowptr[r];
    }
    if (p1 >= 0) {
      a.found[p1] = 1;
      c.y = a.rowptr[r + 2] - a.rowptr[r + 1];
    }
    if (two) {
      *reinterpret_cast<longlong2 *>(a.keep + r) = k;
      *reinterpret_cast<longlong2 *>(a.cnt + r) = c;
    } else {
      a.keep[r] = k.x;
      a.cnt[r] = c.x;
    }
  }
}

// out[0] += distinct ids of ids[0, n) (ascending), out[1] += those whose found byte (at their first position) is 0
__global__ __launch_bounds__(kQsThreads) void k_qs_ids(const int64_t *__restrict__ ids, int64_t n, const uint8_t *__restrict__ found,
                                                       unsigned long long *__restrict__ out) {
  __shared__ unsigned int part[2][kQsThreads / kQsWave];
  unsigned int distinct = 0, missing = 0;
  for (int64_t i = (int64_t)blockIdx.x * kQsThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kQsThreads) {
    const bool first = i == 0 || ids[i - 1] != ids[i];
    if (first) {
      ++distinct;
      if (!found[i]) ++missing;
    }
  }
  distinct = wave_sum(distinct);
  missing = wave_sum(missing);
  if (threadIdx.x % kQsWave == 0) {
    part[0][threadIdx.x / kQsWave] = distinct;
    part[1][threadIdx.x / kQsWave] = missing;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    unsigned int sum = 0;
    for (int w = 0; w < kQsThreads / kQsWave; ++w) sum += part[threadIdx.x][w];
    if (sum) atomicAdd(out + threadIdx.x, (unsigned long long)sum);
  }
}

// slots[row_dst[r]] = r for every selected slot r (row_dst: the exclusive scan of keep)
__global__ __launch_bounds__(kQsThreads) void k_qs_slots(const int64_t *__restrict__ keep, const int64_t *__restrict__ row_dst, int64_t rows,
                                                         int32_t *__restrict__ slots) {
  for (int64_t r = (int64_t)blockIdx.x * kQsThreads + threadIdx.x; r < rows; r += (int64_t)gridDim.x * kQsThreads)
    if (keep[r]) slots[row_dst[r]] = (int32_t)r;
}

struct QsGatherArgs {
  const int32_t *slots;          // [n_sel] selected slots, ascending
  int64_t n_sel;                 // > 0
  const int64_t *rowptr, *ext;   // the store
  const int32_t *idx;
  const float *val;
  const int64_t *nnz_dst;        // [rows + 1] exclusive scan of k_qs_select's cnt
  int64_t *o_rowptr, *o_ext;     // [n_sel + 1] batch-relative offsets, [n_sel]
  int32_t *o_idx;
  float *o_val;
  unsigned int *flags_out;       // [4] zero before the launch; the words of IngestArgs::flags_out: [0] bit2 a negative weight,
                                 // [1] longest row, [2] bits of the largest squared row norm, [3] non-empty rows
};

__global__ __launch_bounds__(kQsThreads) void k_qs_gather(const QsGatherArgs a) {
  __shared__ unsigned int sh[4];
  if (threadIdx.x < 4) sh[threadIdx.x] = 0;
  __syncthreads();
  const int64_t j = ((int64_t)blockIdx.x * kQsThreads + threadIdx.x) / kQsWave;  // (wave-uniform)
  const int lane = threadIdx.x % kQsWave;
  if (j < a.n_sel) {
    const int64_t r = a.slots[j];
    const int64_t lo = a.rowptr[r], len = a.rowptr[r + 1] - lo, o = a.nnz_dst[r];
    if (lane == 0) {
      a.o_rowptr[j] = o;
      a.o_ext[j] = a.ext[r];
      if (j == a.n_sel - 1) a.o_rowptr[a.n_sel] = o + len;
    }
    bool neg = false;
    for (int64_t i = lane; i < len; i += kQsWave) {
      const float v = a.val[lo + i];
      a.o_idx[o + i] = a.idx[lo + i];
      a.o_val[o + i] = v;
      neg |= v < 0.f;
    }
    // the row's squared norm with the summation order of k_ingest_plain / k_ingest_count<kGroup> (16 lanes, each its entries in
    // order, rounded products, butterfly): the bits of the largest one scale the probe's accumulators, and the call must plan as
    // apss_query_dev of the same rows does.  (The 16 lanes read the row again; it is in the cache.)
    float full = 0.f;
    if (lane < kQsNormLanes)
      for (int64_t i = lane; i < len; i += kQsNormLanes) {
        const float v = a.val[lo + i];
        full += __fmul_rn(v, v);
      }
    for (int off = kQsNormLanes / 2; off; off >>= 1) full += __shfl_xor(full, off, kQsNormLanes);
    const bool any_neg = __ballot(neg) != 0ull;
    if (lane == 0) {
      if (any_neg) atomicOr(&sh[0], 4u);
      atomicMax(&sh[1], (unsigned int)len);
      atomicMax(&sh[2], __float_as_uint(full));
      if (len > 0) atomicAdd(&sh[3], 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (sh[0]) atomicOr(a.flags_out, sh[0]);
    if (sh[1]) atomicMax(a.flags_out + 1, sh[1]);
    if (sh[2]) atomicMax(a.flags_out + 2, sh[2]);
    if (sh[3]) atomicAdd(a.flags_out + 3, sh[3]);
  }
}

}  // namespace
}  // namespace apss

#endif  // APSS_QUERY_STORED_HPP
