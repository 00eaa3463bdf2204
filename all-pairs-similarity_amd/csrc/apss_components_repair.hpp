// apss_components_repair.hpp -- the components of the join across a removal and a compaction (include/apss.h:
// apss_set_components_repair).  gfx950, wave64.
//
// apss_remove that newly marks a row: the components that held one are taken apart and their live rows re-joined against the
// store, instead of every slot becoming a singleton.  On the handle's stream, behind k_rm_mark:
//
//   k_cc_label    (apss_components.hpp, mode 0) flattens the forest: parent[x] is x's root, label[] is zero.
//   k_cr_touch    every marked slot sets the FLAG byte of its root -- label[] read as bytes, free as scratch since it is out of date
//                 after any change anyway.  An ordinary byte store of 1; racing writers all write 1.  A row marked by an earlier
//                 call is a singleton (the invariant of DESIGN.md 5j) and flags only itself: no list of the new marks is needed.
//   k_cr_detach   ONE pass over the slots.  A slot whose root is flagged becomes its own parent; if it is live it writes keep = 1 and
//                 its entry count into the handle's scan arrays, the ones k_qs_select writes for apss_query_stored (k_qs_slots and
//                 k_qs_gather do not care who wrote them); every other slot writes 0, 0.  A detached slot that was no root takes one
//                 union back, a flagged root is one touched component: both counted per wave (ballot, popcount), one add each
//                 per wave.  A thread writes only parent[x] of its own slot and reads only that word and the flags, which nobody
//                 writes in this launch: nothing races.
//
// apss_compact: the forest moves with the rows.
//
//   k_cr_remap    the forest is flat; out[rank(x)] = rank(parent[x]) for every live slot x, rank = the scan of the live flags the
//                 compaction takes anyway.  Written aside (label[] again: the rebuild resets the structure on its way) and copied
//                 over parent[] after the rebuild.
//
// The per-slot decisions are apss_components_repair_core.hpp's.  No LDS, no scratch; grid-stride, 256 threads.
#ifndef APSS_COMPONENTS_REPAIR_HPP
#define APSS_COMPONENTS_REPAIR_HPP

#include <hip/hip_runtime.h>

#include <cstdint>

#include "apss_components.hpp"
#include "apss_components_repair_core.hpp"

namespace apss {
namespace {

// parent[] flat, flag[0, rows) zero, dead[0, rows)
__global__ __launch_bounds__(kCcThreads) void k_cr_touch(const int32_t *__restrict__ parent, const uint8_t *__restrict__ dead, int64_t rows,
                                                         uint8_t *__restrict__ flag) {
  for (int64_t x = (int64_t)blockIdx.x * kCcThreads + threadIdx.x; x < rows; x += (int64_t)gridDim.x * kCcThreads) {
    const int32_t f = cr_touch(dead[x] != 0, parent[x]);
    if (f >= 0) flag[f] = 1;
  }
}

struct CrDetachArgs {
  int32_t *parent;              // [rows] flat
  const uint8_t *flag, *dead;   // [rows]
  const int64_t *rowptr;        // [rows + 1] the store's offsets
  int64_t rows;
  int64_t *keep, *cnt;          // [rows] the handle's scan arrays
  unsigned long long *unions;   // [1] the structure's unions word
  unsigned long long *touched;  // [1] flagged roots; zero before the launch
};

__global__ __launch_bounds__(kCcThreads) void k_cr_detach(const CrDetachArgs a) {
  const int lane = threadIdx.x % kCcWave;
  const int64_t wave = ((int64_t)blockIdx.x * kCcThreads + threadIdx.x) / kCcWave;
  const int64_t n_waves = (int64_t)gridDim.x * (kCcThreads / kCcWave);
  unsigned int unhooked = 0, roots = 0;
  for (int64_t base = wave * kCcWave; base < a.rows; base += n_waves * kCcWave) {  // (wave-uniform: every lane takes part in the ballots)
    const int64_t x = base + lane;
    bool unhook = false, root = false;
    if (x < a.rows) {
      const int32_t p = a.parent[x];
      const bool flagged = a.flag[p] != 0;
      const CrDetach d = cr_detach((int32_t)x, p, flagged, a.dead[x] != 0);
      if (d.detach) a.parent[x] = (int32_t)x;
      a.keep[x] = d.select ? 1 : 0;
      a.cnt[x] = d.select ? a.rowptr[x + 1] - a.rowptr[x] : 0;
      unhook = d.unhook;
      root = flagged && p == (int32_t)x;
    }
    unhooked += (unsigned int)__popcll(__ballot(unhook));
    roots += (unsigned int)__popcll(__ballot(root));
  }
  if (lane == 0 && unhooked) atomicAdd(a.unions, 0ull - (unsigned long long)unhooked);  // (the word holds at least that many)
  if (lane == 0 && roots) atomicAdd(a.touched, (unsigned long long)roots);
}

// parent[] flat; rank[x] = live slots below x (exclusive scan of the live flags); out[0, live rows)
__global__ __launch_bounds__(kCcThreads) void k_cr_remap(const int32_t *__restrict__ parent, const uint8_t *__restrict__ dead,
                                                         const int64_t *__restrict__ rank, int64_t rows, int32_t *__restrict__ out) {
  for (int64_t x = (int64_t)blockIdx.x * kCcThreads + threadIdx.x; x < rows; x += (int64_t)gridDim.x * kCcThreads) {
    if (dead[x]) continue;
    const int32_t p = parent[x];
    const int64_t rx = rank[x];
    out[rx] = cr_renumber((int32_t)rx, (int32_t)rank[p], dead[p] != 0);
  }
}

// ---- host side
// flatten, touch, detach and select: launches only.  dead[0, n_rows) holds the call's marks; keep / cnt: [n_rows]; touched: [1], zero
inline hipError_t cr_detach_select(CcWork &w, hipStream_t stream, int64_t n_rows, const uint8_t *dead, const int64_t *rowptr, int64_t *keep,
                                   int64_t *cnt, unsigned long long *touched, int32_t *launches) {
  hipError_t e;
  if ((e = cc_extend(w, stream, n_rows, launches)) != hipSuccess) return e;
  const dim3 grid(cc_grid(n_rows, kCcGridCap)), block(kCcThreads);
  uint8_t *flag = reinterpret_cast<uint8_t *>(w.label.p);  // (the first n_rows bytes of label[0, n_rows): zero after the flattening)
  hipLaunchKernelGGL(k_cc_label, grid, block, 0, stream, w.parent.p, w.label.p, n_rows, 0, dead, n_rows);
  hipLaunchKernelGGL(k_cr_touch, grid, block, 0, stream, (const int32_t *)w.parent.p, dead, n_rows, flag);
  CrDetachArgs a{};
  a.parent = w.parent.p;
  a.flag = flag;
  a.dead = dead;
  a.rowptr = rowptr;
  a.rows = n_rows;
  a.keep = keep;
  a.cnt = cnt;
  a.unions = w.words.p;
  a.touched = touched;
  hipLaunchKernelGGL(k_cr_detach, grid, block, 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  *launches += 3;
  w.dirty = true;
  return hipSuccess;
}

// the forest of the live rows at their ranks, in label[0, live rows): launches only.  Nothing may use the structure until
// cr_install (a reset in between is fine: it launches nothing and frees nothing)
inline hipError_t cr_remap(CcWork &w, hipStream_t stream, int64_t n_rows, const uint8_t *dead, const int64_t *rank, int32_t *launches) {
  hipError_t e;
  if ((e = cc_extend(w, stream, n_rows, launches)) != hipSuccess) return e;
  const dim3 grid(cc_grid(n_rows, kCcGridCap)), block(kCcThreads);
  hipLaunchKernelGGL(k_cc_label, grid, block, 0, stream, w.parent.p, w.label.p, n_rows, 0, dead, n_rows);
  hipLaunchKernelGGL(k_cr_remap, grid, block, 0, stream, (const int32_t *)w.parent.p, dead, rank, n_rows, w.label.p);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  *launches += 2;
  w.dirty = true;
  return hipSuccess;
}

// ... and what cr_remap wrote becomes parent[0, live_rows) of a structure that was reset meanwhile; the unions word is the one
// cr_remap left (a renumbering takes no union away: marked rows hold none)
inline hipError_t cr_install(CcWork &w, hipStream_t stream, int64_t live_rows) {
  if ((size_t)live_rows > w.parent.cap || (size_t)live_rows > w.label.cap) return hipErrorInvalidValue;  // (cannot happen: a compaction shrinks)
  if (live_rows > 0) {
    const hipError_t e = hipMemcpyAsync(w.parent.p, w.label.p, (size_t)live_rows * sizeof(int32_t), hipMemcpyDeviceToDevice, stream);
    if (e != hipSuccess) return e;
  }
  w.rows = live_rows;
  w.zero_unions = false;
  w.dirty = true;
  return hipSuccess;
}

}  // namespace
}  // namespace apss

#endif  // APSS_COMPONENTS_REPAIR_HPP
