// apss_components.hpp -- near-duplicate groups: the connected components of the join, kept on the device (include/apss.h:
// apss_set_components).  gfx950, wave64.
//
// The graph: stored slot - stored slot, an edge for every pair of a query-type call's final list.  It is held as a union-find
// forest parent[rows] that every call's list is hooked into where it lies; the labels (label[slot] = smallest slot of the
// component) are made from it when somebody asks.
//
//   k_cc_init     parent[r] = r for the slots [r0, r1) that have no word yet: the rows an insert stored, or all of them after a
//                 reset.  Ordinary stores; nothing else runs on the structure meanwhile (one stream).
//   k_cc_hook     grid-stride over the list, a pair per lane: u = the query row's slot, v = the candidate's slot.  Pairs whose two
//                 parents already agree leave after two loads (most pairs of a stream, once its groups exist).  The others find
//                 both roots and link the larger under the smaller with a device-scope compare-and-swap; one that fails goes on
//                 from the value it returned (apss_components_core.hpp: cc_link).  Links that joined two components are counted
//                 per wave (ballot, popcount) with one add.
//
//                 What the kernel rests on (MI355X: a load may be served from an XCD's own L2, which another XCD's write does
//                 not refresh; a device-scope atomic executes at the memory side).  The core header's invariants I1 .. I5:
//                 parent[x] <= x always; parent[x] is in x's component; a root changes only by that compare-and-swap; EVERY
//                 read of parent[] in this kernel is a relaxed agent-scope atomic load; path shortening writes only an ancestor,
//                 with atomicMin, never a plain store.  Under these a stale read can only cost steps or a retry -- every value
//                 parent[x] ever held is still an ancestor of x -- and the root a component ends with is its smallest slot.
//   k_cc_label    two modes.  0: every slot walks to its root, halving the path with atomicMin as it goes, and ends right under
//                 it; its word of label[] is zeroed for the count.  (No link runs meanwhile: roots are fixed, and a reversed path
//                 of n edges costs what sequential path halving costs, O(log n) amortised per slot, not n per slot.)
//                 1: label[x] = parent[x], or -1 for a row marked removed.
//   k_cc_count    between the two, in label[] as its scratch.  Phase 0: every slot that is no root adds one to its root's word --
//                 equal roots inside a wave are merged first (ballot per distinct value), and a wave carries a run of one root
//                 across its chunks, so ONE giant component costs one add per wave, not one per slot.  Phase 1: the live roots
//                 give components, singletons and the largest size: sums per wave, per workgroup, one add / max each.
//   k_cc_rep      apss_components_fetch: the external id of every slot's labelled slot (its own for a removed row).
//
// No kernel reads the list or the store's rows; memory: parent and label, 4 B each per slot of capacity.
#ifndef APSS_COMPONENTS_HPP
#define APSS_COMPONENTS_HPP

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "apss_components_core.hpp"
#include "apss_stage.hpp"

namespace apss {
namespace {

constexpr int kCcThreads = 256;
constexpr int kCcWave = 64;
constexpr int64_t kCcGridCap = 2048;  // workgroups of the grid-stride kernels (APSS_DEBUG=cc_grid=N: N, for k_cc_hook)
constexpr int kCcWords = 4;           // unions since the last reset | components, singletons, largest of the last labelling

// the device's accesses: relaxed, agent scope (global_load / global_atomic_* with sc1: served behind the CU's L1)
struct CcDevAtomics {
  __device__ static int32_t load(const int32_t *p) {
    return __hip_atomic_load(const_cast<int32_t *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ static int32_t cas(int32_t *p, int32_t expected, int32_t want) {
    __hip_atomic_compare_exchange_strong(p, &expected, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expected;
  }
  __device__ static void fetch_min(int32_t *p, int32_t v) { (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

__global__ __launch_bounds__(kCcThreads) void k_cc_init(int32_t *__restrict__ parent, int64_t r0, int64_t r1) {
  for (int64_t r = r0 + (int64_t)blockIdx.x * kCcThreads + threadIdx.x; r < r1; r += (int64_t)gridDim.x * kCcThreads) parent[r] = (int32_t)r;
}

struct CcHookArgs {
  const int32_t *q, *c;        // the list: query row, candidate slot
  int64_t n;
  int64_t q_slot_first;        // the batch is the stored rows from this slot on, or (< 0) ...
  const int32_t *q_slots;      // ... [nq] the slot of every batch row
  int64_t nq;
  int64_t rows;                // slots of parent[]
  int32_t *parent;
  unsigned long long *unions;  // [1]
};

__global__ __launch_bounds__(kCcThreads) void k_cc_hook(const CcHookArgs a) {
  const int lane = threadIdx.x % kCcWave;
  const int64_t wave = ((int64_t)blockIdx.x * kCcThreads + threadIdx.x) / kCcWave;
  const int64_t n_waves = (int64_t)gridDim.x * (kCcThreads / kCcWave);
  unsigned int joined_wave = 0;
  for (int64_t base = wave * kCcWave; base < a.n; base += n_waves * kCcWave) {  // (wave-uniform: every lane takes part in the ballot)
    const int64_t i = base + lane;
    bool joined = false;
    if (i < a.n) {
      const int64_t qr = a.q[i];
      int64_t u = -1;
      if (qr >= 0 && qr < a.nq) u = a.q_slot_first >= 0 ? a.q_slot_first + qr : (int64_t)a.q_slots[qr];
      const int64_t v = a.c[i];
      // (a slot outside the structure cannot come out of a join over this store; nothing is written for one)
      if (u >= 0 && u < a.rows && v >= 0 && v < a.rows && u != v && !cc_same_parent<CcDevAtomics>(a.parent, (int32_t)u, (int32_t)v))
        joined = cc_link<CcDevAtomics>(a.parent, (int32_t)u, (int32_t)v);
    }
    joined_wave += (unsigned int)__popcll(__ballot(joined));
  }
  if (lane == 0 && joined_wave) atomicAdd(a.unions, (unsigned long long)joined_wave);
}

__device__ inline bool cc_dead(const uint8_t *__restrict__ dead, int64_t dead_rows, int64_t x) { return x < dead_rows && dead[x]; }

// mode 0: flatten (every slot right under its root), label[x] = 0.  mode 1: label[x] = the root | -1 for a marked row
__global__ __launch_bounds__(kCcThreads) void k_cc_label(int32_t *__restrict__ parent, int32_t *__restrict__ label, int64_t rows, int mode,
                                                         const uint8_t *__restrict__ dead, int64_t dead_rows) {
  for (int64_t x = (int64_t)blockIdx.x * kCcThreads + threadIdx.x; x < rows; x += (int64_t)gridDim.x * kCcThreads) {
    if (mode == 0) {
      (void)cc_root_flat<CcDevAtomics>(parent, (int32_t)x);
      label[x] = 0;
    } else {
      label[x] = cc_dead(dead, dead_rows, x) ? -1 : parent[x];
    }
  }
}

template <class T>
__device__ inline T cc_wave_max(T v) {
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
  return v;
}

// parent[] is flat (k_cc_label mode 0), size[] = label[] zeroed.  phase 0: size[root] += the slots under it.  phase 1: words[1 .. 3]
// += / max= over the live roots (zero before the launch)
__global__ __launch_bounds__(kCcThreads) void k_cc_count(const int32_t *__restrict__ parent, int32_t *__restrict__ size, int64_t rows, int phase,
                                                         const uint8_t *__restrict__ dead, int64_t dead_rows, unsigned long long *__restrict__ words) {
  const int lane = threadIdx.x % kCcWave;
  if (phase == 0) {
    const int64_t wave = ((int64_t)blockIdx.x * kCcThreads + threadIdx.x) / kCcWave;
    const int64_t n_waves = (int64_t)gridDim.x * (kCcThreads / kCcWave);
    int32_t run_root = -1;  // (wave-uniform) the root whose adds this wave still holds
    int32_t run_n = 0;
    for (int64_t base = wave * kCcWave; base < rows; base += n_waves * kCcWave) {
      const int64_t x = base + lane;
      const int32_t r = x < rows ? parent[x] : -1;
      bool open = x < rows && r != (int32_t)x;
      for (unsigned long long left = __ballot(open); left; left = __ballot(open)) {
        const int32_t rr = __shfl(r, __ffsll((long long)left) - 1);
        const bool mine = open && r == rr;
        const int32_t cnt = __popcll(__ballot(mine));
        if (rr == run_root) {
          run_n += cnt;
        } else {
          if (lane == 0 && run_n) atomicAdd(size + run_root, run_n);
          run_root = rr;
          run_n = cnt;
        }
        open = open && !mine;
      }
    }
    if (lane == 0 && run_n) atomicAdd(size + run_root, run_n);
    return;
  }
  __shared__ unsigned int part[3][kCcThreads / kCcWave];
  unsigned int comps = 0, singles = 0, largest = 0;
  for (int64_t x = (int64_t)blockIdx.x * kCcThreads + threadIdx.x; x < rows; x += (int64_t)gridDim.x * kCcThreads) {
    if (parent[x] != (int32_t)x || cc_dead(dead, dead_rows, x)) continue;
    const unsigned int sz = (unsigned int)size[x] + 1u;
    ++comps;
    singles += sz == 1u;
    largest = max(largest, sz);
  }
  comps = wave_sum(comps);
  singles = wave_sum(singles);
  largest = cc_wave_max(largest);
  if (lane == 0) {
    part[0][threadIdx.x / kCcWave] = comps;
    part[1][threadIdx.x / kCcWave] = singles;
    part[2][threadIdx.x / kCcWave] = largest;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned int c = 0, s = 0, l = 0;
    for (int w = 0; w < kCcThreads / kCcWave; ++w) {
      c += part[0][w];
      s += part[1][w];
      l = max(l, part[2][w]);
    }
    if (c) atomicAdd(words + 1, (unsigned long long)c);
    if (s) atomicAdd(words + 2, (unsigned long long)s);
    if (l) atomicMax(words + 3, (unsigned long long)l);
  }
}

// rep[i] = the external id of slot (offset + i)'s labelled slot, its own for a removed row
__global__ __launch_bounds__(kCcThreads) void k_cc_rep(const int32_t *__restrict__ label, const int64_t *__restrict__ ext, int64_t offset, int64_t count,
                                                       int64_t rows, int64_t *__restrict__ rep) {
  for (int64_t i = (int64_t)blockIdx.x * kCcThreads + threadIdx.x; i < count; i += (int64_t)gridDim.x * kCcThreads) {
    const int64_t x = offset + i;
    const int64_t l = label[x];
    rep[i] = ext[l >= 0 && l < rows ? l : x];
  }
}

// ---- host side
struct CcWork {
  StageMem mem;                           // parent, label, words; its event pair times the labelling
  DevEvent h0, h1;                        // ... and this one the hooks of a call (made where first recorded: begin_timed)
  DevBuf<int32_t> parent, label;
  DevBuf<unsigned long long> words;       // [kCcWords]
  int64_t rows = 0;                       // parent[0, rows) is initialised: the rest of the store waits for k_cc_init
  bool zero_unions = true;                // words[0] is to be zeroed before it is next added to
  bool dirty = true;                      // label and the counts are older than parent
  bool hook_open = false;                 // h0 / h1 hold a stretch whose time nobody has read yet
};

// every slot a singleton again, no union counted: nothing is launched here (cc_extend does it when the structure is next used)
inline void cc_reset(CcWork &w) {
  w.rows = 0;
  w.zero_unions = true;
  w.dirty = true;
}

inline unsigned cc_grid(int64_t items, int64_t cap) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + kCcThreads - 1) / kCcThreads, cap)); }

// parent[] covers and is initialised for the slots [0, n_rows): room (grown by half, the initialised words kept), then k_cc_init
// over the slots that have none -- the new rows of an insert, never the store
inline hipError_t cc_extend(CcWork &w, hipStream_t stream, int64_t n_rows, int32_t *launches) {
  hipError_t e;
  if (!w.words.p && (e = w.mem.grow((size_t)kCcWords, w.words)) != hipSuccess) return e;
  if ((size_t)n_rows > w.label.cap) {  // (label grows last: a call that failed half way comes back here, parent keeps what it holds)
    const size_t cap = std::max<size_t>((size_t)n_rows, w.label.cap + w.label.cap / 2);
    if ((e = w.parent.grow(kGrowStageKeep, cap, (size_t)w.rows, stream, w.mem.ledger)) != hipSuccess) return e;
    if ((e = w.mem.grow(cap, w.label)) != hipSuccess) return e;
    w.dirty = true;
  }
  if (w.zero_unions) {
    if ((e = hipMemsetAsync(w.words.p, 0, kCcWords * sizeof(unsigned long long), stream)) != hipSuccess) return e;
    w.zero_unions = false;
  }
  if (w.rows > n_rows) w.rows = 0;  // (cannot happen: a store shrinks only through a reset)
  if (w.rows < n_rows) {
    hipLaunchKernelGGL(k_cc_init, dim3(cc_grid(n_rows - w.rows, kCcGridCap)), dim3(kCcThreads), 0, stream, w.parent.p, w.rows, n_rows);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (launches) ++*launches;
    w.rows = n_rows;
    w.dirty = true;
  }
  return hipSuccess;
}

// the time of the stretch h0 .. h1 (the stream has been waited for), added to *ms
inline void cc_take_hook_time(CcWork &w, double *ms) {
  if (!w.hook_open) return;
  float t = 0.f;
  if (hipEventElapsedTime(&t, w.h0, w.h1) == hipSuccess) *ms += t;
  w.hook_open = false;
}

// One list into the forest.  Launches on `stream`, reads nothing back, waits for nothing.  (A windowed call hooks once per window,
// and every window's cut has waited for the stream by the time the next one hooks: the finished stretch's time is taken then,
// without a wait of the stage's own.  A stretch that is still running is simply extended.)
inline hipError_t cc_hook(CcWork &w, hipStream_t stream, const int32_t *q, const int32_t *c, int64_t n, int64_t q_slot_first, const int32_t *q_slots,
                          int64_t nq, int64_t n_rows, int64_t grid_cap, int32_t *launches, double *ms) {
  hipError_t e;
  if ((e = cc_extend(w, stream, n_rows, nullptr)) != hipSuccess) return e;
  if (w.hook_open) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, w.h0, w.h1) == hipSuccess) {
      *ms += t;
      w.hook_open = false;
    } else {
      (void)hipGetLastError();  // (not ready: no error of this call's)
    }
  }
  if (!w.hook_open && (e = begin_timed(stream, w.h0)) != hipSuccess) return e;
  CcHookArgs a{};
  a.q = q;
  a.c = c;
  a.n = n;
  a.q_slot_first = q_slot_first;
  a.q_slots = q_slots;
  a.nq = nq;
  a.rows = n_rows;
  a.parent = w.parent.p;
  a.unions = w.words.p;
  hipLaunchKernelGGL(k_cc_hook, dim3(cc_grid(n, grid_cap)), dim3(kCcThreads), 0, stream, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  ++*launches;
  w.dirty = true;
  if ((e = begin_timed(stream, w.h1)) != hipSuccess) return e;  // (records h1, made at its first use)
  w.hook_open = true;
  return hipSuccess;
}

// label[0, n_rows) and the four words, from parent[]: flatten, count in label[], write the labels.  ONE synchronisation.
// host[kCcWords]: where the words land
inline hipError_t cc_label(CcWork &w, hipStream_t stream, int64_t n_rows, const uint8_t *dead, int64_t dead_rows, unsigned long long *host,
                           int32_t *launches, double *label_ms, double *hook_ms) {
  hipError_t e;
  *launches = 0;
  if ((e = cc_extend(w, stream, n_rows, nullptr)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(w.words.p + 1, 0, (kCcWords - 1) * sizeof(unsigned long long), stream)) != hipSuccess) return e;
  if ((e = begin_timed(stream, w.mem.e0)) != hipSuccess) return e;
  if (n_rows > 0) {
    const dim3 grid(cc_grid(n_rows, kCcGridCap)), block(kCcThreads);
    hipLaunchKernelGGL(k_cc_label, grid, block, 0, stream, w.parent.p, w.label.p, n_rows, 0, dead, dead_rows);
    hipLaunchKernelGGL(k_cc_count, grid, block, 0, stream, (const int32_t *)w.parent.p, w.label.p, n_rows, 0, dead, dead_rows, w.words.p);
    hipLaunchKernelGGL(k_cc_count, grid, block, 0, stream, (const int32_t *)w.parent.p, w.label.p, n_rows, 1, dead, dead_rows, w.words.p);
    hipLaunchKernelGGL(k_cc_label, grid, block, 0, stream, w.parent.p, w.label.p, n_rows, 1, dead, dead_rows);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    *launches = 4;
  }
  float ms = 0.f;
  if ((e = end_timed_read(stream, w.mem.e0, w.mem.e1, {{host, w.words.p, kCcWords * sizeof(unsigned long long)}}, &ms)) != hipSuccess) return e;
  *label_ms = ms;
  cc_take_hook_time(w, hook_ms);  // (the stream has been waited for: the call's hooks are over)
  w.dirty = false;
  return hipSuccess;
}

}  // namespace
}  // namespace apss

#endif  // APSS_COMPONENTS_HPP
