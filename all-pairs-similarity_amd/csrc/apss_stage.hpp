// apss_stage.hpp -- what the list stages behind the join share (apss_topk.hpp, apss_window.hpp, apss_remove.hpp,
// apss_query_stored.hpp, apss_top_pairs.hpp): three device helpers, a stage's device memory and event pair, and the
// "record, launch, record, read a few words, wait, elapsed" sequence every stage times itself with.
#ifndef APSS_STAGE_HPP
#define APSS_STAGE_HPP

#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>

namespace apss {
namespace {

// first position of `key` in the ascending list ids[0, n), or -1 (n > 0; lo_id, hi_id: the list's first and last id)
__device__ inline int64_t sorted_find(const int64_t *__restrict__ ids, int64_t n, int64_t lo_id, int64_t hi_id, int64_t key) {
  if (key < lo_id || key > hi_id) return -1;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (ids[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && ids[lo] == key ? lo : -1;
}

// the external ids of slots r and r + 1 (r even, ext 16-B aligned) with one 16-B load; `two` false: slot r alone, e1 = 0
__device__ inline void load_two_ids(const int64_t *__restrict__ ext, int64_t r, bool two, int64_t &e0, int64_t &e1) {
  e1 = 0;
  if (two) {
    const longlong2 v = *reinterpret_cast<const longlong2 *>(ext + r);
    e0 = v.x;
    e1 = v.y;
  } else {
    e0 = ext[r];
  }
}

// the sum of v over the 64 lanes of the wave, in every lane (xor butterfly)
template <class T>
__device__ inline T wave_sum(T v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// ---- host side
// A stage's device buffers are its own: what they hold in bytes, and the event pair its launches are timed with
struct StageMem {
  size_t bytes = 0;  // device bytes reserved
  hipEvent_t e0 = nullptr, e1 = nullptr;

  // p[old_n] becomes p[n], contents dropped.  (hipFree synchronises; a stage runs after the call's other work, nothing reads
  // its buffers then)
  template <class T>
  hipError_t grow(T *&p, size_t old_n, size_t n) {
    if (p) {
      (void)hipFree(p);
      p = nullptr;
      bytes -= old_n * sizeof(T);
    }
    const hipError_t e = hipMalloc((void **)&p, n * sizeof(T));
    if (e == hipSuccess) bytes += n * sizeof(T);
    return e;
  }
  void free_all(std::initializer_list<void *> ptrs) {
    for (void *p : ptrs)
      if (p) (void)hipFree(p);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    *this = StageMem{};
  }
};

// The timed stretch of a stage: begin_timed, the launches, end_timed_read.  Both create a missing event on first use.
inline hipError_t begin_timed(hipStream_t stream, hipEvent_t &e0) {
  hipError_t e;
  if (!e0 && (e = hipEventCreate(&e0)) != hipSuccess) return e;
  return hipEventRecord(e0, stream);
}

// ... ends the stretch, copies the stage's few words to the host (a read of 0 bytes is skipped) and waits for the stream: ONE
// synchronisation.  *ms: what the stretch took on the device
struct StageRead {
  void *host_dst;
  const void *dev_src;
  size_t bytes;
};
inline hipError_t end_timed_read(hipStream_t stream, hipEvent_t e0, hipEvent_t &e1, std::initializer_list<StageRead> reads, float *ms) {
  hipError_t e;
  if (!e1 && (e = hipEventCreate(&e1)) != hipSuccess) return e;
  if ((e = hipEventRecord(e1, stream)) != hipSuccess) return e;
  for (const StageRead &r : reads)
    if (r.bytes && (e = hipMemcpyAsync(r.host_dst, r.dev_src, r.bytes, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
  return hipEventElapsedTime(ms, e0, e1);
}

}  // namespace
}  // namespace apss

#endif  // APSS_STAGE_HPP
