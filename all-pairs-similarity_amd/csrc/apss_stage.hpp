// apss_stage.hpp -- what the list stages behind the join share (apss_topk.hpp, apss_window.hpp, apss_remove.hpp,
// apss_query_stored.hpp, apss_top_pairs.hpp): three device helpers, a stage's device memory and event pair, and the
// "record, launch, record, read a few words, wait, elapsed" sequence every stage times itself with.
#ifndef APSS_STAGE_HPP
#define APSS_STAGE_HPP

#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>

#include "apss_owned.hpp"

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
// The HIP back-end of the owning types (apss_owned.hpp): the one place in the library that reserves or frees device memory, pinned
// memory, events and streams
struct HipBackend {
  using Error = hipError_t;
  using Stream = hipStream_t;
  using Event = hipEvent_t;
  static constexpr Error ok = hipSuccess;
  static Error alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
  static void free(void *p) { (void)hipFree(p); }
  static Error copy(void *dst, const void *src, size_t bytes, Stream s) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s); }
  static Error wait(Stream s) { return hipStreamSynchronize(s); }
  static Error host_alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void host_free(void *p) { (void)hipHostFree(p); }
  static Error event_make(Event *e, bool timing) { return timing ? hipEventCreate(e) : hipEventCreateWithFlags(e, hipEventDisableTiming); }
  static Error event_record(Event e, Stream s) { return hipEventRecord(e, s); }
  static void event_drop(Event e) { (void)hipEventDestroy(e); }
  static Error stream_make(Stream *s) { return hipStreamCreateWithFlags(s, hipStreamDefault); }
  static void stream_drop(Stream s) { (void)hipStreamDestroy(s); }
};
template <class T>
using DevBuf = DevArray<T, HipBackend>;
using DevEvent = OwnedEvent<HipBackend>;
template <class T>
using PinBuf = PinnedArray<T, HipBackend>;
using DevStream = OwnedStream<HipBackend>;

// A stage's arrays are its own members (sized by the stage: kGrowStage); what it shares is the ledger they are counted in (a
// handle's reservation, set by run_stage; none for a group) and the event pair its launches are timed with
struct StageMem {
  size_t *ledger = nullptr;
  DevEvent e0, e1;

  // every b becomes b[n], contents dropped; the first failure ends it.  (The free synchronises; a stage runs after the call's other
  // work, nothing reads its buffers then)
  template <class... A>
  hipError_t grow(size_t n, A &...b) {
    return grow_all(kGrowStage, n, 0, nullptr, ledger, b...);
  }
};

// The timed stretch of a stage: begin_timed, the launches, end_timed_read.  Both make a missing event on first use.
inline hipError_t begin_timed(hipStream_t stream, DevEvent &e0) { return e0.record(stream); }

// ... ends the stretch, copies the stage's few words to the host (a read of 0 bytes is skipped) and waits for the stream: ONE
// synchronisation.  *ms: what the stretch took on the device
struct StageRead {
  void *host_dst;
  const void *dev_src;
  size_t bytes;
};
inline hipError_t end_timed_read(hipStream_t stream, const DevEvent &e0, DevEvent &e1, std::initializer_list<StageRead> reads, float *ms) {
  hipError_t e;
  if ((e = e1.record(stream)) != hipSuccess) return e;
  for (const StageRead &r : reads)
    if (r.bytes && (e = hipMemcpyAsync(r.host_dst, r.dev_src, r.bytes, hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
  return hipEventElapsedTime(ms, e0, e1);
}

}  // namespace
}  // namespace apss

#endif  // APSS_STAGE_HPP
