// apss_owned.hpp -- who owns what the library reserves: a device array, an event, a pinned host block and a stream, each freed by
// its destructor.  Written over a back-end policy B (the way apss_components_core.hpp is written over its atomics): the library
// gives it HIP (HipBackend in apss_stage.hpp, which shows what a B has), host/owned_selftest.cpp a counting fake.  No HIP header
// here: plain C++.
#ifndef APSS_OWNED_HPP
#define APSS_OWNED_HPP

#include <algorithm>
#include <cstddef>
#include <utility>

namespace apss {

// ---- how an array grows.  The orders differ in peak memory (both blocks live, or never), so they stay apart:
//   kAllocCopyWaitFree  the new block first, `keep` elements copied on the stream, the stream waited for, the old block freed; a
//                       failure in any step frees the new block and leaves the array and its ledger as they were
//   kWaitFreeAlloc      the stream waited for, the old block freed, then the new one: contents dropped, a failed allocation
//                       leaves the array empty
//   kFreeAlloc          the same without the wait (nothing on the device reads the array any more; the free synchronises)
enum class GrowOrder { kAllocCopyWaitFree, kWaitFreeAlloc, kFreeAlloc };
struct GrowPolicy {
  size_t floor;   // least capacity (elements)
  bool headroom;  // capacity max(n, cap + cap / 2); false: exactly n
  GrowOrder order;
};
constexpr GrowPolicy kGrowHandle{64, true, GrowOrder::kAllocCopyWaitFree};        // a handle's arrays
constexpr GrowPolicy kGrowHandleExact{64, false, GrowOrder::kAllocCopyWaitFree};  // ... whose size the caller knows for good
constexpr GrowPolicy kGrowGroup{256, true, GrowOrder::kWaitFreeAlloc};            // a group's exchange buffers
constexpr GrowPolicy kGrowGroupKeep{256, true, GrowOrder::kAllocCopyWaitFree};    // ... and the lists it appends to
constexpr GrowPolicy kGrowStage{0, false, GrowOrder::kFreeAlloc};                 // a list stage's arrays, sized by the stage
constexpr GrowPolicy kGrowStageKeep{0, false, GrowOrder::kAllocCopyWaitFree};     // ... and the one that keeps its contents

// ---- a device array of `cap` elements at `p`.  Move-only; a moved-from array is empty.  It remembers the ledger (a byte count
// somewhere that outlives it, or none) it last grew against, and takes its bytes off it when the block goes
template <class T, class B>
class DevArray {
 public:
  T *p = nullptr;
  size_t cap = 0;

  DevArray() = default;
  DevArray(const DevArray &) = delete;
  DevArray &operator=(const DevArray &) = delete;
  DevArray(DevArray &&o) noexcept { *this = std::move(o); }
  DevArray &operator=(DevArray &&o) noexcept {
    if (this != &o) {
      reset();
      p = std::exchange(o.p, nullptr), cap = std::exchange(o.cap, 0), ledger_ = std::exchange(o.ledger_, nullptr);
    }
    return *this;
  }
  ~DevArray() { reset(); }

  void reset() {
    if (p) B::free(p);
    if (ledger_) *ledger_ -= cap * sizeof(T);
    p = nullptr, cap = 0, ledger_ = nullptr;
  }

  // room for n elements (a request that fits calls nothing).  keep: elements that survive (kAllocCopyWaitFree only)
  typename B::Error grow(const GrowPolicy &pol, size_t n, size_t keep, typename B::Stream stream, size_t *ledger) {
    if (p && n <= cap) return B::ok;
    const size_t ncap = std::max(pol.headroom ? std::max(n, cap + cap / 2) : n, pol.floor);
    const bool alloc_first = pol.order == GrowOrder::kAllocCopyWaitFree;
    typename B::Error e = B::ok;
    if (p && !alloc_first) {
      if (pol.order == GrowOrder::kWaitFreeAlloc && (e = B::wait(stream)) != B::ok) return e;
      reset();
    }
    void *np = nullptr;
    if ((e = B::alloc(&np, ncap * sizeof(T))) != B::ok) return e;
    if (p) {  // (the new block came first)
      if (keep) e = B::copy(np, p, keep * sizeof(T), stream);
      if (e == B::ok) e = B::wait(stream);
      if (e != B::ok) {
        B::free(np);
        return e;
      }
      reset();
    }
    p = static_cast<T *>(np);
    cap = ncap;
    ledger_ = ledger;
    if (ledger_) *ledger_ += cap * sizeof(T);
    return B::ok;
  }

 private:
  size_t *ledger_ = nullptr;
};

// every array of the list to n elements under one policy; the first failure ends it
template <class T, class B, class... A>
typename B::Error grow_all(const GrowPolicy &pol, size_t n, size_t keep, typename B::Stream stream, size_t *ledger, DevArray<T, B> &first, A &...rest) {
  typename B::Error e = first.grow(pol, n, keep, stream, ledger);
  (void)((e == B::ok) && ... && ((e = rest.grow(pol, n, keep, stream, ledger)) == B::ok));
  return e;
}

// ---- a pinned host block: the same array over the back-end's host side (kGrowStage: exactly n, the old block freed first)
template <class B>
struct HostSide : B {
  static typename B::Error alloc(void **p, size_t bytes) { return B::host_alloc(p, bytes); }
  static void free(void *p) { B::host_free(p); }
};
template <class T, class B>
using PinnedArray = DevArray<T, HostSide<B>>;

// ---- a back-end handle (an event, a stream) that is dropped once if it was ever made.  Move-only (a group's members live in a
// vector); assigning an empty one drops it
template <class H, void (*Drop)(H)>
class OwnedHandle {
 public:
  OwnedHandle() = default;
  OwnedHandle(const OwnedHandle &) = delete;
  OwnedHandle &operator=(const OwnedHandle &) = delete;
  OwnedHandle(OwnedHandle &&o) noexcept : h_(o.h_), made_(o.made_) { o.made_ = false; }
  OwnedHandle &operator=(OwnedHandle &&o) noexcept {
    if (this != &o) {
      if (made_) Drop(h_);
      h_ = o.h_, made_ = o.made_;
      o.made_ = false;
    }
    return *this;
  }
  ~OwnedHandle() {
    if (made_) Drop(h_);
  }
  bool made() const { return made_; }
  operator H() const { return made_ ? h_ : H{}; }  // (for the calls that wait on it, read its time or run on it)

 protected:
  H h_{};
  bool made_ = false;
};

// an event, made where it is first recorded (with timing, or kUntimed)
constexpr bool kUntimed = false;
template <class B>
class OwnedEvent : public OwnedHandle<typename B::Event, &B::event_drop> {
 public:
  OwnedEvent() = default;
  explicit OwnedEvent(bool timing) : timing_(timing) {}
  typename B::Error record(typename B::Stream stream) {
    if (!this->made_) {
      const typename B::Error e = B::event_make(&this->h_, timing_);
      if (e != B::ok) return e;
      this->made_ = true;
    }
    return B::event_record(this->h_, stream);
  }

 private:
  bool timing_ = true;
};

template <class B>
class OwnedStream : public OwnedHandle<typename B::Stream, &B::stream_drop> {
 public:
  typename B::Error make() {
    if (this->made_) return B::ok;
    const typename B::Error e = B::stream_make(&this->h_);
    this->made_ = e == B::ok;
    return e;
  }
};

}  // namespace apss

#endif  // APSS_OWNED_HPP
