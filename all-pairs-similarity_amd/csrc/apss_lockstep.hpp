// apss_lockstep.hpp -- how the member threads of one group call stay in step (apss_group.hip): a reusable barrier, the rule
// "a member publishes its failure BEFORE the next barrier, and every thread acts on the flag AS THAT BARRIER RETURNED IT" as one
// function (Lockstep::step), the start / join of the member threads with the report of the first failed member, and the
// arithmetic of the exchange's offsets.  The rule is what keeps T threads from deadlocking and a collective from being entered
// by some members and not by others.  No HIP header here: plain C++ (host/lockstep_selftest.cpp runs it under the sanitizers).
#ifndef APSS_LOCKSTEP_HPP
#define APSS_LOCKSTEP_HPP

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace apss {

constexpr int32_t kLockstepOk = 0;  // (= APSS_OK of include/apss.h, which this header does not read)

// ---- a reusable barrier for the member threads of one call (C++17: no std::barrier).  wait() returns the call's failure flag
// as the LAST thread to arrive read it, under the mutex: every thread of one generation takes the same go / no-go decision,
// even when a thread that already left fails (and sets the flag) before a slower one has woken up.
class Barrier {
 public:
  Barrier(int n, const std::atomic<int> *failed) : n_(n), failed_(failed) {}
  bool wait() {
    std::unique_lock<std::mutex> lk(mu_);
    const uint64_t gen = gen_;
    if (++count_ == n_) {
      count_ = 0;
      snap_ = failed_->load() != 0;
      ++gen_;
      cv_.notify_all();
    } else {
      cv_.wait(lk, [&] { return gen_ != gen; });
    }
    return snap_;  // (the next generation cannot overwrite it before this thread arrives there)
  }

 private:
  std::mutex mu_;
  std::condition_variable cv_;
  int n_, count_ = 0;
  uint64_t gen_ = 0;
  const std::atomic<int> *failed_;
  bool snap_ = false;
};

// ---- one member thread's handle on the rule.  It holds the barrier of the member's row range (or of the re-layout), the
// call's failure flag -- ONE for all the threads of a call, however many barriers they are spread over -- and where this
// member's result code goes.  Work is a callable that returns int32_t (kLockstepOk, or the member's error code).
enum class When {
  kAlways,        // the work runs whatever the flag says (a pack, a union, a reduction: the peers count on its side effects)
  kUnlessFailed,  // the work is skipped when the call has already failed (a handle call: nobody will use its answer)
};

class Lockstep {
 public:
  Lockstep(Barrier *bar, std::atomic<int> *failed, int32_t *rc) : bar_(bar), failed_(failed), rc_(rc) {}

  // work whose failure rides to the next step's barrier: published at once, acted on there
  template <class F>
  void run(When when, F &&work) {
    if (when == When::kUnlessFailed && failed_->load()) return;
    const int32_t rc = work();
    if (rc != kLockstepOk) {
      *rc_ = rc;
      failed_->store(1);
    }
  }

  // THE RULE: run the work, publish a failure, wait at the barrier; true: the call goes on -- the same answer on every thread of
  // this barrier, because it is the barrier's snapshot of the flag and not this thread's own look at it
  template <class F>
  bool step(When when, F &&work) {
    run(when, std::forward<F>(work));
    return !bar_->wait();
  }

 private:
  Barrier *bar_;
  std::atomic<int> *failed_;
  int32_t *rc_;
};

// ---- fn(m, ctx) for m = 1 .. n - 1 on threads of their own and m = 0 on the caller's; returns when all of them have
template <class Ctx>
void run_members(int n, void (*fn)(int, Ctx *), Ctx *ctx) {
  std::vector<std::thread> th;
  for (int m = 1; m < n; ++m) th.emplace_back(fn, m, ctx);
  fn(0, ctx);
  for (std::thread &t : th) t.join();
}

// what a failed call reports: the lowest-numbered member whose result code is not OK, as "member N: <its message>"; when no
// member holds one (the flag was up all the same), the caller's own code and message
struct MemberFailure {
  int32_t rc;
  std::string msg;
};
template <class RcOf, class ErrOf>
MemberFailure first_failure(int n, RcOf rc_of, ErrOf err_of, int32_t fallback_rc, const char *fallback_msg) {
  for (int m = 0; m < n; ++m)
    if (rc_of(m) != kLockstepOk) return MemberFailure{rc_of(m), "member " + std::to_string(m) + ": " + err_of(m)};
  return MemberFailure{fallback_rc, fallback_msg};
}

// ---- the exchange's offsets: member k's candidate list sits at off[k] of the one buffer every member holds (off[T] = total);
// `least` is the shortest list (the all-gather moves 8 * (total - least) bytes to the member that receives the most)
struct ExchangeOffsets {
  std::vector<int64_t> off;
  int64_t total = 0, mine = 0, least = INT64_MAX;
};
template <class CountOf>
ExchangeOffsets exchange_offsets(int T, int me, CountOf count_of) {
  ExchangeOffsets x;
  x.off.assign((size_t)T + 1, 0);
  for (int k = 0; k < T; ++k) {
    const int64_t nk = count_of(k);
    if (k == me) x.mine = x.total;
    x.off[(size_t)k] = x.total;
    x.total += nk;
    x.least = std::min(x.least, nk);
  }
  x.off[(size_t)T] = x.total;
  return x;
}

// significant bits of a candidate's key: 32 of the slot + the bits of a query row of a batch of n rows (the smallest b in
// [1, 31] with 2^b >= max(2, n))
inline int exchange_key_bits(int64_t n) {
  int q_bits = 1;
  while (q_bits < 31 && (1LL << q_bits) < std::max<int64_t>(2, n)) ++q_bits;
  return 32 + q_bits;
}

}  // namespace apss

#endif  // APSS_LOCKSTEP_HPP
