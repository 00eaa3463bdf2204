// lockstep_selftest.cpp -- the lock-step rule of the group's member threads (csrc/apss_lockstep.hpp) in plain C++, with real
// threads: a failure injected at every (thread, step) of a script, two failures in one step, the "skip if the call has already
// failed" steps, one barrier reused over 12,000 generations while the flag changes behind the threads' backs, two groups of
// threads on one flag (a grid's row ranges), run_members' join, and the exchange's offsets and key width against literal
// tables.  No GPU, no HIP header.  Build: see Makefile in this directory (tests/test_lockstep_host.py builds it under
// -fsanitize=address,undefined and under -fsanitize=thread and runs both).
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <string>
#include <thread>
#include <vector>

#include "../csrc/apss_lockstep.hpp"

using apss::Barrier;
using apss::Lockstep;
using apss::When;

static std::atomic<int> fails{0};
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                \
    }                                                         \
  } while (0)

// a thread's own cheap random numbers (where it yields, what it stores)
struct Lcg {
  uint64_t s;
  uint32_t next() { return (uint32_t)((s = s * 6364136223846793005ULL + 1442695040888963407ULL) >> 33); }
};

// ---- a script of S steps on T threads; fail_step[m] = the step at which thread m fails (-1: never)
constexpr int S = 6;
struct Script {
  int T = 0;
  std::vector<int> fail_step;
  Barrier *bar = nullptr;
  std::atomic<int> failed{0};
  std::vector<int32_t> rc;
  std::vector<std::string> err;
  std::vector<int> left;               // the step after which thread m left (S: it ran the whole script)
  std::vector<std::vector<int>> ran;   // ran[m][s]: how often thread m ran the work of step s
};

static void script_main(int m, Script *sc) {
  Lockstep ls(sc->bar, &sc->failed, &sc->rc[(size_t)m]);
  sc->left[(size_t)m] = S;
  for (int s = 0; s < S; ++s) {
    const bool on = ls.step(When::kAlways, [&]() -> int32_t {
      ++sc->ran[(size_t)m][(size_t)s];
      if (sc->fail_step[(size_t)m] != s) return apss::kLockstepOk;
      sc->err[(size_t)m] = "thread " + std::to_string(m) + " at step " + std::to_string(s);
      return 100 + m;
    });
    if (!on) {
      sc->left[(size_t)m] = s;
      return;
    }
  }
}

static apss::MemberFailure run_script(Script &sc) {
  const size_t T = (size_t)sc.T;
  Barrier bar(sc.T, &sc.failed);
  sc.bar = &bar;
  sc.rc.assign(T, apss::kLockstepOk);
  sc.err.assign(T, "");
  sc.left.assign(T, -1);
  sc.ran.assign(T, std::vector<int>((size_t)S, 0));
  apss::run_members(sc.T, script_main, &sc);
  return apss::first_failure(
      sc.T, [&](int m) { return sc.rc[(size_t)m]; }, [&](int m) -> const std::string & { return sc.err[(size_t)m]; }, -4, "nobody owned up");
}

static void check_script(const Script &sc, int stop) {  // every thread ran steps [0, stop] once and nothing after, and left there
  for (int m = 0; m < sc.T; ++m) {
    CHECK(sc.left[(size_t)m] == stop);
    for (int s = 0; s < S; ++s) CHECK(sc.ran[(size_t)m][(size_t)s] == (s <= stop ? 1 : 0));
  }
}

static void every_injected_failure() {
  for (int T : {1, 2, 3, 8}) {
    {
      Script sc;
      sc.T = T;
      sc.fail_step.assign((size_t)T, -1);
      const apss::MemberFailure f = run_script(sc);
      check_script(sc, S);
      CHECK(sc.failed.load() == 0);
      CHECK(f.rc == -4 && f.msg == "nobody owned up");  // (the fallback: no member holds a code)
    }
    for (int ft = 0; ft < T; ++ft)
      for (int fs = 0; fs < S; ++fs) {
        Script sc;
        sc.T = T;
        sc.fail_step.assign((size_t)T, -1);
        sc.fail_step[(size_t)ft] = fs;
        const apss::MemberFailure f = run_script(sc);
        check_script(sc, fs);
        CHECK(sc.failed.load() == 1);
        CHECK(f.rc == 100 + ft);
        CHECK(f.msg == "member " + std::to_string(ft) + ": thread " + std::to_string(ft) + " at step " + std::to_string(fs));
        for (int m = 0; m < T; ++m) CHECK(sc.rc[(size_t)m] == (m == ft ? 100 + ft : apss::kLockstepOk));
      }
  }
}

static void two_failures_in_one_step() {
  Script sc;
  sc.T = 8;
  sc.fail_step.assign(8, -1);
  sc.fail_step[5] = sc.fail_step[2] = 3;
  const apss::MemberFailure f = run_script(sc);
  check_script(sc, 3);
  CHECK(f.rc == 102 && f.msg == "member 2: thread 2 at step 3");  // the lowest member index
  CHECK(sc.rc[5] == 105);
}

// ---- When::kUnlessFailed skips its work once the flag is up; When::kAlways does not
struct SkipCtx {
  std::atomic<int> failed{0};
  Barrier *bar = nullptr;
  int32_t rc[2] = {0, 0};
  int skipped_ran[2] = {0, 0}, plain_ran[2] = {0, 0}, before_ran[2] = {0, 0};
  bool went_on[2] = {true, true};
};

static void skip_main(int m, SkipCtx *c) {
  Lockstep ls(c->bar, &c->failed, &c->rc[m]);
  // (member 1 fails in the first step; the flag is up on both threads once its barrier has returned)
  const bool on = ls.step(When::kAlways, [&]() -> int32_t {
    ++c->before_ran[m];
    return m == 1 ? 7 : apss::kLockstepOk;
  });
  CHECK(!on);
  // what a member does between two barriers of a failed call: the skipping kind is left out, the plain kind still runs
  ls.run(When::kUnlessFailed, [&]() -> int32_t { return ++c->skipped_ran[m], 9; });
  c->went_on[m] = ls.step(When::kAlways, [&]() -> int32_t { return ++c->plain_ran[m], apss::kLockstepOk; });
}

static void skip_if_already_failed() {
  {  // one thread, no interleaving to think about
    std::atomic<int> failed{0};
    Barrier bar(1, &failed);
    int32_t rc = 0;
    int a = 0, b = 0, c = 0;
    Lockstep ls(&bar, &failed, &rc);
    ls.run(When::kUnlessFailed, [&]() -> int32_t { return ++a, apss::kLockstepOk; });
    CHECK(a == 1 && rc == 0 && failed.load() == 0);
    ls.run(When::kAlways, [&]() -> int32_t { return 5; });
    CHECK(rc == 5 && failed.load() == 1);
    ls.run(When::kUnlessFailed, [&]() -> int32_t { return ++b, 6; });
    CHECK(b == 0 && rc == 5);  // (skipped: the first failure's code stays)
    ls.run(When::kAlways, [&]() -> int32_t { return ++c, apss::kLockstepOk; });
    CHECK(c == 1 && rc == 5);
    CHECK(!ls.step(When::kAlways, [&]() -> int32_t { return ++c, apss::kLockstepOk; }));
    CHECK(c == 2);
    CHECK(!ls.step(When::kUnlessFailed, [&]() -> int32_t { return ++b, 6; }));
    CHECK(b == 0);
  }
  SkipCtx c;
  Barrier bar(2, &c.failed);
  c.bar = &bar;
  apss::run_members(2, skip_main, &c);
  for (int m = 0; m < 2; ++m) {
    CHECK(c.before_ran[m] == 1 && c.skipped_ran[m] == 0 && c.plain_ran[m] == 1 && !c.went_on[m]);
    CHECK(c.rc[m] == (m == 1 ? 7 : 0));
  }
}

// ---- one barrier, many generations.  (a) `toggle`: every thread, having left a generation, now and then stores 0 or 1 into
// the flag -- while slower threads of that generation may not have woken up yet.  Whatever the flag does, the threads of one
// generation must all get the same snapshot.  (b) otherwise: one thread raises the flag right after leaving generation
// `raise_at`: every thread sees "go" up to and including that generation and "no-go" from the next one on.
constexpr int kGenerations = 12000;
struct ReuseCtx {
  int T = 0;
  bool toggle = false;
  int raise_at = -1;
  Barrier *bar = nullptr;
  std::atomic<int> failed{0};
  std::vector<std::vector<char>> seen;  // seen[m][g]
};

static void reuse_main(int m, ReuseCtx *c) {
  Lcg r{0x9e3779b97f4a7c15ULL * (uint64_t)(m + 1)};
  for (int g = 0; g < kGenerations; ++g) {
    if (r.next() % 8 == 0) std::this_thread::yield();
    const bool snap = c->bar->wait();
    c->seen[(size_t)m][(size_t)g] = snap ? 1 : 0;
    if (r.next() % 8 == 0) std::this_thread::yield();
    if (c->toggle) {
      if (r.next() % 16 == 0) c->failed.store((int)(r.next() & 1));
    } else if (g == c->raise_at && m == g % c->T) {
      c->failed.store(1);
    }
  }
}

static void barrier_reuse() {
  for (int T : {2, 3, 8})
    for (int toggle = 0; toggle < 2; ++toggle) {
      ReuseCtx c;
      c.T = T;
      c.toggle = toggle != 0;
      c.raise_at = kGenerations / 2 + T - 1;
      Barrier bar(T, &c.failed);
      c.bar = &bar;
      c.seen.assign((size_t)T, std::vector<char>((size_t)kGenerations, 2));
      apss::run_members(T, reuse_main, &c);
      int64_t ups = 0;
      for (int g = 0; g < kGenerations; ++g) {
        for (int m = 1; m < T; ++m) CHECK(c.seen[(size_t)m][(size_t)g] == c.seen[0][(size_t)g]);
        CHECK(c.seen[0][(size_t)g] != 2);
        if (!toggle) CHECK(c.seen[0][(size_t)g] == (g > c.raise_at ? 1 : 0));
        ups += c.seen[0][(size_t)g] == 1;
      }
      CHECK(ups > 0 && ups < kGenerations);  // (both answers were given)
    }
}

// ---- two groups of threads (two row ranges of a grid), a barrier each, ONE flag.  Range B runs steps until it is stopped;
// a thread of range A fails at step 2, but only after B has gone through several barriers meanwhile -- with A's other threads
// waiting at A's barrier all that time, so B does not wait for A's barrier -- and B stops at its next barrier, all together.
struct GridCtx {
  int Ta = 3, Tb = 2;
  Barrier *bar_a = nullptr, *bar_b = nullptr;
  std::atomic<int> failed{0};
  std::atomic<int64_t> b_steps{0};  // steps of range B's first thread
  int64_t b_steps_at_failure = 0;
  int32_t rc[5] = {0, 0, 0, 0, 0};
  int64_t left[5] = {-1, -1, -1, -1, -1};
};

static void grid_main(int m, GridCtx *c) {
  const bool in_a = m < c->Ta;
  Lockstep ls(in_a ? c->bar_a : c->bar_b, &c->failed, &c->rc[m]);
  for (int64_t s = 0; s < (in_a ? 6 : (int64_t)1 << 40); ++s) {
    const bool on = ls.step(When::kAlways, [&]() -> int32_t {
      if (!in_a) {
        if (m == c->Ta) ++c->b_steps;
        return apss::kLockstepOk;
      }
      if (m != 1 || s != 2) return apss::kLockstepOk;
      while (c->b_steps.load() < 50) std::this_thread::yield();
      c->b_steps_at_failure = c->b_steps.load();
      return 42;
    });
    if (!on) {
      c->left[m] = s;
      return;
    }
  }
}

static void two_groups_one_flag() {
  GridCtx c;
  Barrier bar_a(c.Ta, &c.failed), bar_b(c.Tb, &c.failed);
  c.bar_a = &bar_a;
  c.bar_b = &bar_b;
  apss::run_members(c.Ta + c.Tb, grid_main, &c);
  for (int m = 0; m < c.Ta; ++m) CHECK(c.left[m] == 2);
  CHECK(c.b_steps_at_failure >= 50);
  CHECK(c.left[3] >= 49 && c.left[3] == c.left[4]);  // B stopped, both threads after the same step ...
  CHECK(c.b_steps.load() == c.left[3] + 1);           // ... having run no step's work after it
  const apss::MemberFailure f = apss::first_failure(
      5, [&](int m) { return c.rc[m]; }, [&](int) { return std::string("x"); }, -4, "a member failed");
  CHECK(f.rc == 42 && f.msg == "member 1: x");
}

// ---- run_members joins every thread it started, also when member 0's function returns at once
struct JoinCtx {
  std::atomic<int> done{0};
  int plain_done = 0;  // (written by the last thread only: a thread that was not joined is a race TSan reports)
};

static void join_main(int m, JoinCtx *c) {
  if (m == 0) return;
  std::this_thread::sleep_for(std::chrono::milliseconds(5 * m));
  if (m == 7) c->plain_done = 1;
  ++c->done;
}

static void run_members_joins() {
  JoinCtx c;
  apss::run_members(8, join_main, &c);
  CHECK(c.done.load() == 7 && c.plain_done == 1);
  JoinCtx one;
  apss::run_members(1, join_main, &one);  // (no thread at all)
  CHECK(one.done.load() == 0);
}

// ---- the exchange's offsets and key width, against literal tables
static void check_offsets(const std::vector<int64_t> &counts, int me, const std::vector<int64_t> &off, int64_t mine, int64_t least) {
  const apss::ExchangeOffsets x = apss::exchange_offsets((int)counts.size(), me, [&](int k) { return counts[(size_t)k]; });
  CHECK(x.off == off);
  CHECK(x.total == off.back());
  CHECK(x.mine == mine);
  CHECK(x.least == least);
}

static void offsets_and_key_width() {
  check_offsets({0, 0, 0}, 1, {0, 0, 0, 0}, 0, 0);                    // nothing to exchange
  check_offsets({5, 0, 7, 1}, 0, {0, 5, 5, 12, 13}, 0, 0);            // one empty member among the others
  check_offsets({5, 0, 7, 1}, 1, {0, 5, 5, 12, 13}, 5, 0);            // (the empty member's own offset)
  check_offsets({5, 0, 7, 1}, 2, {0, 5, 5, 12, 13}, 5, 0);
  check_offsets({5, 0, 7, 1}, 3, {0, 5, 5, 12, 13}, 12, 0);
  check_offsets({3, 9, 4}, 2, {0, 3, 12, 16}, 12, 3);
  check_offsets({11}, 0, {0, 11}, 0, 11);                             // T = 1
  check_offsets({0}, 0, {0, 0}, 0, 0);
  const int64_t big = 2147483647;                                     // counts near 2^31: the sums need 64 bits
  check_offsets({big, big - 1, big, 2147483648LL}, 3, {0, big, 2 * big - 1, 3 * big - 1, 3 * big - 1 + 2147483648LL}, 3 * big - 1, big - 1);
  CHECK(3 * big - 1 + 2147483648LL == 8589934588LL);
  // 32 bits of the candidate slot + the smallest b in [1, 31] with 2^b >= max(2, n)
  CHECK(apss::exchange_key_bits(0) == 33);
  CHECK(apss::exchange_key_bits(1) == 33);
  CHECK(apss::exchange_key_bits(2) == 33);
  CHECK(apss::exchange_key_bits(3) == 34);
  CHECK(apss::exchange_key_bits(4) == 34);
  CHECK(apss::exchange_key_bits(5) == 35);
  CHECK(apss::exchange_key_bits((int64_t)1 << 30) == 62);
  CHECK(apss::exchange_key_bits(((int64_t)1 << 30) + 1) == 63);
  CHECK(apss::exchange_key_bits(((int64_t)1 << 31) - 1) == 63);
}

int main() {
  every_injected_failure();
  two_failures_in_one_step();
  skip_if_already_failed();
  barrier_reuse();
  two_groups_one_flag();
  run_members_joins();
  offsets_and_key_width();
  if (fails.load()) {
    std::printf("lockstep selftest: %d check(s) failed\n", fails.load());
    return 1;
  }
  std::printf("lockstep selftest ok\n");
  return 0;
}
