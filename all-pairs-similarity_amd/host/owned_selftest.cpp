// owned_selftest.cpp -- the owning types of csrc/apss_owned.hpp in plain C++, over a counting fake of the back-end: malloc-backed,
// it counts live blocks and bytes, records the order of allocate / copy / wait / free, and fails the k-th allocation, copy or wait
// on request.  Checked: the capacities of every growth policy against literal tables, `keep`, the order of operations, the
// ledger after every step, a failure injected at every back-end call of every policy (error returned, nothing leaked, ledger
// consistent, allocate-first arrays intact, free-first arrays empty), moves, the event / pinned / stream owners, and a struct of
// arrays assigned from an empty one.
// No GPU, no HIP header.  Build: see Makefile in this directory (tests/test_owned_host.py builds it under the sanitizers and runs it).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../csrc/apss_owned.hpp"

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++fails;                                                \
    }                                                         \
  } while (0)

struct Fake {
  using Error = int;
  using Stream = int;
  using Event = int;
  static constexpr Error ok = 0;
  static inline std::map<void *, size_t> blocks, host_blocks;  // live, with their sizes
  static inline std::string log;                               // a(llocate) c(opy) w(ait) f(ree), in order
  static inline int fail_alloc = 0, fail_copy = 0, fail_wait = 0;  // k: the k-th call from now fails (0: none)
  static inline int events_made = 0, events_dropped = 0, events_untimed = 0, streams_made = 0, streams_dropped = 0, records = 0;
  static inline int fail_event = 0, fail_host = 0;

  static bool hit(int &k) { return k > 0 && --k == 0; }
  static size_t live_bytes() {
    size_t b = 0;
    for (const auto &kv : blocks) b += kv.second;
    return b;
  }
  static Error alloc(void **p, size_t bytes) {
    log += 'a';
    if (hit(fail_alloc)) return 2;
    *p = std::malloc(bytes ? bytes : 1);
    blocks[*p] = bytes;
    return ok;
  }
  static void free(void *p) {
    log += 'f';
    CHECK(blocks.erase(p) == 1);  // (a double free, or a pointer that was never ours)
    std::free(p);
  }
  static Error copy(void *dst, const void *src, size_t bytes, Stream) {
    log += 'c';
    if (hit(fail_copy)) return 3;
    CHECK(blocks.count(dst) && blocks[dst] >= bytes && blocks.count(const_cast<void *>(src)) && blocks[const_cast<void *>(src)] >= bytes);
    std::memcpy(dst, src, bytes);
    return ok;
  }
  static Error wait(Stream) {
    log += 'w';
    return hit(fail_wait) ? 4 : ok;
  }
  static Error host_alloc(void **p, size_t bytes) {
    if (hit(fail_host)) return 5;
    *p = std::malloc(bytes ? bytes : 1);
    host_blocks[*p] = bytes;
    return ok;
  }
  static void host_free(void *p) {
    CHECK(host_blocks.erase(p) == 1);
    std::free(p);
  }
  static Error event_make(Event *e, bool timing) {
    if (hit(fail_event)) return 6;
    *e = 100 + ++events_made;
    if (!timing) ++events_untimed;
    return ok;
  }
  static Error event_record(Event e, Stream) {
    CHECK(e > 100);
    ++records;
    return ok;
  }
  static void event_drop(Event e) {
    CHECK(e > 100);
    ++events_dropped;
  }
  static Error stream_make(Stream *s) {
    *s = 200 + ++streams_made;
    return ok;
  }
  static void stream_drop(Stream s) {
    CHECK(s > 200);
    ++streams_dropped;
  }
};

template <class T>
using Arr = apss::DevArray<T, Fake>;
using apss::GrowPolicy;

static std::string take_log() {
  std::string l;
  l.swap(Fake::log);
  return l;
}

// ---- capacities, against literal tables
struct CapStep {
  const GrowPolicy *pol;
  size_t n, want_cap;
  const char *want_log;  // the back-end calls of the step ("" : a request that fits calls nothing)
};

static void run_table(const char *what, const std::vector<CapStep> &steps) {
  size_t ledger = 0;
  {
    Arr<int32_t> a;
    take_log();
    for (const CapStep &s : steps) {
      CHECK(a.grow(*s.pol, s.n, 0, 0, &ledger) == Fake::ok);
      const std::string l = take_log();
      if (a.cap != s.want_cap || l != s.want_log) {
        std::printf("FAIL %s: n = %zu: cap %zu (want %zu), calls '%s' (want '%s')\n", what, s.n, a.cap, s.want_cap, l.c_str(), s.want_log);
        ++fails;
      }
      CHECK(ledger == a.cap * sizeof(int32_t) && Fake::live_bytes() == ledger && Fake::blocks.size() == 1);
    }
  }
  CHECK(ledger == 0 && Fake::blocks.empty());
  take_log();
}

static void capacities() {
  using namespace apss;
  // the handle: max(n, cap + cap / 2), or exactly n, and never under 64; the new block first
  run_table("handle", {{&kGrowHandle, 1, 64, "a"}, {&kGrowHandle, 64, 64, ""}, {&kGrowHandle, 65, 96, "awf"}, {&kGrowHandle, 200, 200, "awf"}});
  run_table("handle, exact", {{&kGrowHandleExact, 10, 64, "a"}, {&kGrowHandleExact, 100, 100, "awf"}, {&kGrowHandleExact, 1000, 1000, "awf"},
                              {&kGrowHandleExact, 999, 1000, ""}});
  // the group: the same rule over a floor of 256; the old block first
  run_table("group", {{&kGrowGroup, 1, 256, "a"}, {&kGrowGroup, 256, 256, ""}, {&kGrowGroup, 257, 384, "wfa"}, {&kGrowGroup, 1000, 1000, "wfa"}});
  run_table("group, appended to", {{&kGrowGroupKeep, 0, 256, "a"}, {&kGrowGroupKeep, 300, 384, "awf"}, {&kGrowGroupKeep, 2000, 2000, "awf"}});
  // a stage: exactly n, no floor; the old block first, no wait
  run_table("stage", {{&kGrowStage, 1, 1, "a"}, {&kGrowStage, 7, 7, "fa"}, {&kGrowStage, 5, 7, ""}, {&kGrowStage, 1000, 1000, "fa"}});
  run_table("stage, kept", {{&kGrowStageKeep, 3, 3, "a"}, {&kGrowStageKeep, 4, 4, "awf"}});
}

// ---- keep: the first elements survive, and the copy stands between the allocation and the wait
static void keeps() {
  using namespace apss;
  for (const GrowPolicy *pol : {&kGrowHandle, &kGrowHandleExact, &kGrowGroupKeep, &kGrowStageKeep}) {
    Arr<int64_t> a;
    CHECK(a.grow(*pol, 100, 0, 0, nullptr) == Fake::ok);
    for (size_t i = 0; i < a.cap; ++i) a.p[i] = (int64_t)(i * 7 + 1);
    const int64_t *old = a.p;
    take_log();
    CHECK(a.grow(*pol, 5000, 77, 0, nullptr) == Fake::ok);
    CHECK(take_log() == "acwf" && a.p != old && a.cap >= 5000);
    bool same = true;
    for (size_t i = 0; i < 77; ++i) same = same && a.p[i] == (int64_t)(i * 7 + 1);
    CHECK(same);
  }
  CHECK(Fake::blocks.empty());
  take_log();
}

// ---- ledgers: each the sum over its own arrays after every step
static void ledgers() {
  using namespace apss;
  size_t la = 0, lb = 0;
  {
    Arr<float> x, y;
    Arr<char> z;
    Arr<double> other;
    const auto sum = [&] { return x.cap * sizeof(float) + y.cap * sizeof(float) + z.cap; };
    CHECK(x.grow(kGrowHandle, 10, 0, 0, &la) == Fake::ok && la == sum());
    CHECK(other.grow(kGrowStage, 33, 0, 0, &lb) == Fake::ok && la == sum() && lb == 33 * sizeof(double));
    CHECK(y.grow(kGrowGroup, 300, 0, 0, &la) == Fake::ok && la == sum());
    CHECK(z.grow(kGrowStage, 12345, 0, 0, &la) == Fake::ok && la == sum());
    CHECK(x.grow(kGrowHandle, 1000, 10, 0, &la) == Fake::ok && la == sum());
    CHECK(other.grow(kGrowStage, 77, 0, 0, &lb) == Fake::ok && la == sum() && lb == 77 * sizeof(double));
    CHECK(y.grow(kGrowGroup, 3000, 0, 0, &la) == Fake::ok && la == sum());
    y.reset();
    CHECK(y.cap == 0 && !y.p && la == sum());
    CHECK(Fake::live_bytes() == la + lb);
    CHECK(la == 1000 * sizeof(float) + 12345);
  }
  CHECK(la == 0 && lb == 0 && Fake::blocks.empty());
  take_log();
}

// ---- a failure at every back-end call of every policy
static void failures() {
  using namespace apss;
  struct Case {
    const GrowPolicy *pol;
    size_t keep;
    const char *calls;  // the growth's calls when nothing fails
  };
  const Case cases[] = {{&kGrowHandle, 40, "acwf"},      {&kGrowHandle, 0, "awf"},   {&kGrowHandleExact, 40, "acwf"}, {&kGrowGroupKeep, 40, "acwf"},
                        {&kGrowGroupKeep, 0, "awf"},     {&kGrowStageKeep, 40, "acwf"}, {&kGrowGroup, 0, "wfa"},       {&kGrowStage, 0, "fa"}};
  for (const Case &c : cases) {
    const std::string calls = c.calls;
    for (size_t at = 0; at < calls.size(); ++at) {
      if (calls[at] == 'f') continue;  // (a free cannot fail)
      size_t ledger = 0;
      {
        Arr<int32_t> a;
        CHECK(a.grow(*c.pol, 100, 0, 0, &ledger) == Fake::ok);
        for (size_t i = 0; i < a.cap; ++i) a.p[i] = (int32_t)i - 5;
        const int32_t *old = a.p;
        const size_t old_cap = a.cap;
        take_log();
        (calls[at] == 'a' ? Fake::fail_alloc : calls[at] == 'c' ? Fake::fail_copy : Fake::fail_wait) = 1;
        const int e = a.grow(*c.pol, 100000, c.keep, 0, &ledger);
        CHECK(e == (calls[at] == 'a' ? 2 : calls[at] == 'c' ? 3 : 4));
        CHECK(Fake::fail_alloc == 0 && Fake::fail_copy == 0 && Fake::fail_wait == 0);  // (the call that was to fail was reached)
        const bool free_first = c.pol->order != GrowOrder::kAllocCopyWaitFree;
        if (free_first && calls[at] == 'a') {
          CHECK(!a.p && a.cap == 0 && ledger == 0 && Fake::blocks.empty());  // empty, as the code it replaces left it
        } else {  // the array, its contents and the ledger are what they were
          CHECK(a.p == old && a.cap == old_cap && ledger == old_cap * sizeof(int32_t));
          CHECK(Fake::blocks.size() == 1 && Fake::live_bytes() == ledger);
          bool same = true;
          for (size_t i = 0; i < a.cap; ++i) same = same && a.p[i] == (int32_t)i - 5;
          CHECK(same);
        }
        // ... and it grows when asked again
        CHECK(a.grow(*c.pol, 100000, free_first && calls[at] == 'a' ? 0 : c.keep, 0, &ledger) == Fake::ok);
        CHECK(a.cap == 100000 && ledger == a.cap * sizeof(int32_t) && Fake::live_bytes() == ledger);
      }
      CHECK(ledger == 0 && Fake::blocks.empty());
    }
  }
  // the first allocation of an empty array
  for (const GrowPolicy *pol : {&kGrowHandle, &kGrowGroup, &kGrowStage}) {
    size_t ledger = 0;
    Arr<double> a;
    Fake::fail_alloc = 1;
    CHECK(a.grow(*pol, 10, 0, 0, &ledger) == 2 && !a.p && a.cap == 0 && ledger == 0 && Fake::blocks.empty());
  }
  take_log();
}

// ---- moves
struct Holder {
  Arr<int32_t> q, c;
  Arr<float> s;
  int tag = 0;
};

static void moves() {
  using namespace apss;
  size_t ledger = 0;
  {
    Arr<int32_t> a, x, y, z;
    CHECK(grow_all(kGrowStage, 9, 0, 0, &ledger, x, y, z) == Fake::ok && x.cap == 9 && y.cap == 9 && z.cap == 9 && ledger == 108);
    Fake::fail_alloc = 2;  // the first failure ends it: x grown, y emptied by its free-first order, z untouched
    CHECK(grow_all(kGrowStage, 20, 0, 0, &ledger, x, y, z) == 2 && x.cap == 20 && !y.p && z.cap == 9 && ledger == 116);
    CHECK(grow_all(kGrowStage, 20, 0, 0, &ledger, x, y, z) == Fake::ok && z.cap == 20 && ledger == 240 && Fake::live_bytes() == 240);
    x.reset(), y.reset(), z.reset();
    CHECK(a.grow(kGrowHandle, 10, 0, 0, &ledger) == Fake::ok);
    int32_t *pa = a.p;
    Arr<int32_t> b(std::move(a));
    CHECK(!a.p && a.cap == 0 && b.p == pa && b.cap == 64 && ledger == 64 * sizeof(int32_t));
    Arr<int32_t> full;
    CHECK(full.grow(kGrowStage, 1000, 0, 0, &ledger) == Fake::ok && Fake::blocks.size() == 2);
    full = std::move(b);  // onto a full array: its block goes
    CHECK(full.p == pa && full.cap == 64 && !b.p && b.cap == 0 && Fake::blocks.size() == 1 && ledger == 64 * sizeof(int32_t));
    Arr<int32_t> &same = full;
    full = std::move(same);  // (self-assignment changes nothing)
    CHECK(full.p == pa && Fake::blocks.size() == 1);
    Arr<int32_t> other;
    CHECK(other.grow(kGrowGroup, 1, 0, 0, nullptr) == Fake::ok);
    int32_t *po = other.p;
    std::swap(full, other);  // (arrays of different ledgers: each takes its own along)
    CHECK(full.p == po && full.cap == 256 && other.p == pa && other.cap == 64 && Fake::blocks.size() == 2 && ledger == 64 * sizeof(int32_t));
    other.reset();
    CHECK(ledger == 0 && Fake::blocks.size() == 1);
    a.reset();  // (an empty array: nothing happens)
    CHECK(ledger == 0 && Fake::blocks.size() == 1);
  }
  CHECK(Fake::blocks.empty() && ledger == 0);
  {
    std::vector<Holder> v;
    for (int i = 0; i < 40; ++i) {  // (the vector reallocates several times on the way)
      v.emplace_back();
      Holder &h = v.back();
      h.tag = i;
      CHECK(h.q.grow(kGrowGroup, (size_t)i + 1, 0, 0, &ledger) == Fake::ok && h.s.grow(kGrowStage, (size_t)i + 1, 0, 0, &ledger) == Fake::ok);
      h.s.p[i] = (float)i;
    }
    CHECK(Fake::blocks.size() == 80 && Fake::live_bytes() == ledger);
    bool same = true;
    for (int i = 0; i < 40; ++i) same = same && v[(size_t)i].tag == i && v[(size_t)i].s.p[i] == (float)i && !v[(size_t)i].c.p;
    CHECK(same);
    v.erase(v.begin() + 3);
    CHECK(Fake::blocks.size() == 78 && Fake::live_bytes() == ledger && v[3].tag == 4 && v[3].s.p[4] == 4.f);
  }
  CHECK(Fake::blocks.empty() && ledger == 0);
  take_log();
}

// ---- the other owners
static void owners() {
  using namespace apss;
  {
    OwnedEvent<Fake> never, timed, untimed{kUntimed};
    CHECK(!timed.made() && Fake::events_made == 0);
    CHECK(timed.record(0) == Fake::ok && timed.made() && Fake::events_made == 1 && Fake::records == 1);
    CHECK(timed.record(0) == Fake::ok && Fake::events_made == 1 && Fake::records == 2);  // made once
    CHECK((int)timed == 101);
    CHECK(untimed.record(0) == Fake::ok && Fake::events_made == 2 && Fake::events_untimed == 1);
    Fake::fail_event = 1;
    OwnedEvent<Fake> failing;
    CHECK(failing.record(0) == 6 && !failing.made() && Fake::records == 3);
    CHECK(failing.record(0) == Fake::ok && failing.made() && Fake::events_made == 3);
    OwnedEvent<Fake> moved(std::move(failing));
    CHECK(moved.made() && !failing.made());
    timed = OwnedEvent<Fake>{};  // assigned from an empty one: dropped at once
    CHECK(!timed.made() && Fake::events_dropped == 1);
  }
  CHECK(Fake::events_made == 3 && Fake::events_dropped == 3);  // dropped once each; the one never recorded never made
  {
    PinnedArray<int64_t, Fake> pin, never;  // (the array over the back-end's host side: exactly n, the old block freed first)
    const auto want = [&](size_t n) { return pin.grow(kGrowStage, n, 0, 0, nullptr); };
    CHECK(want(100) == Fake::ok && pin.cap == 100 && Fake::host_blocks.size() == 1 && Fake::host_blocks.begin()->second == 800);
    int64_t *p = pin.p;
    p[99] = 5;
    CHECK(want(50) == Fake::ok && pin.p == p);  // fits
    CHECK(want(101) == Fake::ok && pin.cap == 101 && Fake::host_blocks.size() == 1);
    Fake::fail_host = 1;
    CHECK(want(1000) == 5 && !pin.p && pin.cap == 0 && Fake::host_blocks.empty());
    CHECK(want(10) == Fake::ok && Fake::blocks.empty());  // (never a device block)
  }
  CHECK(Fake::host_blocks.empty());
  {
    OwnedStream<Fake> never, s;
    CHECK(!s.made() && s.make() == Fake::ok && s.made() && (int)s == 201 && s.make() == Fake::ok && Fake::streams_made == 1);
    std::vector<OwnedStream<Fake>> v(3);
    CHECK(v[1].make() == Fake::ok);
    v.resize(100);
    CHECK((int)v[1] == 202 && v[1].made() && !v[0].made() && Fake::streams_dropped == 0);
    v[1] = {};  // assigned from an empty one: destroyed at once
    CHECK(Fake::streams_dropped == 1 && !v[1].made());
  }
  CHECK(Fake::streams_made == 2 && Fake::streams_dropped == 2);
}

// ---- a stage's work as the components stage holds it: arrays, events and flags in one struct beside the owner's ledger; turning the
// stage off is an assignment from an empty struct
struct Work {
  size_t *ledger = nullptr;
  apss::OwnedEvent<Fake> e0, e1;
  Arr<int32_t> parent, label;
  Arr<unsigned long long> words;
  size_t cap = 0;
  bool dirty = true;
};

static void stage_off() {
  using namespace apss;
  size_t reserved = 0;
  Arr<float> store;
  CHECK(store.grow(kGrowHandle, 500, 0, 0, &reserved) == Fake::ok);
  const size_t before = reserved;
  const int dropped = Fake::events_dropped;
  Work w;
  for (int round = 0; round < 2; ++round) {  // on, off, on, off
    w.ledger = &reserved;
    CHECK(w.words.grow(kGrowStage, 4, 0, 0, w.ledger) == Fake::ok);
    for (size_t rows : {1000u, 1200u, 5000u}) {
      CHECK(w.parent.grow(kGrowStageKeep, rows, w.cap, 0, w.ledger) == Fake::ok && w.label.grow(kGrowStage, rows, 0, 0, w.ledger) == Fake::ok);
      w.cap = rows;
      CHECK(reserved == before + 2 * rows * sizeof(int32_t) + 4 * sizeof(unsigned long long) && Fake::live_bytes() == reserved);
    }
    CHECK(w.e0.record(0) == Fake::ok && w.e1.record(0) == Fake::ok);
    w.dirty = false;
    w = Work{};
    CHECK(reserved == before && Fake::blocks.size() == 1 && Fake::live_bytes() == reserved);
    CHECK(!w.parent.p && !w.label.p && !w.words.p && w.cap == 0 && w.dirty && !w.ledger && !w.e0.made());
    CHECK(Fake::events_dropped == dropped + 2 * (round + 1));
  }
  store.reset();
  CHECK(reserved == 0 && Fake::blocks.empty());
}

int main() {
  capacities();
  keeps();
  ledgers();
  failures();
  moves();
  owners();
  stage_off();
  CHECK(Fake::blocks.empty() && Fake::host_blocks.empty() && Fake::events_made == Fake::events_dropped && Fake::streams_made == Fake::streams_dropped);
  if (fails) {
    std::printf("owned selftest: %d check(s) failed\n", fails);
    return 1;
  }
  std::printf("owned selftest ok\n");
  return 0;
}
