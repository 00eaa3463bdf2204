// apss_components_core.hpp -- find / link / shorten of the union-find behind apss_set_components (apss_components.hpp;
// DESIGN.md 5i), as functions over a small atomics policy, so that plain C++ runs the very code the kernels run
// (host/components_selftest.cpp, under the sanitizers).
//
// parent[] is a forest over slots 0 .. rows - 1.  A policy P gives the three accesses to one of its words:
//   P::load(p)                 the word, read atomically (relaxed)
//   P::cas(p, expected, want)  compare-and-swap, returns the word as it was
//   P::fetch_min(p, v)         atomic minimum
// The device policy (apss_components.hpp) uses __hip_atomic_* at agent scope, the host policy below __atomic_*.
//
// Invariants, kept by every function here at every moment and whatever the interleaving:
//   I1  parent[x] <= x.
//   I2  parent[x] is a slot of x's component (an ancestor of x, or x).
//   I3  a root (parent[r] == r) stops being one only by the compare-and-swap of cc_link, which puts it under a SMALLER slot of
//       another component.  So a link never closes a cycle, and every successful one joins two components.
//   I4  every read of parent[] is P::load: never a plain load.
//   I5  a path is shortened only by writing an ANCESTOR of x into parent[x], with P::fetch_min: never a plain store, so a late
//       shortening cannot undo an earlier, deeper one.
// A value read from parent[x] that is out of date (I1, I2 and I5: every value parent[x] ever held is still an ancestor of x or x
// itself) therefore costs steps or a retry, never a wrong answer; and since every link points from the larger root to the
// smaller slot, the root a component ends with is its smallest slot -- whatever the order of the links.
#ifndef APSS_COMPONENTS_CORE_HPP
#define APSS_COMPONENTS_CORE_HPP

#include <cstdint>

#if defined(__HIPCC__)
#define APSS_CC_FN __host__ __device__ inline
#else
#define APSS_CC_FN inline
#endif

namespace apss {

// the host's accesses (GCC / Clang builtins)
struct CcHostAtomics {
  static int32_t load(const int32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
  static int32_t cas(int32_t *p, int32_t expected, int32_t want) {
    __atomic_compare_exchange_n(p, &expected, want, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
    return expected;
  }
  static void fetch_min(int32_t *p, int32_t v) {
    int32_t cur = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < cur && !__atomic_compare_exchange_n(p, &cur, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
  }
};

// A slot that was a root of x's component when it was read.  Path halving on the way: every slot passed gets its grandparent (I5).
template <class P>
APSS_CC_FN int32_t cc_find(int32_t *parent, int32_t x) {
  int32_t p = P::load(parent + x);
  while (p != x) {
    const int32_t g = P::load(parent + p);
    if (g != p) P::fetch_min(parent + x, g);
    x = p;
    p = g;
  }
  return x;
}

// do u and v hang under one parent already?  (I2: then they are of one component.)  Two loads, no walk
template <class P>
APSS_CC_FN bool cc_same_parent(const int32_t *parent, int32_t u, int32_t v) {
  return P::load(parent + u) == P::load(parent + v);
}

// The edge u - v.  True when this call joined two components.  The larger root goes under the smaller; a compare-and-swap that
// finds the larger one no root any more goes on from what it holds now
template <class P>
APSS_CC_FN bool cc_link(int32_t *parent, int32_t u, int32_t v) {
  for (;;) {
    u = cc_find<P>(parent, u);
    v = cc_find<P>(parent, v);
    if (u == v) return false;
    const int32_t hi = u > v ? u : v, lo = u > v ? v : u;
    const int32_t was = P::cas(parent + hi, hi, lo);
    if (was == hi) return true;
    u = was;
    v = lo;
  }
}

// x's root while nothing links (the labelling), with x itself put right under it (I5)
template <class P>
APSS_CC_FN int32_t cc_root_flat(int32_t *parent, int32_t x) {
  const int32_t r = cc_find<P>(parent, x);
  if (r != x) P::fetch_min(parent + x, r);
  return r;
}

}  // namespace apss

#endif  // APSS_COMPONENTS_CORE_HPP
