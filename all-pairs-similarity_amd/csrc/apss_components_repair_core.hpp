// apss_components_repair_core.hpp -- the per-slot decisions of the components' repair (apss_components_repair.hpp) as
// plain functions, so that a C++ program runs the very decisions the kernels take (host/components_repair_selftest.cpp, under the
// sanitizers).
//
// All three work on a FLAT forest (k_cc_label mode 0: parent[x] is x's root) and on the mark bytes of apss_remove.  They rest on
// one invariant, kept by apss_remove itself: a marked row is a singleton of the forest once the call returns.  So before a call's
// repair the only marked rows with anything under or above them are the ones this call marked.
//   touch     a marked slot flags its root: the component has to be taken apart.  (A row marked earlier flags itself.)
//   detach    a slot whose root is flagged becomes its own parent; one that hung under another slot gives one union back; one
//             that is live is a row of the re-join.
//   renumber  a compaction moves live slot x to rank(x), the live slots below it: parent[x] moves with it.  Ranks are monotone, so
//             parent <= slot keeps holding and a component's smallest slot stays its smallest.
#ifndef APSS_COMPONENTS_REPAIR_CORE_HPP
#define APSS_COMPONENTS_REPAIR_CORE_HPP

#include <cstdint>

#include "apss_components_core.hpp"

namespace apss {

// touch: the flag a slot sets, or -1 for none.  parent_x: x's root
APSS_CC_FN int32_t cr_touch(bool dead_x, int32_t parent_x) { return dead_x ? parent_x : -1; }

struct CrDetach {
  bool detach;  // parent[x] = x
  bool unhook;  // x was no root: one union of the count goes with it
  bool select;  // a live row of a touched component: re-joined
};

// detach: root_flagged: the flag of parent_x, x's root
APSS_CC_FN CrDetach cr_detach(int32_t x, int32_t parent_x, bool root_flagged, bool dead_x) {
  CrDetach d;
  d.detach = root_flagged;
  d.unhook = root_flagged && parent_x != x;
  d.select = root_flagged && !dead_x;
  return d;
}

// renumber: the parent of live slot x at its new place rank_x.  rank_parent: the rank of x's root, parent_dead: its mark (by the
// invariant never set -- a live row under a marked one would take the rank of the next live slot, a row it has no edge with: it
// becomes a singleton instead, which loses edges but claims none)
APSS_CC_FN int32_t cr_renumber(int32_t rank_x, int32_t rank_parent, bool parent_dead) { return parent_dead ? rank_x : rank_parent; }

}  // namespace apss

#endif  // APSS_COMPONENTS_REPAIR_CORE_HPP
