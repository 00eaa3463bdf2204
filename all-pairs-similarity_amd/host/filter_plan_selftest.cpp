// The filter plan (csrc/apss_filter_plan.hpp) against tables of literal decisions, on the CPU.  A wrong instantiation, window or
// scale still returns the right pairs, only slower, so no result test sees the rule: this one pins it down on both sides of every
// threshold -- the workgroup size by tile rows and 8-bit sums, the window's clamp, virtual rows, the 1024-thread kernel's 17.0, the
// long tail at kLongLenW, the thin-round rule (long segments per tile, staging waves at nw / 4 for every lane count, adding waves x
// steps against k_probe_coarse's 8 x U, 7 steps, the measured chunks, the 1.05 x longest-row bound), merged rounds, two planes,
// the 8- and 16-bit scales at every k, the coarse tile choice, every hook alone, and the shapes DESIGN.md and the thin-round tests
// quote -- and then sweeps a grid of facts: the plans without a listed variant are exactly the literal list (at run time they are
// APSS_E_UNSUPPORTED errors), one number over every decision of the grid is the literal one, and every listed variant is returned
// at least once by the table or the grid.
// The expected values were printed by the decision code as it stood before the header existed (pick_cx_tile, the scale section of
// choose_path, merged_scale, the merge loop of plan_merged_rounds and plan_filter of csrc/apss_hip.hip, copied into a scratch
// program with a stand-in for the handle fields they read), not by the code under test; so were the diag lines the formatter is
// held to, the unlisted plans, and the grid's number.  Built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>

#include "../csrc/apss_filter_plan.hpp"

namespace {

using apss::CxVariant;
using apss::FilterFacts;
using apss::FilterHooks;
using apss::TileFacts;

// a variant by the name apss_stats.probe_kernel gives it, template arguments in the tables' order
std::string variant_name(const CxVariant &v) {
  char s[160];
  if (v.even && v.planes) snprintf(s, sizeof s, "planes<%d>%s", v.u, v.block == 512 && !v.shard && !v.sgn && v.acc8 && !v.merge ? "" : " (odd)");
  else if (v.even && v.merge) snprintf(s, sizeof s, "merged<%d, a8 %d>%s", v.u, (int)v.acc8, v.block == 512 && v.shard && !v.sgn ? "" : " (odd)");
  else if (v.even) snprintf(s, sizeof s, "even<%d, %d, sh %d, sg %d, a8 %d>", v.block, v.u, (int)v.shard, (int)v.sgn, (int)v.acc8);
  else snprintf(s, sizeof s, "coarse<%d, %d, sh %d, ch %d, vr %d, sg %d, lp %d, a8 %d>", v.block, v.u, (int)v.shard, v.chunk, (int)v.vrows, (int)v.sgn, (int)v.longpf, (int)v.acc8);
  std::string name = s;
  if (v.even && (v.chunk != 16 || v.vrows || v.longpf)) name += " (no even shape)";
  return name;
}

// ---- the shapes the project quotes (apss/synth.py; tests/test_gpu_even_wipe.py), as one whole-store self-join sees them.
// FilterFacts: acc8, shard_rule, sgn, hybrid | s_max_nnz, s_nnz_end, nq, idx_nnz | max_merge_log2, planes_scale, q_chunk |
//              cb, max_seg, long_segs, n_tiles, round_chunks | n_rows, dim, term_lo, term_hi, no_acc8
// C3: a million rows of 100 uniform terms over 100,000, 31 tiles of 32768 rows, 33 postings per (tile, term)
FilterFacts c3() { return {false, false, false, false, 100, 100000000, 1000000, 100000000, 0, 128.0, 977, 32768, 64, 0, 31, 255.0, 1000000, 100000, 0, 100000, false}; }
// ... one of its T term shards: 8-bit sums over 65536-row tiles, two rows may share a round
FilterFacts c3_shard(int T) {
  FilterFacts f = c3();
  f.acc8 = f.shard_rule = true;
  f.s_max_nnz = T == 2 ? 70 : (T == 4 ? 45 : 30);
  f.s_nnz_end = f.idx_nnz = 100000000 / T;
  f.max_merge_log2 = 1;
  f.planes_scale = 0.0;
  f.cb = 65536;
  f.n_tiles = 16;
  f.round_chunks = 0.0;
  f.term_hi = 100000 / T;
  return f;
}
// ... the same shard on a handle latched back to 16-bit sums over 32768-row tiles
FilterFacts c3_shard16(int T) {
  FilterFacts f = c3_shard(T);
  f.acc8 = false;
  f.cb = 32768;
  f.n_tiles = 31;
  f.no_acc8 = true;
  return f;
}
// C5's sparse shape at a fifth of N: two million rows of 200 terms over a million, 131072-row tiles, 8-bit sums, 1024 threads
FilterFacts c5s() { return {true, false, false, false, 200, 400000000, 2000000, 400000000, 0, 64.0, 1954, 131072, 60, 0, 16, 210.0, 2000000, 1000000, 0, 1000000, false}; }
// the power-law tail behind a dense-head block on a term shard: 66 terms of a row left, uniform estimate 85 chunks per round
FilterFacts power_law_tail(double measured) {
  return {true, true, false, true, 120, 132000000, 2000000, 132000000, 0, 0.0, 1954, 65536, 200, 40, 31, measured, 2000000, 1000000, 0, 125000, false};
}
// tests/test_gpu_even_wipe.py: 6144 rows of 100 terms, filter tiles of 2048 rows, APSS_DEBUG=planes
FilterFacts wipe(int dim) { return {false, false, false, false, 100, 614400, 6144, 614400, 0, 128.0, 6, 2048, 60, 0, 3, 215.0, 6144, dim, 0, dim, false}; }

#define H(...) ([] { FilterHooks k; __VA_ARGS__; return k; }())
#define F(base, ...) ([] { FilterFacts f = base; __VA_ARGS__; return f; }())

// ---- the sweep's grid: a few values of every fact on either side of its thresholds, under no hook and under every hook alone.
// Combinations that choose_path cannot hand over are left out (valid()): 8-bit sums need tiles of >= 65536 rows, non-negative
// weights and rows of <= 512 terms; the shard rule over larger tiles than 32768 rows needs 8-bit sums, and so do 131072-row tiles,
// which only a plain handle picks; a dense-head block sets the shard rule and takes no signed weights; chunk8 and window take
// neither signed weights nor 8-bit sums; rows merge on a term shard of non-negative weights only.
struct Hook {
  const char *name;
  FilterHooks k;
};
const Hook kGridHooks[] = {
    {"", H()},
    {"chunk8", H(k.chunk8 = true)},
    {"window=2", H(k.window = 2)},
    {"window=3", H(k.window = 3)},
    {"window=4", H(k.window = 4)},
    {"window=5", H(k.window = 5)},
    {"no_acc8", H(k.no_acc8 = true)},
    {"no_planes", H(k.no_planes = true)},
    {"planes", H(k.planes = true)},
    {"flat_group=0", H(k.flat_group = 0)},
    {"flat_group=1", H(k.flat_group = 1)},
    {"no_even", H(k.no_even = true)},
    {"merge_u=5", H(k.merge_u = 5)},
    {"merge_single=2", H(k.merge_single = 2)},
};
bool valid(const FilterFacts &f, const FilterHooks &k) {
  if (f.acc8 && (f.cb < 65536 || f.sgn || f.s_max_nnz > 512 || f.no_acc8 || k.no_acc8 || k.chunk8)) return false;
  if (!f.acc8 && (f.cb > 65536 || (f.shard_rule && f.cb > 32768))) return false;
  if (f.cb > 65536 && f.shard_rule) return false;
  if (f.hybrid && (!f.shard_rule || f.sgn)) return false;
  if (f.sgn && (k.chunk8 || k.window || (f.cb > 32768 && f.s_max_nnz > 512))) return false;
  if (f.max_merge_log2 > 0 && (!f.shard_rule || f.sgn)) return false;
  if (f.planes_scale > 0 && (f.sgn || f.s_max_nnz > 512)) return false;
  return true;
}
struct RowShape {
  int64_t max_nnz;
  double terms;  // of a mean row
};
const RowShape kGridRows[] = {{12, 6.0}, {30, 12.5}, {45, 25.0}, {70, 50.0}, {100, 100.0}, {120, 118.0}, {128, 100.0}, {250, 200.0}, {512, 300.0}, {513, 300.0}};
struct TermShape {
  int32_t dim, term_lo, term_hi;
};
const TermShape kGridTerms[] = {{100000, 0, 100000}, {100000, 12500, 25000}, {1000000, 0, 1000000}, {6800, 0, 6800}};
struct GridPoint {
  const char *hook;
  RowShape r;
  int longs_per_tile, m, pl;
};
std::string grid_name(const GridPoint &g, const FilterFacts &f) {
  char name[256];
  snprintf(name, sizeof name, "%s%scb %d a8 %d sh %d sg %d hy %d | row %lld of %.1f | dim %d [%d, %d) | max_seg %u longs/tile %d measured %.0f | merge %d planes %d latch %d",
           g.hook, g.hook[0] ? " | " : "", (int)f.cb, (int)f.acc8, (int)f.shard_rule, (int)f.sgn, (int)f.hybrid, (long long)g.r.max_nnz, g.r.terms, (int)f.dim, (int)f.term_lo,
           (int)f.term_hi, (unsigned)f.max_seg, g.longs_per_tile, f.round_chunks, g.m, g.pl, (int)f.no_acc8);
  return name;
}
template <class Fn>
void for_each_grid(Fn fn) {
  const int64_t n = 1000000;
  for (const Hook &hk : kGridHooks)
    for (int32_t cb : {2048, 32768, 65536, 131072})
      for (int layout = 0; layout < 16; ++layout)  // acc8, shard_rule, sgn, hybrid
        for (const RowShape &r : kGridRows) {
          FilterFacts f{};
          f.acc8 = layout & 1;
          f.shard_rule = layout & 2;
          f.sgn = layout & 4;
          f.hybrid = layout & 8;
          f.s_max_nnz = r.max_nnz;
          f.s_nnz_end = f.idx_nnz = (int64_t)(r.terms * (double)n);
          f.nq = f.n_rows = n;
          f.cb = cb;
          f.n_tiles = (n + cb - 1) / cb;
          if (!valid(f, hk.k)) continue;
          for (const TermShape &t : kGridTerms)
            for (int seg_case = 0; seg_case < 4; ++seg_case)  // (max_seg 256 | 257) x (long segments 16 | 17 per tile)
              for (double measured : {0.0, 200.0})
                for (int m = 0; m <= 2; ++m)
                  for (int pl = 0; pl < 3; ++pl) {  // (two planes: no room | room, chunks of 255 | room, chunks of 256)
                    f.max_merge_log2 = m;
                    f.planes_scale = pl ? 64.0 : 0.0;
                    f.q_chunk = pl == 2 ? 256 : 255;
                    f.max_seg = seg_case & 1 ? 257 : 256;
                    f.long_segs = (uint32_t)((seg_case & 2 ? 17 : 16) * f.n_tiles);
                    f.round_chunks = measured;
                    f.dim = t.dim;
                    f.term_lo = t.term_lo;
                    f.term_hi = t.term_hi;
                    // (the handle's latch: tried where it matters, on a plain handle that could take two planes)
                    for (int latch = 0; latch <= (pl && !f.shard_rule && !f.acc8 ? 1 : 0); ++latch) {
                      f.no_acc8 = latch;
                      if (valid(f, hk.k)) fn(GridPoint{hk.name, r, seg_case & 2 ? 17 : 16, m, pl}, f, hk.k);
                    }
                  }
        }
}
// one number over everything a plan decides (FNV-1a over its fields)
struct PlanHash {
  uint64_t h = 1469598103934665603ULL;
  void add(int64_t x) {
    for (int i = 0; i < 8; ++i) h = (h ^ (uint64_t)((x >> (8 * i)) & 255)) * 1099511628211ULL;
  }
  void add(const apss::FilterPlan &p) {
    const CxVariant &v = p.v;
    for (int64_t x : {(int64_t)v.block, (int64_t)v.u, (int64_t)v.shard, (int64_t)v.chunk, (int64_t)v.vrows, (int64_t)v.sgn, (int64_t)v.longpf, (int64_t)v.acc8, (int64_t)v.even,
                      (int64_t)v.merge, (int64_t)v.planes, (int64_t)p.flat_waves, (int64_t)p.flat_group_log2, (int64_t)p.merge_log2, (int64_t)p.listed})
      add(x);
  }
};

// ---- plan_filter: name, facts, hooks | the variant, staging waves, log2 of the staging lanes per term and of the rows per round, listed
struct PlanRow {
  const char *name;
  FilterFacts f;
  FilterHooks k;
  const char *variant;
  int flat_waves, flat_group_log2, merge_log2;
  bool listed;
};
const PlanRow kPlanRows[] = {
    // workgroup size: 1024 threads over tiles of more than 65536 rows, and of more than 32768 without 8-bit sums
    {"block: cb 32768", F(c3()), H(), "planes<6>", 2, 0, 0, true},
    {"block: cb 65536, 16-bit sums", F(c5s(), f.acc8 = false; f.cb = 65536), H(), "even<1024, 3, sh 0, sg 0, a8 0>", 4, 0, 0, true},
    {"block: cb 65536, 8-bit sums", F(c5s(), f.cb = 65536), H(), "coarse<512, 5, sh 0, ch 16, vr 0, sg 0, lp 0, a8 1>", 0, 0, 0, true},
    {"block: cb 131072, 8-bit sums", F(c5s()), H(), "even<1024, 5, sh 0, sg 0, a8 1>", 4, 0, 0, true},
    // window of k_probe_coarse (no_even shows it): virtual rows, the clamp to 2 .. 5, the 1024-thread kernel's 17.0, forced windows, the long tail
    {"vrows: longest row 512", F(c3(), f.s_max_nnz = 512; f.planes_scale = 0), H(), "coarse<512, 5, sh 0, ch 16, vr 0, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"vrows: longest row 513", F(c3(), f.s_max_nnz = 513; f.planes_scale = 0), H(), "coarse<512, 5, sh 0, ch 16, vr 1, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"window: 1 step clamped to 2", F(c3(), f.s_nnz_end = 8000000; f.idx_nnz = 8000000), H(k.no_even = true), "coarse<512, 2, sh 0, ch 16, vr 0, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"window: 3 steps", F(c3(), f.s_nnz_end = 60000000), H(k.no_even = true), "coarse<512, 3, sh 0, ch 16, vr 0, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"window: 5 steps", F(c3()), H(k.no_even = true), "coarse<512, 5, sh 0, ch 16, vr 0, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"window: 6 steps clamped to 5", F(c3(), f.s_max_nnz = 120; f.s_nnz_end = 120000000), H(k.no_even = true), "coarse<512, 5, sh 0, ch 16, vr 0, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"1024 threads: 206 terms, 16.98 <= 17.0", F(c5s(), f.acc8 = false; f.cb = 65536; f.s_max_nnz = 250; f.s_nnz_end = 412000000), H(k.no_even = true), "coarse<1024, 3, sh 0, ch 16, vr 0, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"1024 threads: 207 terms, 17.06 > 17.0", F(c5s(), f.acc8 = false; f.cb = 65536; f.s_max_nnz = 250; f.s_nnz_end = 414000000), H(k.no_even = true), "coarse<1024, 5, sh 0, ch 16, vr 0, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"signed weights force 5 steps", F(c3(), f.sgn = true; f.planes_scale = 0; f.s_nnz_end = 8000000; f.idx_nnz = 8000000), H(), "coarse<512, 5, sh 0, ch 16, vr 0, sg 1, lp 0, a8 0>", 0, 0, 0, true},
    {"virtual rows force 5 steps", F(c3(), f.s_max_nnz = 513; f.planes_scale = 0; f.s_nnz_end = 8000000; f.idx_nnz = 8000000), H(), "coarse<512, 5, sh 0, ch 16, vr 1, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"signed weights, 1024 threads keep 3 steps", F(c5s(), f.acc8 = false; f.sgn = true; f.planes_scale = 0; f.cb = 65536; f.s_nnz_end = 40000000), H(), "coarse<1024, 3, sh 0, ch 16, vr 0, sg 1, lp 0, a8 0>", 0, 0, 0, true},
    {"virtual rows, 1024 threads keep 3 steps", F(c5s(), f.acc8 = false; f.planes_scale = 0; f.cb = 65536; f.s_max_nnz = 513), H(), "coarse<1024, 3, sh 0, ch 16, vr 1, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"virtual rows and signed weights", F(c3(), f.sgn = true; f.s_max_nnz = 513; f.planes_scale = 0), H(), "coarse<512, 5, sh 0, ch 16, vr 1, sg 1, lp 0, a8 0>", 0, 0, 0, true},
    {"virtual rows on a term shard: long sweeps", F(c3_shard16(2), f.s_max_nnz = 513; f.max_merge_log2 = 0), H(), "coarse<512, 5, sh 1, ch 16, vr 1, sg 0, lp 1, a8 0>", 0, 0, 0, true},
    {"long tail: longest segment kLongLenW", F(power_law_tail(200.0), f.acc8 = false; f.cb = 32768; f.max_seg = 256), H(), "even<512, 6, sh 1, sg 0, a8 0>", 2, 0, 0, true},
    {"long tail: longest segment kLongLenW + 1", F(power_law_tail(200.0), f.acc8 = false; f.cb = 32768; f.max_seg = 257), H(), "coarse<512, 5, sh 1, ch 16, vr 0, sg 0, lp 1, a8 0>", 0, 0, 0, true},
    {"long tail: 8-bit sums take none", F(power_law_tail(200.0), f.max_seg = 257), H(), "even<512, 6, sh 1, sg 0, a8 1>", 2, 0, 0, true},
    {"long tail: no dense-head block, none", F(power_law_tail(200.0), f.acc8 = false; f.hybrid = false; f.cb = 32768; f.max_seg = 257), H(), "even<512, 6, sh 1, sg 0, a8 0>", 2, 0, 0, true},
    // thin rounds (k_probe_even): long segments, staging waves, window steps against k_probe_coarse's, the measured chunks, the longest row
    {"long segments: 16 per tile", F(c3(), f.long_segs = 496), H(), "planes<6>", 2, 0, 0, true},
    {"long segments: 16 per tile and one", F(c3(), f.long_segs = 497), H(), "coarse<512, 5, sh 0, ch 16, vr 0, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"long segments: a term shard takes them", F(c3_shard(4), f.long_segs = 4970), H(), "merged<7, a8 1>", 2, 0, 1, true},
    {"staging: 32 terms, 16 lanes each, 2 waves", F(c3(), f.s_max_nnz = 32; f.s_nnz_end = 30000000), H(), "planes<2>", 2, 2, 0, true},
    {"staging: 33 terms, 32 lanes each", F(c3(), f.s_max_nnz = 33; f.s_nnz_end = 30000000), H(), "planes<2>", 2, 1, 0, true},
    {"staging: 64 terms, 32 lanes each, 2 waves", F(c3(), f.s_max_nnz = 64; f.s_nnz_end = 60000000), H(), "planes<4>", 2, 1, 0, true},
    {"staging: 65 terms, 64 lanes each", F(c3(), f.s_max_nnz = 65; f.s_nnz_end = 60000000), H(), "planes<4>", 2, 0, 0, true},
    {"staging: 128 terms, 2 waves = nw / 4", F(c3(), f.s_max_nnz = 128; f.s_nnz_end = 90000000; f.round_chunks = 0), H(), "planes<6>", 2, 0, 0, true},
    {"staging: 129 terms, 3 waves", F(c3(), f.s_max_nnz = 129; f.s_nnz_end = 90000000; f.round_chunks = 0), H(), "coarse<512, 5, sh 0, ch 16, vr 0, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"staging, 1024 threads: 256 terms, 4 waves = nw / 4", F(c5s(), f.s_max_nnz = 256), H(), "even<1024, 6, sh 0, sg 0, a8 1>", 4, 0, 0, true},
    {"staging, 1024 threads: 257 terms, 5 waves", F(c5s(), f.s_max_nnz = 257), H(), "coarse<1024, 5, sh 0, ch 16, vr 0, sg 0, lp 0, a8 1>", 0, 0, 0, true},
    {"staging: flat_group=0 at 32 terms", F(c3(), f.s_max_nnz = 32; f.s_nnz_end = 30000000), H(k.flat_group = 0), "planes<2>", 1, 0, 0, true},
    {"staging: flat_group=1 at 32 terms", F(c3(), f.s_max_nnz = 32; f.s_nnz_end = 30000000), H(k.flat_group = 1), "planes<2>", 1, 1, 0, true},
    {"staging: flat_group=2 at 65 terms asks too much", F(c3(), f.s_max_nnz = 65; f.s_nnz_end = 60000000), H(k.flat_group = 2), "planes<4>", 2, 0, 0, true},
    {"steps: 6 adding waves x 6 = 36 <= 40", F(c3()), H(), "planes<6>", 2, 0, 0, true},
    {"steps: 6 adding waves x 7 = 42 > 40", F(c3(), f.s_max_nnz = 120; f.s_nnz_end = 120000000), H(), "coarse<512, 5, sh 0, ch 16, vr 0, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"steps: 7 adding waves x 5 = 35 <= 40", F(c3(), f.s_max_nnz = 64; f.s_nnz_end = 64000000; f.round_chunks = 0; f.idx_nnz = 170900000), H(k.flat_group = 0), "planes<5>", 1, 0, 0, true},
    {"steps: 7 adding waves x 6 = 42 > 40", F(c3(), f.s_max_nnz = 64; f.s_nnz_end = 64000000; f.round_chunks = 0; f.idx_nnz = 200000000), H(k.flat_group = 0), "coarse<512, 5, sh 0, ch 16, vr 0, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"steps: 6 x 5 = 30 <= 8 x 4", F(c3(), f.s_max_nnz = 80; f.s_nnz_end = 80000000; f.round_chunks = 0; f.idx_nnz = 112000000), H(), "planes<5>", 2, 0, 0, true},
    {"steps: 6 x 6 = 36 > 8 x 4", F(c3(), f.s_max_nnz = 80; f.s_nnz_end = 80000000; f.round_chunks = 0; f.idx_nnz = 120000000), H(), "coarse<512, 4, sh 0, ch 16, vr 0, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"steps: rows of 48 terms, 6 x 3 = 18 <= 8 x 3", F(c3(), f.s_max_nnz = 48; f.s_nnz_end = 48000000; f.round_chunks = 0), H(), "planes<3>", 2, 1, 0, true},
    {"steps: rows of 60 terms, 6 x 4 = 24 <= 8 x 3", F(c3(), f.s_max_nnz = 60; f.s_nnz_end = 60000000; f.round_chunks = 0), H(), "planes<4>", 2, 1, 0, true},
    {"steps: rows of 48 terms, no_planes", F(c3(), f.s_max_nnz = 48; f.s_nnz_end = 48000000; f.round_chunks = 0), H(k.no_planes = true), "even<512, 3, sh 0, sg 0, a8 0>", 2, 1, 0, true},
    {"steps: rows of 60 terms, no_planes", F(c3(), f.s_max_nnz = 60; f.s_nnz_end = 60000000; f.round_chunks = 0), H(k.no_planes = true), "even<512, 4, sh 0, sg 0, a8 0>", 2, 1, 0, true},
    {"ue 7 on a term shard", F(c3_shard16(2), f.s_max_nnz = 128; f.s_nnz_end = 100000000; f.max_merge_log2 = 0), H(), "even<512, 7, sh 1, sg 0, a8 0>", 2, 0, 0, true},
    {"ue 8 on a term shard", F(c3_shard16(2), f.s_max_nnz = 128; f.s_nnz_end = 112000000; f.max_merge_log2 = 0), H(), "coarse<512, 5, sh 1, ch 16, vr 0, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"ue 7, 1024 threads", F(c5s(), f.s_max_nnz = 256; f.idx_nnz = 500000000; f.round_chunks = 0), H(), "even<1024, 7, sh 0, sg 0, a8 1>", 4, 0, 0, true},
    {"ue 8, 1024 threads", F(c5s(), f.s_max_nnz = 256; f.s_nnz_end = 500000000; f.idx_nnz = 500000000; f.round_chunks = 0), H(), "coarse<1024, 5, sh 0, ch 16, vr 0, sg 0, lp 0, a8 1>", 0, 0, 0, true},
    {"ue 4 becomes 5, 1024 threads", F(c5s(), f.s_nnz_end = 260000000; f.round_chunks = 0), H(), "even<1024, 5, sh 0, sg 0, a8 1>", 4, 0, 0, true},
    {"ue 3, 1024 threads", F(c5s(), f.s_max_nnz = 60; f.s_nnz_end = 100000000; f.round_chunks = 0), H(), "even<1024, 3, sh 0, sg 0, a8 1>", 4, 2, 0, true},
    {"measured chunks: none, the estimate's 85", F(power_law_tail(0.0)), H(), "even<512, 5, sh 1, sg 0, a8 1>", 2, 0, 0, true},
    {"measured chunks: 200 dealt out against 85 estimated", F(power_law_tail(200.0)), H(), "even<512, 6, sh 1, sg 0, a8 1>", 2, 0, 0, true},
    {"measured chunks: 60 do not override 85", F(power_law_tail(60.0)), H(), "even<512, 5, sh 1, sg 0, a8 1>", 2, 0, 0, true},
    {"longest row: 1.05 x 100 terms bounds the round", F(c3()), H(), "planes<6>", 2, 0, 0, true},
    {"longest row: 1.05 x 128 terms does not", F(c3(), f.s_max_nnz = 128), H(), "coarse<512, 5, sh 0, ch 16, vr 0, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"longest row: no bound on a term shard", F(c3_shard16(2), f.s_max_nnz = 50; f.max_merge_log2 = 0), H(), "even<512, 4, sh 1, sg 0, a8 0>", 2, 1, 0, true},
    {"signed weights take no thin rounds", F(c3(), f.sgn = true; f.planes_scale = 0), H(), "coarse<512, 5, sh 0, ch 16, vr 0, sg 1, lp 0, a8 0>", 0, 0, 0, true},
    // merged rounds: the merged round's window of at most 7 steps, a single row's of at most 4 (two rows of more never leave 7 steps, so merge_single moves that bound)
    {"merge: merged round 7 steps", F(c3_shard(4)), H(), "merged<7, a8 1>", 2, 0, 1, true},
    {"merge: merged round 8 steps", F(c3_shard(4), f.s_nnz_end = 30000000), H(), "even<512, 4, sh 1, sg 0, a8 1>", 2, 1, 0, true},
    {"merge: merged round 5 steps", F(c3_shard(8), f.s_nnz_end = 17000000), H(), "merged<5, a8 1>", 2, 1, 1, true},
    {"merge: merged round 5 steps, 16-bit sums", F(c3_shard16(8), f.s_max_nnz = 45; f.s_nnz_end = 31000000), H(), "merged<5, a8 0>", 2, 0, 1, true},
    {"merge: single row 4 steps, merge_single=4", F(c3_shard(4)), H(k.merge_single = 4), "merged<7, a8 1>", 2, 0, 1, true},
    {"merge: single row 4 steps, merge_single=3", F(c3_shard(4)), H(k.merge_single = 3), "even<512, 4, sh 1, sg 0, a8 1>", 2, 1, 0, true},
    {"merge: merged round 7 steps, merge_u=7", F(c3_shard(4)), H(k.merge_u = 7), "merged<7, a8 1>", 2, 0, 1, true},
    {"merge: merged round 7 steps, merge_u=6", F(c3_shard(4)), H(k.merge_u = 6), "even<512, 4, sh 1, sg 0, a8 1>", 2, 1, 0, true},
    {"merge: four rows allowed, four fit", F(c3_shard(8), f.max_merge_log2 = 2), H(), "merged<7, a8 1>", 2, 0, 2, true},
    {"merge: four rows allowed, two fit", F(c3_shard(4), f.max_merge_log2 = 2), H(), "merged<7, a8 1>", 2, 0, 1, true},
    {"merge: none allowed", F(c3_shard(8), f.max_merge_log2 = 0), H(), "even<512, 2, sh 1, sg 0, a8 1>", 2, 2, 0, true},
    {"merge: staging two rows of 70 terms takes 3 waves", F(c3_shard(2)), H(), "even<512, 7, sh 1, sg 0, a8 1>", 2, 0, 0, true},
    // two planes: chunks of kPlanesMinChunk rounds, room for byte sums, tiles of a plane's size, the handle's latch
    {"planes: chunks of 255 rounds", F(c3(), f.q_chunk = 255), H(), "even<512, 6, sh 0, sg 0, a8 0>", 2, 0, 0, true},
    {"planes: chunks of 256 rounds", F(c3(), f.q_chunk = 256), H(), "planes<6>", 2, 0, 0, true},
    {"planes: no room for byte sums", F(c3(), f.planes_scale = 0.0), H(), "even<512, 6, sh 0, sg 0, a8 0>", 2, 0, 0, true},
    {"planes: cb 32768", F(c3()), H(), "planes<6>", 2, 0, 0, true},
    {"planes: cb 65536 with 8-bit sums", F(c3(), f.cb = 65536; f.acc8 = true; f.n_tiles = 16), H(), "coarse<512, 5, sh 0, ch 16, vr 0, sg 0, lp 0, a8 1>", 0, 0, 0, true},
    {"planes: cb 65536 without", F(c3(), f.cb = 65536; f.n_tiles = 16), H(), "even<1024, 6, sh 0, sg 0, a8 0>", 4, 1, 0, true},
    {"planes: latched off", F(c3(), f.no_acc8 = true), H(), "even<512, 6, sh 0, sg 0, a8 0>", 2, 0, 0, true},
    {"planes: not on a term shard", F(c3_shard16(8), f.planes_scale = 64.0; f.no_acc8 = false; f.max_merge_log2 = 0), H(), "even<512, 2, sh 1, sg 0, a8 0>", 2, 2, 0, true},
    // every filter token alone
    {"chunk8", F(c3()), H(k.chunk8 = true), "coarse<512, 4, sh 0, ch 8, vr 0, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"chunk8 on a term shard", F(c3_shard16(4)), H(k.chunk8 = true), "coarse<512, 4, sh 1, ch 8, vr 0, sg 0, lp 0, a8 0>", 0, 0, 0, false},
    {"window=2", F(c3()), H(k.window = 2), "coarse<512, 2, sh 0, ch 16, vr 0, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"window=5", F(c3()), H(k.window = 5), "coarse<512, 5, sh 0, ch 16, vr 0, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"window=6", F(c3()), H(k.window = 6), "coarse<512, 6, sh 0, ch 16, vr 0, sg 0, lp 0, a8 0>", 0, 0, 0, false},
    {"window=3 on a term shard", F(c3_shard16(4)), H(k.window = 3), "coarse<512, 3, sh 1, ch 16, vr 0, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"window=3, 1024 threads ignore it", F(c5s()), H(k.window = 3), "coarse<1024, 5, sh 0, ch 16, vr 0, sg 0, lp 0, a8 1>", 0, 0, 0, true},
    {"window=3 keeps the long tail's kernel out", F(power_law_tail(200.0), f.acc8 = false; f.cb = 32768; f.max_seg = 257), H(k.window = 3), "coarse<512, 3, sh 1, ch 16, vr 0, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"no_acc8", F(c3()), H(k.no_acc8 = true), "even<512, 6, sh 0, sg 0, a8 0>", 2, 0, 0, true},
    {"no_planes", F(c3()), H(k.no_planes = true), "even<512, 6, sh 0, sg 0, a8 0>", 2, 0, 0, true},
    {"planes, chunks of 6 rounds", F(c3(), f.q_chunk = 6), H(k.planes = true), "planes<6>", 2, 0, 0, true},
    {"planes, no room for byte sums", F(c3(), f.planes_scale = 0.0), H(k.planes = true), "even<512, 6, sh 0, sg 0, a8 0>", 2, 0, 0, true},
    {"flat_group=0", F(c3_shard(8)), H(k.flat_group = 0), "merged<3, a8 1>", 1, 0, 1, true},
    {"flat_group=1", F(c3_shard(8)), H(k.flat_group = 1), "merged<4, a8 1>", 2, 1, 1, true},
    {"no_even", F(c3()), H(k.no_even = true), "coarse<512, 5, sh 0, ch 16, vr 0, sg 0, lp 0, a8 0>", 0, 0, 0, true},
    {"no_even on a term shard", F(c3_shard(8)), H(k.no_even = true), "coarse<512, 2, sh 1, ch 16, vr 0, sg 0, lp 0, a8 1>", 0, 0, 0, true},
    {"merge_u=3", F(c3_shard(8)), H(k.merge_u = 3), "even<512, 2, sh 1, sg 0, a8 1>", 2, 2, 0, true},
    {"merge_single=1", F(c3_shard(8)), H(k.merge_single = 1), "even<512, 2, sh 1, sg 0, a8 1>", 2, 2, 0, true},
    // the shapes the project quotes
    {"C3 plain: six adding waves x 6 steps", F(c3()), H(), "planes<6>", 2, 0, 0, true},
    {"C3 plain, a streamed batch: chunks of 64 rounds", F(c3(), f.nq = 16384; f.s_nnz_end = 1638400; f.q_chunk = 64), H(), "even<512, 6, sh 0, sg 0, a8 0>", 2, 0, 0, true},
    {"C3 shard T = 2", F(c3_shard(2)), H(), "even<512, 7, sh 1, sg 0, a8 1>", 2, 0, 0, true},
    {"C3 shard T = 4", F(c3_shard(4)), H(), "merged<7, a8 1>", 2, 0, 1, true},
    {"C3 shard T = 8", F(c3_shard(8)), H(), "merged<4, a8 1>", 2, 1, 1, true},
    {"C3 shard T = 2, 16-bit sums", F(c3_shard16(2)), H(), "even<512, 4, sh 1, sg 0, a8 0>", 2, 0, 0, true},
    {"C3 shard T = 8, four rows per round", F(c3_shard(8), f.max_merge_log2 = 2), H(), "merged<7, a8 1>", 2, 0, 2, true},
    {"C5 sparse", F(c5s()), H(), "even<1024, 5, sh 0, sg 0, a8 1>", 4, 0, 0, true},
    {"C5 sparse, latched back to 65536-row tiles", F(c5s(), f.acc8 = false; f.cb = 65536; f.n_tiles = 31; f.no_acc8 = true), H(), "even<1024, 3, sh 0, sg 0, a8 0>", 4, 0, 0, true},
    {"power-law tail: 85 chunks estimated", F(power_law_tail(0.0)), H(), "even<512, 5, sh 1, sg 0, a8 1>", 2, 0, 0, true},
    {"power-law tail: 200 dealt out", F(power_law_tail(200.0)), H(), "even<512, 6, sh 1, sg 0, a8 1>", 2, 0, 0, true},
    {"even_wipe: dim 8000 takes five steps", F(wipe(8000)), H(k.planes = true), "planes<5>", 2, 0, 0, true},
    {"even_wipe: dim 6800 takes six steps", F(wipe(6800)), H(k.planes = true), "planes<6>", 2, 0, 0, true},
    {"even_wipe: dim 8000, no_planes", F(wipe(8000)), H(k.no_planes = true), "even<512, 5, sh 0, sg 0, a8 0>", 2, 0, 0, true},
    {"even_wipe: dim 6800, no_planes", F(wipe(6800)), H(k.no_planes = true), "even<512, 6, sh 0, sg 0, a8 0>", 2, 0, 0, true},
};

// ... and the diag lines of some of them (a row that never weighs k_probe_even prints none)
struct DiagRow {
  const char *row, *text;
};
const DiagRow kDiagRows[] = {
    {"staging: 129 terms, 3 waves", ""},
    {"steps: 6 x 6 = 36 > 8 x 4", "[apss diag] even? merge 1 block 512 u 4 | F 2 G 1 A 6 chunks 248.4 ue 6 fits 0 exists 1 q_max 80 q_terms 80.0 seg 39.3\n"},
    {"C3 plain: six adding waves x 6 steps", "[apss diag] even? merge 1 block 512 u 5 | F 2 G 1 A 6 chunks 267.5 ue 6 fits 1 exists 1 q_max 100 q_terms 100.0 seg 32.8\n"},
    {"C3 shard T = 8", "[apss diag] even? merge 1 block 512 u 2 | F 2 G 4 A 6 chunks 90.2 ue 2 fits 1 exists 1 q_max 30 q_terms 12.5 seg 8.2\n[apss diag] even? merge 2 block 512 u 2 | F 2 G 2 A 6 chunks 161.2 ue 4 fits 1 exists 1 q_max 30 q_terms 12.5 seg 8.2\n"},
    {"C3 shard T = 8, four rows per round", "[apss diag] even? merge 1 block 512 u 2 | F 2 G 4 A 6 chunks 90.2 ue 2 fits 1 exists 1 q_max 30 q_terms 12.5 seg 8.2\n[apss diag] even? merge 2 block 512 u 2 | F 2 G 2 A 6 chunks 161.2 ue 4 fits 1 exists 1 q_max 30 q_terms 12.5 seg 8.2\n[apss diag] even? merge 4 block 512 u 4 | F 2 G 1 A 6 chunks 295.3 ue 7 fits 1 exists 1 q_max 30 q_terms 12.5 seg 8.2\n"},
    {"C5 sparse", "[apss diag] even? merge 1 block 1024 u 5 | F 4 G 1 A 12 chunks 449.1 ue 5 fits 1 exists 1 q_max 200 q_terms 200.0 seg 26.2\n"},
    {"power-law tail: 200 dealt out", "[apss diag] even? merge 1 block 512 u 2 | F 2 G 1 A 6 chunks 249.2 ue 6 fits 1 exists 1 q_max 120 q_terms 66.0 seg 4.3\n"},
    {"even_wipe: dim 8000 takes five steps", "[apss diag] even? merge 1 block 512 u 4 | F 2 G 1 A 6 chunks 220.5 ue 5 fits 1 exists 1 q_max 100 q_terms 100.0 seg 25.6\n"},
    {"even_wipe: dim 6800 takes six steps", "[apss diag] even? merge 1 block 512 u 5 | F 2 G 1 A 6 chunks 250.1 ue 6 fits 1 exists 1 q_max 100 q_terms 100.0 seg 30.1\n"},
};

struct ScaleRow {
  const char *name;
  double bound, shared, theta, scale;
};
// acc8_scale(bound, shared, theta): k = 7, 6, 5 by the norm bound, by 255 - shared, and the floor of 12 units above the slack
const ScaleRow kScale8Rows[] = {
    {"k 7: unit norms", 1.0001, 100, 0.8, 128.0},
    {"k 6: bound 1.5", 1.5, 100, 0.8, 64.0},
    {"k 5: bound 3", 3.0, 100, 0.8, 32.0},
    {"none: bound 5", 5.0, 100, 0.8, 0.0},
    {"k 7: 126 shared terms", 1.0001, 126, 0.8, 128.0},
    {"k 6: 127 shared terms", 1.0001, 127, 0.8, 64.0},
    {"k 6: 190 shared terms", 1.0001, 190, 0.8, 64.0},
    {"k 5: 191 shared terms", 1.0001, 191, 0.8, 32.0},
    {"k 5: 222 shared terms", 1.0001, 222, 0.8, 32.0},
    {"none: 223 shared terms", 1.0001, 223, 0.8, 0.0},
    {"floor: theta 0.110 leaves 14 units at k 7", 1.0001, 100, 0.110, 128.0},
    {"floor: theta 0.109 leaves 13", 1.0001, 100, 0.109, 0.0},
    {"floor: k 6 by the bound, theta 0.219 leaves 14", 1.5, 100, 0.219, 64.0},
    {"floor: k 6 by the bound, theta 0.218 leaves 13", 1.5, 100, 0.218, 0.0},
    {"floor: k 5 by the bound, theta 0.438 leaves 14", 3.0, 100, 0.438, 32.0},
    {"floor: k 5 by the bound, theta 0.437 leaves 13", 3.0, 100, 0.437, 0.0},
};
struct Scale16Row {
  const char *name;
  double bound, shared, theta, scale;
  bool selective;
};
// acc16_scale(bound, shared, theta): every k, and the selectivity test below 16384 units
const Scale16Row kScale16Rows[] = {
    {"k 15: unit norms", 1.0001, 100, 0.8, 32768.0, true},
    {"k 14: bound 2.5", 2.5, 100, 0.8, 16384.0, true},
    {"k 13: bound 4", 4.0, 100, 0.8, 8192.0, true},
    {"k 12: bound 8", 8.0, 100, 0.8, 4096.0, true},
    {"k 11: bound 16", 16.0, 100, 0.8, 2048.0, true},
    {"k 10: bound 32", 32.0, 100, 0.8, 1024.0, true},
    {"k 9: bound 64", 64.0, 100, 0.8, 512.0, true},
    {"k 8: bound 128", 128.0, 100, 0.8, 256.0, false},
    {"k 7: bound 256", 256.0, 100, 0.8, 128.0, false},
    {"k 6: bound 512", 512.0, 100, 0.8, 64.0, false},
    {"k 5: bound 1024", 1024.0, 100, 0.8, 32.0, false},
    {"k 5: bound 2000", 2000.0, 100, 0.8, 32.0, false},
    {"k 4: bound 2048", 2048.0, 100, 0.8, 16.0, false},
    {"k 4: bound 4000", 4000.0, 100, 0.8, 16.0, false},
    {"none: bound 4096", 4096.0, 100, 0.8, 0.0, false},
    {"none, no shared terms", 4096.0, 0, 0.8, 0.0, true},
    {"k 15 by one shared term less", 1.9988, 5, 0.8, 32768.0, true},
    {"k 14 by one shared term more", 1.9988, 6, 0.8, 16384.0, true},
    {"selective at 16384 units whatever the terms", 2.5, 5000, 0.8, 16384.0, true},
    {"selective: 8192 units, 6550 >= 4 x 1637", 4.0, 1637, 0.8, 8192.0, true},
    {"not selective: 8192 units, 6550 < 4 x 1638", 4.0, 1638, 0.8, 8192.0, false},
};
struct MergedRow {
  const char *name;
  bool acc8;
  double bound, shared, theta;
  int m;
  double scale;
};
// merged_scale(acc8, bound, shared, theta, m): the scale of M rows
const MergedRow kMergedRows[] = {
    {"8-bit, two rows of C3's T = 8 shard", true, 1.0001, 30, 0.8, 1, 64.0},
    {"8-bit, four rows", true, 1.0001, 30, 0.8, 2, 32.0},
    {"8-bit, two rows of 70 terms", true, 1.0001, 70, 0.8, 1, 32.0},
    {"8-bit, four rows of 70 terms: no room", true, 1.0001, 70, 0.8, 2, 0.0},
    {"8-bit, four rows, theta 0.44: 14 units", true, 1.0001, 30, 0.44, 2, 32.0},
    {"8-bit, four rows, theta 0.43: 13 units", true, 1.0001, 30, 0.43, 2, 0.0},
    {"16-bit, two rows", false, 1.0001, 70, 0.8, 1, 16384.0},
    {"16-bit, four rows: 8192 units, selective", false, 1.0001, 70, 0.8, 2, 8192.0},
    {"16-bit, four rows of 410 terms: 6550 < 6560", false, 1.0001, 410, 0.8, 2, 0.0},
    {"16-bit, four rows of 409 terms: 6550 >= 6544", false, 1.0001, 409, 0.8, 2, 8192.0},
};

// C3's store: a million unit rows of 100 terms over 100,000, theta 0.8
// TileFacts: rows, nnz, max_nnz, max_norm2 | sharded, head_k, head_longseg, nonneg, no_acc8 | theta, dim
TileFacts c3_store() { return {1000000, 100000000, 100, 1.0f, false, 0, false, true, false, 0.8, 100000}; }
#define T(base, ...) ([] { TileFacts s = base; __VA_ARGS__; return s; }())
struct TileRow {
  const char *name;
  TileFacts s;
  FilterHooks k;
  int32_t cb;
};
// pick_cx_tile: 16 and 8 postings per (32768-row tile, term), the shard / dense-head branch
const TileRow kTileRows[] = {
    {"C3: 32.8 postings", T(c3_store()), H(), 32768},
    {"seg32 16.0", T(c3_store(), s.nnz = 48828125), H(), 32768},
    {"seg32 just below 16", T(c3_store(), s.nnz = 48828124), H(), 65536},
    {"seg32 just below 16, term shard", T(c3_store(), s.nnz = 48828124; s.sharded = true; s.max_nnz = 300), H(), 32768},
    {"seg32 just below 16, dense-head block", T(c3_store(), s.nnz = 48828124; s.head_k = 256; s.max_nnz = 300), H(), 32768},
    {"seg32 just above 8", T(c3_store(), s.nnz = 24414063), H(), 65536},
    {"seg32 just below 8", T(c3_store(), s.nnz = 24414062), H(), 131072},
    {"seg32 just below 8, a negative weight", T(c3_store(), s.nnz = 24414062; s.nonneg = false), H(), 65536},
    {"seg32 just below 8, latched", T(c3_store(), s.nnz = 24414062; s.no_acc8 = true), H(), 65536},
    {"seg32 just below 8, no_acc8", T(c3_store(), s.nnz = 24414062), H(k.no_acc8 = true), 65536},
    {"seg32 just below 8, longest row 223: no room", T(c3_store(), s.nnz = 24414062; s.max_nnz = 223), H(), 65536},
    {"seg32 just below 8, longest row 222", T(c3_store(), s.nnz = 24414062; s.max_nnz = 222), H(), 131072},
    {"seg32 just below 8, norms of 2.3: no room", T(c3_store(), s.nnz = 24414062; s.max_norm2 = 5.3f), H(), 65536},
    {"C5 sparse: 6.6 postings", T(c3_store(), s.rows = 2000000; s.nnz = 400000000; s.max_nnz = 200; s.dim = 1000000; s.theta = 0.9), H(), 131072},
    {"term shard", T(c3_store(), s.sharded = true), H(), 65536},
    {"term shard, a negative weight", T(c3_store(), s.sharded = true; s.nonneg = false), H(), 65536},
    {"term shard, no room", T(c3_store(), s.sharded = true; s.max_nnz = 223), H(), 32768},
    {"term shard, latched", T(c3_store(), s.sharded = true; s.no_acc8 = true), H(), 32768},
    {"term shard, no_acc8", T(c3_store(), s.sharded = true), H(k.no_acc8 = true), 32768},
    {"dense-head block", T(c3_store(), s.head_k = 256), H(), 65536},
    {"dense-head block, long segments in the tail", T(c3_store(), s.head_k = 256; s.head_longseg = true), H(), 32768},
    {"term shard with a block", T(c3_store(), s.sharded = true; s.head_k = 128), H(), 65536},
    {"term shard with a block, long segments in the tail", T(c3_store(), s.sharded = true; s.head_k = 128; s.head_longseg = true), H(), 32768},
    {"term shard, long segments flagged without a block", T(c3_store(), s.sharded = true; s.head_longseg = true), H(), 65536},
};
struct MergeRow {
  const char *name;
  int64_t nq, s_nnz_end;
  int32_t term_lo, term_hi;
  bool acc8;
  double bound, shared, theta;
  FilterHooks k;
  int m;
};
// merge_rows_log2(nq, s_nnz_end, term_lo, term_hi, acc8, bound, shared, theta): t >= 8 terms of a row in the shard, M t^2 <= 0.25 R for the M = 2, 4 rows of a round
const MergeRow kMergeRows[] = {
    {"C3 shard T = 8: t 12.5, R 12500", 1000000, 12500000, 12500, 25000, true, 1.0001, 30, 0.8, H(), 1},
    {"C3 shard T = 2: t 50, R 50000", 1000000, 50000000, 0, 50000, true, 1.0001, 70, 0.8, H(), 1},
    {"t 8.0", 1000000, 8000000, 0, 12500, true, 1.0001, 30, 0.8, H(), 1},
    {"t just below 8", 1000000, 7999999, 0, 12500, true, 1.0001, 30, 0.8, H(), 0},
    {"2 x 625 = 0.25 x 5000", 1000000, 25000000, 0, 5000, true, 1.0001, 45, 0.8, H(), 1},
    {"2 x 625 > 0.25 x 4999", 1000000, 25000000, 0, 4999, true, 1.0001, 45, 0.8, H(), 0},
    {"merge=2: 4 x 156.25 = 0.25 x 2500", 1000000, 12500000, 0, 2500, true, 1.0001, 30, 0.8, H(k.merge = 2), 2},
    {"merge=2: 4 x 156.25 > 0.25 x 2499", 1000000, 12500000, 0, 2499, true, 1.0001, 30, 0.8, H(k.merge = 2), 1},
    {"merge=2", 1000000, 12500000, 12500, 25000, true, 1.0001, 30, 0.8, H(k.merge = 2), 2},
    {"merge=3 is merge=2", 1000000, 12500000, 12500, 25000, true, 1.0001, 30, 0.8, H(k.merge = 3), 2},
    {"merge=2, four rows of 70 terms have no room", 1000000, 50000000, 0, 50000, true, 1.0001, 70, 0.8, H(k.merge = 2), 1},
    {"merge=0", 1000000, 12500000, 12500, 25000, true, 1.0001, 30, 0.8, H(k.merge = 0), 0},
    {"merge=1", 1000000, 12500000, 12500, 25000, true, 1.0001, 30, 0.8, H(k.merge = 1), 1},
    {"one query row", 1, 13, 12500, 25000, true, 1.0001, 30, 0.8, H(), 0},
    {"two query rows", 2, 25, 12500, 25000, true, 1.0001, 30, 0.8, H(), 1},
    {"merge=2, three query rows", 3, 38, 12500, 25000, true, 1.0001, 30, 0.8, H(k.merge = 2), 1},
    {"merge=2, four query rows", 4, 50, 12500, 25000, true, 1.0001, 30, 0.8, H(k.merge = 2), 2},
    {"no query row", 0, 0, 12500, 25000, true, 1.0001, 30, 0.8, H(), 0},
    {"16-bit sums, two rows of 410 shared terms are not selective", 1000000, 12500000, 12500, 25000, false, 4.0, 410, 0.8, H(), 0},
    {"16-bit sums, two rows of 409 are", 1000000, 12500000, 12500, 25000, false, 4.0, 409, 0.8, H(), 1},
};

// ---- the sweep: the grid's plans without a listed variant, by the variant they arrive at, with how many combinations do:
// chunk8 has one instantiation (512 threads, no shard rule, no virtual rows), and virtual rows of signed weights have none under the shard rule
struct Unlisted {
  const char *variant;
  int combinations;
};
const Unlisted kUnlisted[] = {
    {"coarse<1024, 4, sh 0, ch 8, vr 0, sg 0, lp 0, a8 0>", 1440},
    {"coarse<1024, 4, sh 0, ch 8, vr 1, sg 0, lp 0, a8 0>", 32},
    {"coarse<512, 4, sh 0, ch 8, vr 1, sg 0, lp 0, a8 0>", 64},
    {"coarse<512, 4, sh 1, ch 8, vr 0, sg 0, lp 0, a8 0>", 7776},
    {"coarse<512, 5, sh 1, ch 16, vr 1, sg 1, lp 0, a8 0>", 576},
    {"coarse<512, 5, sh 1, ch 8, vr 0, sg 0, lp 1, a8 0>", 2592},
    {"coarse<512, 5, sh 1, ch 8, vr 1, sg 0, lp 1, a8 0>", 384},
};
constexpr long long kSweepCombinations = 309408;
constexpr unsigned long long kSweepHash = 14155001304634968603ULL;
// listed variants that neither the table nor the grid reaches, with what was tried (none)
const char *const kNotReached[] = {nullptr};

int failures = 0;
#define CHECK(ok, ...)                   \
  if (!(ok)) {                           \
    ++failures;                          \
    std::fprintf(stderr, "FAIL " __VA_ARGS__); \
    std::fprintf(stderr, "\n");          \
  }

}  // namespace

int main() {
  std::set<std::string> reached;
  int traced = 0;
  for (const PlanRow &r : kPlanRows) {
    CHECK(valid(r.f, r.k), "%s: facts that choose_path cannot hand over", r.name);
    std::string text;
    const apss::FilterPlan p = apss::plan_filter(r.f, r.k, &text);
    const std::string got = variant_name(p.v);
    CHECK(got == r.variant && p.flat_waves == r.flat_waves && p.flat_group_log2 == r.flat_group_log2 && p.merge_log2 == r.merge_log2 && p.listed == r.listed,
          "%s: %s, F %d, G 2^%d, rows 2^%d, listed %d; expected %s, %d, %d, %d, %d", r.name, got.c_str(), (int)p.flat_waves, (int)p.flat_group_log2, (int)p.merge_log2,
          (int)p.listed, r.variant, r.flat_waves, r.flat_group_log2, r.merge_log2, (int)r.listed);
    if (p.listed) reached.insert(got);
    for (const DiagRow &d : kDiagRows) {
      if (std::strcmp(d.row, r.name)) continue;
      ++traced;
      CHECK(text == d.text, "diag of %s:\n%s-- expected:\n%s", r.name, text.c_str(), d.text);
    }
  }
  CHECK(traced == (int)(sizeof kDiagRows / sizeof kDiagRows[0]), "%d of the diag rows found", traced);
  for (const ScaleRow &r : kScale8Rows) {
    const double s = apss::acc8_scale(r.bound, r.shared, r.theta);
    CHECK(s == r.scale, "acc8_scale, %s: %.1f; expected %.1f", r.name, s, r.scale);
  }
  for (const Scale16Row &r : kScale16Rows) {
    const apss::Scale16 s = apss::acc16_scale(r.bound, r.shared, r.theta);
    CHECK(s.scale == r.scale && s.selective == r.selective, "acc16_scale, %s: %.1f, selective %d; expected %.1f, %d", r.name, s.scale, (int)s.selective, r.scale, (int)r.selective);
  }
  for (const MergedRow &r : kMergedRows) {
    const double s = apss::merged_scale(r.acc8, r.bound, r.shared, r.theta, r.m);
    CHECK(s == r.scale, "merged_scale, %s: %.1f; expected %.1f", r.name, s, r.scale);
  }
  for (const TileRow &r : kTileRows) {
    const int32_t cb = apss::pick_cx_tile(r.s, r.k);
    CHECK(cb == r.cb, "pick_cx_tile, %s: %d; expected %d", r.name, (int)cb, (int)r.cb);
  }
  for (const MergeRow &r : kMergeRows) {
    const int m = apss::merge_rows_log2(r.nq, r.s_nnz_end, r.term_lo, r.term_hi, r.acc8, r.bound, r.shared, r.theta, r.k);
    CHECK(m == r.m, "merge_rows_log2, %s: %d; expected %d", r.name, m, r.m);
  }
  // the threshold is the one formula: theta * S * (1 - 2^-11 - 1e-6), rounded down
  CHECK(apss::filter_threshold(0.8, 32768.0) == 26201.0 && apss::filter_threshold(0.8, 128.0) == 102.0 && apss::filter_threshold(0.5, 0.0) == 0.0,
        "filter_threshold: %.1f, %.1f", apss::filter_threshold(0.8, 32768.0), apss::filter_threshold(0.8, 128.0));

  // ---- the sweep
  std::map<std::string, int> unlisted;
  PlanHash hash;
  long long n = 0;
  for_each_grid([&](const GridPoint &g, const FilterFacts &f, const FilterHooks &k) {
    const apss::FilterPlan p = apss::plan_filter(f, k);
    hash.add(p);
    ++n;
    const std::string name = variant_name(p.v);
    if (p.listed) reached.insert(name);
    else if (++unlisted[name] == 1) std::printf("not listed: %s, e.g. %s\n", name.c_str(), grid_name(g, f).c_str());
  });
  CHECK(n == kSweepCombinations, "the grid has %lld combinations; expected %lld", n, kSweepCombinations);
  CHECK(hash.h == kSweepHash, "the grid's decisions hash to %llu; expected %llu", (unsigned long long)hash.h, kSweepHash);
  for (const Unlisted &u : kUnlisted) {
    CHECK(unlisted.count(u.variant) && unlisted[u.variant] == u.combinations, "%s: %d combinations without a listed variant; expected %d", u.variant,
          unlisted.count(u.variant) ? unlisted[u.variant] : 0, u.combinations);
    unlisted.erase(u.variant);
  }
  for (const auto &u : unlisted) CHECK(false, "%s: %d combinations without a listed variant; expected none", u.first.c_str(), u.second);
  // ---- every listed variant is reached
  int n_listed = 0;
  const auto want = [&](const CxVariant &v) {
    ++n_listed;
    const std::string name = variant_name(v);
    bool excused = false;
    for (const char *e : kNotReached) excused = excused || (e && name == e);
    CHECK(apss::filter_variant_listed(v), "%s is in a table and not listed", name.c_str());
    CHECK(reached.count(name) || excused, "%s is listed and no row or grid point reaches it", name.c_str());
  };
#define X(U) want(CxVariant{512, U, false, 16, false, false, false, true, true, false, true});
  APSS_EVEN_PLANES_VARIANTS(X)
#undef X
#define X(U, A8) want(CxVariant{512, U, true, 16, false, false, false, A8, true, true, false});
  APSS_EVEN_MERGE_VARIANTS(X)
#undef X
#define X(B, U, SH, SG, A8) want(CxVariant{B, U, SH, 16, false, SG, false, A8, true, false, false});
  APSS_EVEN_VARIANTS(X)
#undef X
#define X(B, U, SH, CH, VR, SG, LP, A8) want(CxVariant{B, U, SH, CH, VR, SG, LP, A8, false, false, false});
  APSS_CX_VARIANTS(X)
#undef X
  CHECK((int)reached.size() == n_listed, "%d variants reached, %d listed", (int)reached.size(), n_listed);
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("filter plan selftest ok: %d plan rows, %d diag rows, %d scale rows, %d tile rows, %d merge rows, %lld grid points, %d variants reached\n",
              (int)(sizeof kPlanRows / sizeof kPlanRows[0]), traced,
              (int)(sizeof kScale8Rows / sizeof kScale8Rows[0] + sizeof kScale16Rows / sizeof kScale16Rows[0] + sizeof kMergedRows / sizeof kMergedRows[0]),
              (int)(sizeof kTileRows / sizeof kTileRows[0]), (int)(sizeof kMergeRows / sizeof kMergeRows[0]), n, n_listed);
  return 0;
}
