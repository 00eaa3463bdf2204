// The PLAN of the two-pass join's filter: which instantiation of the filter kernel a call takes -- workgroup size, register
// window, staging waves, query rows per round -- the accumulator scales it counts in, and the rows per tile of the coarse
// rendering it runs over.  Plain C++ (no HIP): choose_path, plan_merged_rounds and build_index fill the fact structs and decide
// with it (apss_hip.hip), and host/filter_plan_selftest.cpp checks the rule on both sides of every threshold.  A wrong choice
// still returns the right pairs, only slower.  The kernels are in apss_kernels.hpp (k_probe_coarse) and apss_even.hpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

namespace apss {

constexpr int kWave = 64;             // CDNA wavefront
constexpr int kLongLenW = 256;        // longer segments are swept by the whole workgroup
constexpr int kPlanesMinChunk = 256;  // k_probe_planes: query chunks of this many rounds or more (plan_filter)

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the filter tokens of APSS_DEBUG (DebugCfg, apss_hip.hip, has the others)
struct FilterHooks {
  bool chunk8 = false;     // chunk8         filter kernel with 8-posting chunks (4-step window)
  int window = 0;          // window=U       register-window steps of the 512-thread filter kernel (2..5)
  bool no_acc8 = false;    // no_acc8        term shards keep 16-bit accumulators over 32768-row tiles
  bool no_planes = false;  // no_planes      a plain 512-thread handle keeps k_probe_even's 16-bit sums and two barriers per round (never k_probe_planes); no_acc8 implies it
  bool planes = false;     // planes         ... and takes k_probe_planes whatever the length of its query chunks (default: chunks of kPlanesMinChunk rounds or more)
  int flat_group = -1;     // flat_group=L   k_probe_even: 2^L staging lanes per term (default: as many as keep the staging waves <= 1/4)
  bool no_even = false;    // no_even        the filter stages every round on all waves (k_probe_coarse), never on F of them (k_probe_even)
  int merge = -1;          // merge=L        a term shard's thin rounds: at most 2^L query rows share a round (0: never; default 1: two rows)
  int merge_u = 0;         // merge_u=U      ... as long as the merged round fits a window of U steps (default 7)
  int merge_single = 0;    // merge_single=U ... and a single row's round takes a window of at most U steps (default 4)
};

// ---- scales ----
// theta in the units of a filter that counts S units per 1.0: the coarse threshold before the per-query slack (fp16 weights: 2^-11)
inline double filter_threshold(double theta, double S) { return std::floor(theta * S * (1.0 - 1.0 / 2048 - 1e-6)); }

// 8-bit accumulator scale of a term shard: the largest S = 2^k <= 2^7 with  S * max|q||c| * 1.0005 + shared terms < 2^8  (no
// carry into the neighbour's byte), taken only while the threshold in units stays well above what a chance pair collects
// (one unit of round-up per shared term).  0: not usable.
inline double acc8_scale(double bound, double shared, double theta) {
  for (int k = 7; k >= 5; --k) {
    const double S = std::ldexp(1.0, k);
    if (bound * 1.0005 * S < 255.0 - shared && filter_threshold(theta, S) - 2 >= 12.0) return S;
  }
  return 0.0;
}

// accumulator units per 1.0 of the 16-bit filter: a sum holds S * |q||c| (fp16 weights: + 2^-11) plus one unit per shared term.
// S = the largest power of two that fits (2^15 for unit-norm input; 0: none); un-normalised input gets a smaller one, SELECTIVE
// only as long as the threshold in units stays well above the round-up bias (one unit per shared term), else the filter passes too much
struct Scale16 {
  double scale;
  bool selective;
};
inline Scale16 acc16_scale(double bound, double shared, double theta) {
  double S = 0.0;
  for (int k = 15; k >= 4 && S == 0.0; --k)
    if (bound * 1.0005 * std::ldexp(1.0, k) < 65535.0 - shared) S = std::ldexp(1.0, k);
  return {S, S >= 16384.0 || filter_threshold(theta, S) >= 4.0 * shared};
}

// MERGED rounds (a term shard's thin rounds, apss_even.hpp): M = 2^m neighbouring query rows share a round, their M filter sums one
// accumulator -- which then has to hold M sums: the scale for M rows is the scale of one row with M times the norm bound and
// M times the shared terms (0: the accumulators have no room for M rows).  acc8: the call counts in 8-bit sums.
inline double merged_scale(bool acc8, double bound, double shared, double theta, int m) {
  const double Mx = (double)(1 << m);
  if (acc8) return acc8_scale(bound * Mx, shared * Mx, theta);
  const Scale16 s = acc16_scale(bound * Mx, shared * Mx, theta);
  return s.selective ? s.scale : 0.0;
}

// ---- rows per tile of the coarse rendering when the handle chooses them (no tile_rows, no cx_tile), from the store's shape ----
struct TileFacts {
  int64_t rows, nnz, max_nnz;  // the store: rows, entries, the longest row
  float max_norm2;             // its largest squared row norm
  bool sharded;
  int32_t head_k;              // columns of the dense-head block (0: none)
  bool head_longseg, nonneg, no_acc8;  // its tail proved to hold long segments; every stored weight so far is >= 0; the handle's latch (FilterFacts)
  double theta;
  int32_t dim;
};
inline int32_t pick_cx_tile(const TileFacts &s, const FilterHooks &k) {
  // a round's cost is mostly fixed, so what matters is how many postings a (tile, term) segment holds:
  // rows_per_tile * nnz_per_row / dim.  Below ~16 at 32768 rows (C5 shape: 6.5) the 65536-row tile with one
  // 1024-thread workgroup per CU wins (C5 shape at N=2M: 647 vs 790 ms); at C3 (33) two workgroups per CU win.
  const double seg32 = 32768.0 * ((double)s.nnz / (double)s.rows) / (double)s.dim;
  int32_t cb = seg32 < 16.0 && !s.sharded && !s.head_k ? 65536 : 32768;  // (the 1024-thread kernel has no shard variant)
  const bool room8 = !k.no_acc8 && !s.no_acc8 && acc8_scale((double)s.max_norm2 * 1.0001 + 1e-6, (double)s.max_nnz, s.theta) > 0;
  // sparser still (C5: 6.5): 131072-row tiles with 8-bit accumulators (k_probe_coarse<1024, .., ACC8>) when the norms and
  // row lengths leave room for them: half the segment-descriptor look-ups and half the half-empty posting lines
  if (cb == 65536 && seg32 < 8.0 && s.nonneg && s.max_nnz <= 512 && room8) cb = 131072;
  // a term shard's rounds are thin (1/T of every query's terms): 8-bit accumulators hold 65536 candidates in the same
  // 64 KB, i.e. half the rounds at the same two workgroups per CU -- when the norms and row lengths leave room for them
  // (with a dense-head block: only while the tail has no long segments -- the prefetched long-segment sweeps exist for
  // 16-bit accumulators over 32768-row tiles only; known after the build, so an optimistic first build may be repeated)
  if ((s.sharded || s.head_k) && !(s.head_k && s.head_longseg) && room8) cb = 65536;
  return cb;
}

// ---- how many query rows may share a round of a term shard: 2^(the result), as many as the accumulators have room for AND the
// filter stays SELECTIVE with: a chance pair collects about 1 / t of the threshold's scale per shared term (t = terms of a row
// inside this shard), and a round of M rows hits a given candidate M t^2 / R times on average (R = terms of the range).  Rows of a
// dozen terms over thousands of terms (C3's shards: t = 12.5, R = 12500): a chance candidate is hit once, by one row.  Rows of
// three or four terms over a few hundred: three chance hits from different rows of a round cross the threshold (measured: 8 x
// more candidates than unmerged) -- not there.  (plan_filter decides how many rows a window has.)
inline int merge_rows_log2(int64_t nq, int64_t s_nnz_end, int32_t term_lo, int32_t term_hi, bool acc8, double bound, double shared,
                           double theta, const FilterHooks &k) {
  const double t_shard = (double)s_nnz_end / (double)std::max<int64_t>(nq, 1);
  const double r_shard = (double)std::max<int64_t>(1, (int64_t)term_hi - term_lo);
  int m = 0;
  if (k.merge != 0 && t_shard >= 8.0)
    while (m < (k.merge > 0 ? std::min(k.merge, 2) : 1) && (nq >> (m + 1)) >= 1 && (double)(2 << m) * t_shard * t_shard <= 0.25 * r_shard &&
           merged_scale(acc8, bound, shared, theta, m + 1) > 0)
      ++m;
  return m;
}

// ---- the filter kernel's instantiations, a line per family of windows: (threads, register-window steps, shard rule, postings per
// chunk, virtual rows, signed weights, prefetched long sweeps, 8-bit accumulators).  One table, one lookup (cx_kernel, apss_hip.hip, expands the
// same lists into addresses, in filter_variant_index's order): a combination that is not listed is an error, never another kernel.
// (512, 5, no shard rule, LONGPF was listed for APSS_DEBUG=longpf alone: long sweeps are taken behind a dense-head block or by
// a term shard's virtual rows, and both set the shard rule)
#define APSS_CX_VARIANTS(X) \
  X(512, 5, false, 16, false, false, false, false) X(512, 4, false, 16, false, false, false, false) X(512, 3, false, 16, false, false, false, false) X(512, 2, false, 16, false, false, false, false) \
  X(512, 5, true, 16, false, false, false, false) X(512, 4, true, 16, false, false, false, false) X(512, 3, true, 16, false, false, false, false) X(512, 2, true, 16, false, false, false, false) \
  X(512, 5, true, 16, false, false, false, true) X(512, 4, true, 16, false, false, false, true) X(512, 3, true, 16, false, false, false, true) X(512, 2, true, 16, false, false, false, true) \
  X(512, 5, false, 16, false, false, false, true) X(512, 4, false, 16, false, false, false, true) X(512, 3, false, 16, false, false, false, true) X(512, 2, false, 16, false, false, false, true) \
  X(512, 5, true, 16, false, false, true, false) \
  X(512, 5, true, 16, true, false, true, false) \
  X(512, 4, false, 8, false, false, false, false) \
  X(512, 5, false, 16, true, false, false, false) \
  X(512, 5, false, 16, false, true, false, false) \
  X(512, 5, true, 16, false, true, false, false) \
  X(512, 5, false, 16, true, true, false, false) \
  X(1024, 5, false, 16, false, false, false, false) X(1024, 3, false, 16, false, false, false, false) \
  X(1024, 5, false, 16, true, false, false, false) X(1024, 3, false, 16, true, false, false, false) \
  X(1024, 5, false, 16, false, true, false, false) X(1024, 3, false, 16, false, true, false, false) \
  X(1024, 5, false, 16, false, false, false, true) X(1024, 3, false, 16, false, false, false, true)

struct CxVariant {
  int block, u;
  bool shard;
  int chunk;
  bool vrows, sgn;
  bool longpf;  // prefetched long-segment sweeps: the sparse half of a handle with a dense-head block
  bool acc8;    // 8-bit accumulators over 65536-row tiles: thin rounds of a term shard
  bool even;    // k_probe_even: a round is staged by ceil(longest query / 64) waves and its chunks dealt out evenly
  bool merge;   // k_probe_even<.., MERGE>: neighbouring query rows share a round (term shards)
  bool planes;  // k_probe_planes: two planes of 8-bit sums over the 16-bit rendering of <= 32768-row tiles, one barrier per round (acc8 is set too)
};

// k_probe_even's instantiations: (threads, window steps, shard rule, signed weights, 8-bit accumulators)
// (512, 7 without the shard rule was listed for APSS_DEBUG=even_wide alone: a plain 512-thread handle has at least 6 adding waves,
// and 6 x 7 = 42 window steps exceed k_probe_coarse's 8 x 5 = 40, so plan_filter's `fits` refuses the seven-step window)
#define APSS_EVEN_VARIANTS(X) \
  X(512, 6, false, false, false) X(512, 5, false, false, false) X(512, 4, false, false, false) X(512, 3, false, false, false) X(512, 2, false, false, false) \
  X(512, 7, true, false, false) X(512, 6, true, false, false) X(512, 5, true, false, false) X(512, 4, true, false, false) X(512, 3, true, false, false) X(512, 2, true, false, false) \
  X(512, 7, true, false, true) X(512, 6, true, false, true) X(512, 5, true, false, true) X(512, 4, true, false, true) X(512, 3, true, false, true) X(512, 2, true, false, true) \
  X(512, 4, false, false, true) X(512, 3, false, false, true) X(512, 2, false, false, true) \
  X(1024, 7, false, false, false) X(1024, 6, false, false, false) X(1024, 5, false, false, false) X(1024, 3, false, false, false) \
  X(1024, 7, false, false, true) X(1024, 6, false, false, true) X(1024, 5, false, false, true) X(1024, 3, false, false, true)
// ... and with MERGE (shard rule, non-negative weights): (window steps, 8-bit accumulators)
#define APSS_EVEN_MERGE_VARIANTS(X) \
  X(7, false) X(6, false) X(5, false) X(4, false) X(3, false) X(2, false) \
  X(7, true) X(6, true) X(5, true) X(4, true) X(3, true) X(2, true)
// ... and with two planes of 8-bit sums (k_probe_planes): every window a plain 512-thread handle takes (2 .. 6 steps)
#define APSS_EVEN_PLANES_VARIANTS(X) X(6) X(5) X(4) X(3) X(2)

// THE walk of the tables: the variant's place in them, planes first, then merged, even, coarse (-1: not listed).  cx_kernel keeps
// the instantiations' addresses in the same order.
inline int filter_variant_index(const CxVariant &v) {
  const bool even_shape = v.chunk == 16 && !v.vrows && !v.longpf;  // (what every k_probe_even is built for)
  const bool planes = v.even && v.planes, merged = v.even && !v.planes && v.merge, even = v.even && !v.planes && !v.merge;
  int i = 0;
#define X(U)                                                                                                      \
  if (planes && v.block == 512 && v.u == U && !v.shard && !v.sgn && v.acc8 && !v.merge && even_shape) return i; \
  ++i;
  APSS_EVEN_PLANES_VARIANTS(X)
#undef X
#define X(U, A8)                                                                                            \
  if (merged && v.block == 512 && v.u == U && v.shard && !v.sgn && v.acc8 == A8 && even_shape) return i; \
  ++i;
  APSS_EVEN_MERGE_VARIANTS(X)
#undef X
#define X(B, U, SH, SG, A8)                                                                                        \
  if (even && v.block == B && v.u == U && v.shard == SH && v.sgn == SG && v.acc8 == A8 && even_shape) return i; \
  ++i;
  APSS_EVEN_VARIANTS(X)
#undef X
#define X(B, U, SH, CH, VR, SG, LP, A8)                                                                                         \
  if (!v.even && v.block == B && v.u == U && v.shard == SH && v.chunk == CH && v.vrows == VR && v.sgn == SG && v.longpf == LP && \
      v.acc8 == A8)                                                                                                             \
    return i;                                                                                                                   \
  ++i;
  APSS_CX_VARIANTS(X)
#undef X
  return -1;
}
inline bool filter_variant_listed(const CxVariant &v) { return filter_variant_index(v) >= 0; }

// ---- which instantiation of the filter kernel ----
// What a probe knows when it picks it
struct FilterFacts {
  bool acc8;         // this call's norms and row lengths leave room for 8-bit sums over the handle's >= 65536-row tiles
  bool shard_rule;   // term shard, or the sparse half of a handle with a dense-head block
  bool sgn;          // weights of either sign: the filter sums the positive products
  bool hybrid;       // the handle has a dense-head block
  int64_t s_max_nnz, s_nnz_end;  // longest staged query row, elements staged
  int64_t nq, idx_nnz;           // query rows, postings in the inverted index
  int max_merge_log2;            // k_probe_even: up to 2^this query rows may share a round (0: none; merge_rows_log2)
  double planes_scale;           // k_probe_planes: units per 1.0 at which this call's sums fit a byte (acc8_scale; 0: they do not)
  int32_t q_chunk;               // query rows per chunk of this call
  // the coarse rendering: rows per tile, longest (tile, term) segment, long segments, tiles, chunks an average stored row deals out per round
  int32_t cb;
  uint32_t max_seg, long_segs;
  int64_t n_tiles;
  double round_chunks;
  // the handle: stored rows, dimension, term range, and its latch (the 8-bit filter proved unusable on its data)
  int64_t n_rows;
  int32_t dim, term_lo, term_hi;
  bool no_acc8;
};
struct FilterPlan {
  CxVariant v;
  int32_t flat_waves, flat_group_log2, merge_log2;  // k_probe_even: staging waves, log2 of the staging lanes per term, log2 of the rows per round
  bool listed;                                      // v has an instantiation (false: APSS_E_UNSUPPORTED)
};

// The register window (U steps of 8 chunks per wave) is sized for the chunks a wave expects per round; a round's cost grows
// with U whether or not its slots hold postings, so thin rounds (term shards: 1/T of a query's terms; sparse regimes: short
// segments) take a short window.  Pure arithmetic on what ingest and the index build measured; the choice is reported in
// apss_stats.probe_kernel.  diag: gets a line per candidate of k_probe_even (APSS_DEBUG=diag prints them; the thin-round tests parse them)
inline FilterPlan plan_filter(const FilterFacts &f, const FilterHooks &dbg, std::string *diag = nullptr) {
  FilterPlan p{};
  CxVariant &cxv = p.v;
  cxv.acc8 = f.acc8;
  cxv.block = f.cb > 65536 || (f.cb > 32768 && !cxv.acc8) ? 1024 : 512;
  cxv.shard = f.shard_rule;
  cxv.chunk = dbg.chunk8 ? 8 : 16;
  cxv.vrows = f.s_max_nnz > 512;
  cxv.sgn = f.sgn;
  const double nw = cxv.block / kWave;
  const double seg = (double)f.cb * ((double)f.idx_nnz / (double)f.n_rows) / (double)f.dim;  // postings per (tile, term)
  const double q_terms = (double)f.s_nnz_end / (double)f.nq;
  // a shard holds a binomial share of each query's terms; a window that overflows costs a whole-tile clear, so the
  // shard-rule launches size it for the upper end (3 sigma) and for segments one chunk longer than their mean
  const double t_hi = f.shard_rule ? q_terms + 3.0 * std::sqrt(q_terms) : q_terms;
  const double wave_chunks = std::ceil(t_hi / nw - 1e-9) * std::max(1.0, seg / 16.0 + (f.shard_rule ? 1.0 : 0.5));
  int u = (int)std::ceil(wave_chunks * (f.shard_rule ? 1.0 : 1.05) / 8.0);
  if (cxv.block == 1024) u = (q_terms / nw) * std::max(1.0, seg / 16.0 + 0.5) <= 17.0 ? 3 : 5;
  else u = std::max(2, std::min(5, u));
  if (cxv.vrows || cxv.sgn) u = cxv.block == 1024 ? u : 5;
  if (dbg.chunk8) u = 4;
  if (dbg.window && cxv.block == 512 && !cxv.vrows && !cxv.sgn) u = dbg.window;
  // the skewed tail of a handle with a dense-head block: full window, prefetched long sweeps.  (A term shard's tail range
  // may hold no long segment at all once the block has taken the frequent terms: it then runs like any other shard)
  const bool long_tail = f.hybrid && f.max_seg > (uint32_t)kLongLenW && !cxv.acc8;
  if (long_tail && !dbg.window) {
    u = 5;
    cxv.longpf = true;
  }
  if (cxv.vrows && cxv.shard && !cxv.sgn) {  // long rows (real TF-IDF) on a term shard: the shard-rule instantiation that takes virtual rows
    u = 5;
    cxv.longpf = true;
  }
  cxv.u = u;
  // k_probe_even (apss_even.hpp): F waves stage the round, the others add an even share of its chunks -- a wave's window
  // then holds a 1/A share of the ROUND's chunks, not the chunks of the wave's own terms.
  // Staging lanes per term: as many as keep the staging waves at <= a quarter of the workgroup.
  // Where it is taken (measured on C3 and its shards, ms of the filter kernel, k_probe_even vs k_probe_coarse): term shards
  // T = 8: 23.4 vs 40.5, T = 4: 35.6 vs 62.4, T = 2 (one staging lane per term, 7-step windows): 58.7 vs 77.9; the sparse
  // regime's 1024-thread kernel (C5's shape at a fifth of N): 218.2 vs 291.5; the plain handle of C3 itself (100-term rows,
  // LDS-throughput-bound): 100.6 vs 111.3 with six adding waves x 6 steps, 115.4 with 7 steps -- a plain 512-thread handle
  // takes it when its adding waves issue no more window steps per round than k_probe_coarse's eight would.
  const bool wide_ok = f.shard_rule || cxv.block == 1024;
  // (not where long segments abound -- more than 16 long terms per tile: the thin-round kernel sweeps them on its rare
  // path, meant for one round in a few.  C3 with Zipf(0.5) terms, ~400 long terms per tile and half a dozen in every round,
  // measured 1395 ms there against 518 ms on k_probe_coarse)
  const bool few_longs = (double)f.long_segs <= 16.0 * (double)std::max<int64_t>(1, f.n_tiles) || f.shard_rule || cxv.block == 1024;
  // MERGED rounds (apss_even.hpp): M = 2^m neighbouring query rows staged as one row, when a single query's round is thin (a
  // window of <= 4 steps) and the merged round still fits a window; the caller says how many the accumulators have room for
  int ue_single = 0;
  for (int m = 0; m <= f.max_merge_log2; ++m) {
    const int64_t M = 1LL << m;
    const int64_t row_max = std::min<int64_t>(f.s_max_nnz * M, f.s_nnz_end);  // longest staged row: at most M of the longest
    int flat_group_log2 = 2;
    while (flat_group_log2 > 0 && ceil_div(row_max, kWave >> flat_group_log2) > (int64_t)nw / 4) --flat_group_log2;
    if (dbg.flat_group >= 0 && dbg.flat_group < flat_group_log2) flat_group_log2 = dbg.flat_group;
    const int64_t flat_waves = std::max<int64_t>(1, ceil_div(row_max, kWave >> flat_group_log2));
    if (!(!cxv.vrows && !cxv.longpf && cxv.chunk == 16 && !dbg.no_even && !dbg.window && flat_waves <= (int64_t)nw / 4 && few_longs)) break;
    CxVariant ev = cxv;
    ev.even = true;
    ev.merge = m > 0;
    const double add_waves = nw - (double)flat_waves;               // a wave that stages a round adds nothing in it
    // postings per (tile, term) over the terms this handle indexes (a term shard: its range, not the whole dimension)
    const double seg_here = seg * (double)f.dim / (double)std::max<int64_t>(1, (int64_t)f.term_hi - f.term_lo);
    const double cpt = std::max(1.0, seg_here / 16.0 + 0.5);      // chunks per term
    const double mq_terms = q_terms * (double)M;                    // terms of a round
    // (mean + 2 sigma of a binomial share of the terms: the rounds beyond read their last chunks from the strip and end
    // with a whole-tile clear, ~2 % of them; at 3 sigma the T = 8 shard took a 3-step window: 24.8 vs 23.2 ms)
    double round_chunks = mq_terms * cpt + 2.0 * std::sqrt(mq_terms * cpt * cpt + mq_terms * 0.3);
    // ... that is the uniform-terms estimate; the index build MEASURED what an average stored row deals out per tile
    // (sum over terms of P(term in the row) x chunks of its segment): under a skewed distribution the terms a query holds
    // are the ones with the long segments, and the estimate above falls short by a factor (power-law C5's tail: 85
    // estimated, 200 dealt out: most rounds overflowed their window, a whole-tile clear each)
    if (f.round_chunks > 0.0) {
      const double rc = f.round_chunks * (double)M;
      const double per_term = std::max(1.0, rc / std::max(1.0, mq_terms));
      round_chunks = std::max(round_chunks, rc + 2.0 * std::sqrt(rc * per_term));
    }
    // (a plain handle's rows are whole rows: no binomial share of the terms; the longest row bounds the round)
    if (!f.shard_rule) round_chunks = std::min(round_chunks, 1.05 * (double)f.s_max_nnz * cpt);
    int ue = (int)std::ceil(round_chunks / (8.0 * add_waves));
    // (a window that overflows most rounds pays a whole-tile clear each time)
    const bool fits = ue <= 7 && !cxv.sgn && (wide_ok || add_waves * std::max(2, ue) <= nw * (double)cxv.u);
    ue = cxv.block == 1024 ? (ue <= 3 ? 3 : std::max(5, ue)) : std::max(2, ue);
    ev.u = ue;
    const bool listed = filter_variant_listed(ev);
    if (diag) {
      char line[320];
      snprintf(line, sizeof line, "[apss diag] even? merge %lld block %d u %d | F %lld G %d A %.0f chunks %.1f ue %d fits %d exists %d q_max %lld q_terms %.1f seg %.1f\n",
               (long long)M, cxv.block, cxv.u, (long long)flat_waves, 1 << flat_group_log2, add_waves, round_chunks, ue, (int)fits, (int)listed, (long long)f.s_max_nnz, q_terms, seg);
      *diag += line;
    }
    if (m == 0) ue_single = ue;
    if (!(fits && listed)) break;
    // (measured on C3's shards, filter kernel: T = 8, window 2 -> 4 steps: 13.1 -> 11.1 ms; T = 4, 4 -> 7 steps: 19.9 -> 17.3 ms; T = 2
    // needs its 7 steps for one row.  FOUR rows per round at T = 8, 7 steps and 2^5 units per 1.0: 10.6 ms but 6.5 x the
    // candidates for the exchange -- not by default, APSS_DEBUG=merge=2)
    if (m > 0 && !(ue_single <= (dbg.merge_single > 0 ? dbg.merge_single : 4) && ue <= (dbg.merge_u > 0 ? dbg.merge_u : 7))) break;
    cxv = ev;
    p.flat_waves = (int32_t)flat_waves;
    p.flat_group_log2 = flat_group_log2;
    p.merge_log2 = m;
  }
  // TWO PLANES (apss_even.hpp): exactly where the plain 512-thread k_probe_even is taken -- same U, F and work list, the
  // same 16-bit rendering of the index -- when the tiles fit a plane and this call's norms and row lengths leave room for byte
  // sums; the caller launches it on the 8-bit scale.  A launch that turns out unselective latches the handle back (drop_planes).
  // Only for query chunks of kPlanesMinChunk rounds or more: what the kernel saves, it saves per round, and what two planes cost
  // they cost per item.  Measured (profiles/even_planes.md): the whole-store join of C3, chunks of 977 rounds (the last items
  // in pieces of 128): filter kernel -2.2 %; C3 streamed in batches of 16,384 rows, chunks of 16 to 124 rounds: +0.6 %.
  if (cxv.even && !cxv.merge && cxv.block == 512 && !cxv.shard && !cxv.sgn && !cxv.acc8 && f.cb <= 32768 && f.planes_scale > 0 &&
      (f.q_chunk >= kPlanesMinChunk || dbg.planes) && !dbg.no_planes && !dbg.no_acc8 && !f.no_acc8) {
    CxVariant pv = cxv;
    pv.acc8 = pv.planes = true;
    if (filter_variant_listed(pv)) cxv = pv;
  }
  p.listed = filter_variant_listed(cxv);
  return p;
}

}  // namespace apss
