// The PLAN of an index build: which kernels the build of tiles [tile0, n_tiles) takes and in which form, settled before the first
// launch from the shape of what is built.  Plain C++ (no HIP): build_tiles decides with it (apss_hip.hip), the ingest asks it
// beforehand whether the rows it stores will be read by runs (ingest_wants_cuts), so that the two cannot drift apart, and
// host/build_plan_selftest.cpp checks the rule on both sides of every threshold.  The kernels, and what each form is and saves, are in apss_build.hpp.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>

namespace apss {

constexpr int kBuildRange = 16384;    // 64 KB of LDS counters: two workgroups per CU (C3: 217 workgroups instead of 124; build 5.0 -> 3.8 ms)
constexpr int kBuildMaxRanges = 16;
constexpr int kRunRange = 16384;  // terms per range of the run-reading build (8192: twice the workgroups, half the run per row -- C3 build
                                  //   3.1 ms against 2.5, profiles/build_runs.md)
// ... the mean row length (entries the handle keeps of a row) below which the streaming kernels are kept -- the cut table and
// the second pass are paid per row and per (tile, sub-range), the re-reads they remove per entry.  Measured on term shards of C3
// (profiles/build_runs.md): T = 2 (50 entries per row) build 3.42 -> 2.67 ms, T = 4 (25) 2.09 -> 1.94, T = 8 (12.5) 1.36 -> 1.78.
constexpr double kRunMinMeanRow = 20.0;
constexpr int kRunSub = 256;  // terms per sub-range of the two-pass scatter
constexpr int kPlaceMaxTerms = 1024;
constexpr int kBucketSlices = 64;       // workgroups per tile
constexpr int kBucketMaxRanges = 1024;  // dims up to 2^24
// (terms per range of a bucketed build, measured on C5's shape, build ms per step: 1024: 28.3, 2048: 23.9, 4096: 20.4, 8192: 15.6,
// 16384: 17.4 -- against 37.5 with the global-atomic kernels; narrow ranges multiply the workgroups' fixed work)
constexpr int kBucketRange = 8192;

// what is built: tiles [tile0, n_tiles) of `cb` rows of a handle's rendering, from `rows` rows of `nnz` entries, the longest of `max_nnz`
struct BuildShape {
  int32_t dim, term_lo, term_hi;  // of the handle
  int64_t cb;
  bool coarse;  // the rendering: rows per tile, 4-B postings
  int64_t tile0, n_tiles, rows, nnz, max_nnz;
};
// the build tokens of APSS_DEBUG (each described with the other tokens, in DebugCfg)
struct BuildHooks {
  bool build_lds = false, build_atomic = false, build_stream = false, build_runs = false;
  int run_range = 0, run_lanes = 0, run_sub = -1;
  bool no_bucket = false;
};
enum class BuildKind { Atomic, Stream, Runs, Bucketed, Append };  // (Append: never planned -- build_tiles takes it for a batch that lands in the partly filled last tile)
struct BuildPlan {
  BuildKind kind;
  int32_t n_ranges, range_terms;  // (tile, term range) workgroups of the LDS kinds
  int32_t run_sub, n_sub;         // Runs: terms per sub-range of a scatter in two passes (0: one pass), sub-ranges per tile
  int run_lanes;                  // Runs: lanes per row
  double mean_run;
  int64_t group_tiles;            // Bucketed: tiles whose entries are bucketed together
};

inline BuildPlan build_plan(const BuildShape &s, const BuildHooks &k) {
  const auto plan_ceil_div = [](int64_t a, int64_t b) { return (a + b - 1) / b; };
  // LDS kinds, one workgroup per (tile, term range): with fewer than ~48 of them -- a small batch, a rebuilt tail tile, a 1/8 candidate
  // range -- the row-parallel global-atomic kernels are faster; build_lds / build_atomic force either
  int32_t n_ranges = (int32_t)plan_ceil_div(s.dim, kBuildRange);
  // large dims (more than kBuildMaxRanges ranges: vectorDim = 2^20): a build from the first tile is bucketed by term range first
  int32_t bucket_rt = kBucketRange;
  while (plan_ceil_div(s.dim, bucket_rt) > kBucketMaxRanges && bucket_rt < kBuildRange) bucket_rt *= 2;
  const bool bucket_build = n_ranges > kBuildMaxRanges && plan_ceil_div(s.dim, bucket_rt) <= kBucketMaxRanges && !k.build_atomic &&
                            !k.no_bucket && s.tile0 == 0 && s.n_tiles * n_ranges >= 48 && s.nnz > 0 && s.nnz <= (1LL << 32) &&
                            s.n_tiles * (int64_t)kBucketSlices < (1LL << 31);
  if (bucket_build) n_ranges = (int32_t)plan_ceil_div(s.dim, bucket_rt);
  const bool lds_build = bucket_build || (n_ranges <= kBuildMaxRanges && !k.build_atomic &&
                                          ((s.n_tiles - s.tile0) * n_ranges >= 48 || k.build_lds));
  // Runs: wherever the streaming kernels would re-read the tile's entries -- two term ranges or more -- and the rows are long enough to be
  // worth a cut table (kRunMinMeanRow).  32-bit cut points: (longest row) x (rows per tile) < 2^31.
  const double mean_row = s.rows > 0 ? (double)s.nnz / (double)s.rows : 0.0;
  const int32_t run_rt = k.run_range > 0 ? std::min(k.run_range, kBuildRange) : kRunRange;
  const int64_t run_active = std::max<int64_t>(1, plan_ceil_div(s.term_hi, run_rt) - s.term_lo / run_rt);  // ranges that hold terms of this handle
  const bool run_build = lds_build && !bucket_build && !k.build_stream && std::max<int64_t>(s.max_nnz, 1) * s.cb < (1LL << 31) &&
                         plan_ceil_div(s.dim, run_rt) <= 64 && (k.build_runs || (n_ranges >= 2 && mean_row >= kRunMinMeanRow));
  if (run_build) n_ranges = (int32_t)plan_ceil_div(s.dim, run_rt);
  BuildPlan p{bucket_build ? BuildKind::Bucketed : (run_build ? BuildKind::Runs : (lds_build ? BuildKind::Stream : BuildKind::Atomic)), n_ranges,
              run_build ? run_rt : (bucket_build ? bucket_rt : kBuildRange)};
  p.mean_run = mean_row / (double)run_active;
  // ... and its scatter in two passes (BuildArgs::sub_shift) when the scratch copy of the entries is affordable
  p.run_sub = k.run_sub >= 0 ? k.run_sub : kRunSub;
  if (p.run_sub < 64 || p.run_sub > kPlaceMaxTerms || (p.run_sub & (p.run_sub - 1)) || run_rt % p.run_sub || !s.coarse || s.nnz > (int64_t)6e8 || s.nnz <= 0)
    p.run_sub = 0;
  p.n_sub = p.run_sub ? (int32_t)plan_ceil_div(s.dim, p.run_sub) : 0;
  // lanes per row, a power of two in 4 .. 32 (measured at C3, mean run 14.3: profiles/build_runs.md): about the mean run where the
  // scatter's 4-B stores go straight to memory (one pass: 16), half of it where they are 8-B stores into a handful of streams
  // (two passes: 8) -- there more rows in flight per workgroup pay more than lanes that never wait for a second chunk
  const double run_want = p.run_sub ? p.mean_run * 0.5 : p.mean_run;
  p.run_lanes = k.run_lanes;
  if (p.run_lanes != 4 && p.run_lanes != 8 && p.run_lanes != 16 && p.run_lanes != 32)
    p.run_lanes = run_want <= 4.0 ? 4 : (run_want <= 8.0 ? 8 : (run_want <= 16.0 ? 16 : 32));
  // bucketed build: tiles in GROUPS whose entries fit a bounded scratch (12 B per entry: a one-shot join of 2e9 entries would otherwise
  // spend 1.2 s allocating 24 GB to save 0.5 s of atomics; C5's shape at N = 2M is a single group of 4.8 GB)
  p.group_tiles = !bucket_build ? s.n_tiles : std::max<int64_t>(1, std::min<int64_t>(s.n_tiles, (int64_t)6e8 / std::max<int64_t>(1, s.nnz / s.n_tiles)));
  return p;
}

// the build_trace line(s) of a planned build (APSS_DEBUG=build_trace; the build tests parse them)
inline std::string build_trace_text(const BuildShape &s, const BuildPlan &p) {
  static const char *const names[] = {"atomic", "stream", "runs", "bucketed"};
  const bool runs = p.kind == BuildKind::Runs;
  char line[320];
  const int n = snprintf(line, sizeof line, "[apss] build %s tiles [%lld, %lld): %s, %d ranges of %d terms, %d lanes per row (mean run %.2f)\n",
                   s.coarse ? "coarse" : "exact", (long long)s.tile0, (long long)s.n_tiles, names[(int)p.kind], (int)p.n_ranges, (int)p.range_terms,
                   runs ? p.run_lanes : 0, p.mean_run);
  if (runs) snprintf(line + n, sizeof line - (size_t)n, "[apss]   scatter through sub-ranges of %d terms\n", (int)p.run_sub);
  return line;
}

}  // namespace apss
