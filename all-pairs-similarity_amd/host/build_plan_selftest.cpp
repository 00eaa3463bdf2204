// The build plan (csrc/apss_build_plan.hpp) against a table of literal decisions, on the CPU.  A wrong form still builds a correct
// index, only slower, so no result test sees the rule: this one pins it down on both sides of every threshold -- the 48 workgroups of
// the LDS kinds (with and without tiles that stay) and of the bucketed build, kRunMinMeanRow, one / two and 16 / 17 ranges, the
// doubling bucket range, the 2^31 cut points, the 6e8 and 2^32 entry bounds, exact renderings, term ranges, every hook alone, the
// run_sub values that are refused, and the shapes DESIGN.md measures.  The expected values were printed by the decision code as it
// stood before the plan existed (build_form and the inline decisions of build_tiles), not by the code under test; so were the
// trace lines the formatter is held to.  Built with -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>

#include "../csrc/apss_build_plan.hpp"

using apss::BuildHooks;
using apss::BuildPlan;
using apss::BuildShape;
using K = apss::BuildKind;

namespace {

struct Row {
  const char *name;
  BuildShape s;  // dim, term_lo, term_hi, cb, coarse, tile0, n_tiles, rows, nnz, max_nnz
  BuildHooks k;
  K kind;
  int32_t n_ranges, range_terms, run_sub, n_sub;
  int run_lanes;
  int64_t group_tiles;
};
#define H(...) ([] { BuildHooks k; __VA_ARGS__; return k; }())

const Row kRows[] = {
    // workgroup threshold of the LDS kinds: (n_tiles - tile0) * n_ranges >= 48
    {"lds 47 workgroups, tile0 0", {10000, 0, 10000, 1024, true, 0, 47, 48000, 2400000, 60}, H(), K::Atomic, 1, 16384, 256, 40, 32, 47},
    {"lds 48 workgroups, tile0 0", {10000, 0, 10000, 1024, true, 0, 48, 49000, 2450000, 60}, H(), K::Stream, 1, 16384, 256, 40, 32, 48},
    {"lds 47 workgroups, tile0 2", {10000, 0, 10000, 1024, true, 2, 49, 50000, 2500000, 60}, H(), K::Atomic, 1, 16384, 256, 40, 32, 49},
    {"lds 48 workgroups, tile0 2", {10000, 0, 10000, 1024, true, 2, 50, 51000, 2550000, 60}, H(), K::Stream, 1, 16384, 256, 40, 32, 50},
    {"lds 7 ranges, 6 tiles = 42", {100000, 0, 100000, 32768, true, 0, 6, 196000, 19600000, 100}, H(), K::Atomic, 7, 16384, 256, 391, 8, 6},
    {"lds 7 ranges, 7 tiles = 49", {100000, 0, 100000, 32768, true, 0, 7, 229000, 22900000, 100}, H(), K::Runs, 7, 16384, 256, 391, 8, 7},
    {"lds 7 ranges, tiles [1, 7) = 42", {100000, 0, 100000, 32768, true, 1, 7, 229000, 22900000, 100}, H(), K::Atomic, 7, 16384, 256, 391, 8, 7},
    {"lds 7 ranges, tiles [1, 8) = 49", {100000, 0, 100000, 32768, true, 1, 8, 262000, 26200000, 100}, H(), K::Runs, 7, 16384, 256, 391, 8, 8},
    // ... of the bucketed build: n_tiles * n_ranges >= 48 and tile0 == 0
    {"bucketed 47 ranges, 1 tile", {770048, 0, 770048, 65536, true, 0, 1, 60000, 6000000, 100}, H(), K::Atomic, 47, 16384, 256, 3008, 4, 1},
    {"bucketed 48 ranges, 1 tile", {786432, 0, 786432, 65536, true, 0, 1, 60000, 6000000, 100}, H(), K::Bucketed, 96, 8192, 256, 3072, 4, 1},
    {"bucketed dim 2^20, tile0 0", {1048576, 0, 1048576, 65536, true, 0, 2, 100000, 10000000, 100}, H(), K::Bucketed, 128, 8192, 256, 4096, 4, 2},
    {"bucketed dim 2^20, tile0 1", {1048576, 0, 1048576, 65536, true, 1, 2, 100000, 10000000, 100}, H(), K::Atomic, 64, 16384, 256, 4096, 4, 2},
    {"bucketed dim 2^20, tile0 1 of 50", {1048576, 0, 1048576, 65536, true, 1, 50, 3200000, 320000000, 100}, H(), K::Atomic, 64, 16384, 256, 4096, 4, 50},
    // mean row against kRunMinMeanRow
    {"mean row 19.9", {100000, 0, 100000, 128, true, 0, 8, 1000, 19900, 40}, H(), K::Stream, 7, 16384, 256, 391, 4, 8},
    {"mean row 20.0", {100000, 0, 100000, 128, true, 0, 8, 1000, 20000, 40}, H(), K::Runs, 7, 16384, 256, 391, 4, 8},
    // one range / two ranges
    {"one range", {16384, 0, 16384, 1024, true, 0, 48, 49000, 2450000, 60}, H(), K::Stream, 1, 16384, 256, 64, 32, 48},
    {"two ranges", {16385, 0, 16385, 1024, true, 0, 48, 49000, 2450000, 60}, H(), K::Runs, 2, 16384, 256, 65, 16, 48},
    // 16 / 17 ranges of 16384 terms
    {"16 ranges", {262144, 0, 262144, 32768, true, 0, 3, 90000, 9000000, 100}, H(), K::Runs, 16, 16384, 256, 1024, 4, 3},
    {"17 ranges", {262145, 0, 262145, 32768, true, 0, 3, 90000, 9000000, 100}, H(), K::Bucketed, 33, 8192, 256, 1025, 4, 3},
    {"17 ranges, 2 tiles = 34", {262145, 0, 262145, 32768, true, 0, 2, 60000, 6000000, 100}, H(), K::Atomic, 17, 16384, 256, 1025, 4, 2},
    // ceil(dim / 8192) at 1024 / 1025: the bucket range doubles
    {"1024 bucket ranges", {8388608, 0, 8388608, 65536, true, 0, 4, 250000, 25000000, 100}, H(), K::Bucketed, 1024, 8192, 256, 32768, 4, 4},
    {"1025 bucket ranges", {8388609, 0, 8388609, 65536, true, 0, 4, 250000, 25000000, 100}, H(), K::Bucketed, 513, 16384, 256, 32769, 4, 4},
    {"dim 2^24", {16777216, 0, 16777216, 65536, true, 0, 4, 250000, 25000000, 100}, H(), K::Bucketed, 1024, 16384, 256, 65536, 4, 4},
    {"dim 2^24 + 1", {16777217, 0, 16777217, 65536, true, 0, 4, 250000, 25000000, 100}, H(), K::Atomic, 1025, 16384, 256, 65537, 4, 4},
    // 32-bit cut points: max_nnz * cb against 2^31
    {"cuts below 2^31", {100000, 0, 100000, 32768, true, 0, 8, 262144, 26214400, 65535}, H(), K::Runs, 7, 16384, 256, 391, 8, 8},
    {"cuts at 2^31", {100000, 0, 100000, 32768, true, 0, 8, 262144, 26214400, 65536}, H(), K::Stream, 7, 16384, 256, 391, 8, 8},
    {"max_nnz 0", {100000, 0, 100000, 32768, true, 0, 8, 262144, 26214400, 0}, H(), K::Runs, 7, 16384, 256, 391, 8, 8},
    // the scratch copy of the two-pass scatter: nnz against 6e8, nnz = 0
    {"nnz 6e8", {100000, 0, 100000, 32768, true, 0, 184, 6000000, 600000000, 100}, H(), K::Runs, 7, 16384, 256, 391, 8, 184},
    {"nnz 6e8 + 1", {100000, 0, 100000, 32768, true, 0, 184, 6000000, 600000001, 100}, H(), K::Runs, 7, 16384, 0, 0, 16, 184},
    {"nnz 0", {100000, 0, 100000, 32768, true, 0, 8, 262144, 0, 100}, H(), K::Stream, 7, 16384, 0, 0, 4, 8},
    {"nnz 0, build_runs", {100000, 0, 100000, 32768, true, 0, 8, 262144, 0, 100}, H(k.build_runs = true), K::Runs, 7, 16384, 0, 0, 4, 8},
    {"rows 0", {100000, 0, 100000, 32768, true, 0, 8, 0, 0, 0}, H(), K::Stream, 7, 16384, 0, 0, 4, 8},
    // the bucketed build's bounds on nnz: > 0, <= 2^32
    {"bucketed nnz 0", {1048576, 0, 1048576, 65536, true, 0, 4, 250000, 0, 100}, H(), K::Atomic, 64, 16384, 0, 0, 4, 4},
    {"bucketed nnz 2^32", {1048576, 0, 1048576, 131072, true, 0, 164, 21474836, 4294967296, 200}, H(), K::Bucketed, 128, 8192, 0, 0, 4, 22},
    {"bucketed nnz 2^32 + 1", {1048576, 0, 1048576, 131072, true, 0, 164, 21474836, 4294967297, 200}, H(), K::Atomic, 64, 16384, 0, 0, 4, 164},
    // exact rendering: no sub-ranges
    {"exact rendering", {100000, 0, 100000, 16384, false, 0, 62, 1000000, 100000000, 100}, H(), K::Runs, 7, 16384, 0, 0, 16, 62},
    {"exact rendering, run_sub 256", {100000, 0, 100000, 16384, false, 0, 62, 1000000, 100000000, 100}, H(k.run_sub = 256), K::Runs, 7, 16384, 0, 0, 16, 62},
    // a term range that leaves one active range
    {"terms [20000, 30000)", {100000, 20000, 30000, 65536, true, 0, 16, 1000000, 25000000, 100}, H(), K::Runs, 7, 16384, 256, 391, 16, 16},
    {"terms [16000, 17000)", {100000, 16000, 17000, 65536, true, 0, 16, 1000000, 25000000, 100}, H(), K::Runs, 7, 16384, 256, 391, 8, 16},
    // each hook alone
    {"build_lds, 7 workgroups", {100000, 0, 100000, 32768, true, 0, 1, 30000, 3000000, 100}, H(k.build_lds = true), K::Runs, 7, 16384, 256, 391, 8, 1},
    {"build_lds, 17 ranges", {262145, 0, 262145, 32768, true, 0, 2, 60000, 6000000, 100}, H(k.build_lds = true), K::Atomic, 17, 16384, 256, 1025, 4, 2},
    {"build_atomic", {100000, 0, 100000, 32768, true, 0, 31, 1000000, 100000000, 100}, H(k.build_atomic = true), K::Atomic, 7, 16384, 256, 391, 8, 31},
    {"build_atomic, dim 2^20", {1048576, 0, 1048576, 65536, true, 0, 4, 250000, 25000000, 100}, H(k.build_atomic = true), K::Atomic, 64, 16384, 256, 4096, 4, 4},
    {"build_stream", {100000, 0, 100000, 32768, true, 0, 31, 1000000, 100000000, 100}, H(k.build_stream = true), K::Stream, 7, 16384, 256, 391, 8, 31},
    {"build_runs, one range", {16384, 0, 16384, 1024, true, 0, 48, 49000, 2450000, 60}, H(k.build_runs = true), K::Runs, 1, 16384, 256, 64, 32, 48},
    {"build_runs, short rows", {100000, 0, 100000, 128, true, 0, 8, 1000, 5000, 10}, H(k.build_runs = true), K::Runs, 7, 16384, 256, 391, 4, 8},
    {"build_runs, 7 workgroups", {100000, 0, 100000, 32768, true, 0, 1, 30000, 3000000, 100}, H(k.build_runs = true), K::Atomic, 7, 16384, 256, 391, 8, 1},
    {"build_runs, cuts at 2^31", {100000, 0, 100000, 32768, true, 0, 8, 262144, 26214400, 65536}, H(k.build_runs = true), K::Stream, 7, 16384, 256, 391, 8, 8},
    {"run_range 8192", {100000, 0, 100000, 32768, true, 0, 31, 1000000, 100000000, 100}, H(k.run_range = 8192), K::Runs, 13, 8192, 256, 391, 4, 31},
    {"run_range 1024 (98 ranges)", {100000, 0, 100000, 32768, true, 0, 31, 1000000, 100000000, 100}, H(k.run_range = 1024), K::Stream, 7, 16384, 256, 391, 4, 31},
    {"run_range 32768 (capped)", {100000, 0, 100000, 32768, true, 0, 31, 1000000, 100000000, 100}, H(k.run_range = 32768), K::Runs, 7, 16384, 256, 391, 8, 31},
    {"run_lanes 4", {100000, 0, 100000, 32768, true, 0, 31, 1000000, 100000000, 100}, H(k.run_lanes = 4), K::Runs, 7, 16384, 256, 391, 4, 31},
    {"run_lanes 32", {100000, 0, 100000, 32768, true, 0, 31, 1000000, 100000000, 100}, H(k.run_lanes = 32), K::Runs, 7, 16384, 256, 391, 32, 31},
    {"run_lanes 5 (ignored)", {100000, 0, 100000, 32768, true, 0, 31, 1000000, 100000000, 100}, H(k.run_lanes = 5), K::Runs, 7, 16384, 256, 391, 8, 31},
    {"run_sub 0", {100000, 0, 100000, 32768, true, 0, 31, 1000000, 100000000, 100}, H(k.run_sub = 0), K::Runs, 7, 16384, 0, 0, 16, 31},
    {"run_sub 128", {100000, 0, 100000, 32768, true, 0, 31, 1000000, 100000000, 100}, H(k.run_sub = 128), K::Runs, 7, 16384, 128, 782, 8, 31},
    {"run_sub 64", {100000, 0, 100000, 32768, true, 0, 31, 1000000, 100000000, 100}, H(k.run_sub = 64), K::Runs, 7, 16384, 64, 1563, 8, 31},
    {"run_sub 1024", {100000, 0, 100000, 32768, true, 0, 31, 1000000, 100000000, 100}, H(k.run_sub = 1024), K::Runs, 7, 16384, 1024, 98, 8, 31},
    {"no_bucket", {1048576, 0, 1048576, 65536, true, 0, 4, 250000, 25000000, 100}, H(k.no_bucket = true), K::Atomic, 64, 16384, 256, 4096, 4, 4},
    // run_sub values that are rejected
    {"run_sub 63", {100000, 0, 100000, 32768, true, 0, 31, 1000000, 100000000, 100}, H(k.run_sub = 63), K::Runs, 7, 16384, 0, 0, 16, 31},
    {"run_sub 96", {100000, 0, 100000, 32768, true, 0, 31, 1000000, 100000000, 100}, H(k.run_sub = 96), K::Runs, 7, 16384, 0, 0, 16, 31},
    {"run_sub 2048", {100000, 0, 100000, 32768, true, 0, 31, 1000000, 100000000, 100}, H(k.run_sub = 2048), K::Runs, 7, 16384, 0, 0, 16, 31},
    {"run_sub 256 does not divide run_range 10000", {100000, 0, 100000, 32768, true, 0, 31, 1000000, 100000000, 100}, H(k.run_range = 10000; k.run_sub = 256), K::Runs, 10, 10000, 0, 0, 16, 31},
    // lanes per row from the mean run: 4 | 8 | 16 | 32
    {"mean run 8.0 in one pass", {100000, 0, 100000, 32768, true, 0, 31, 1000000, 56000000, 100}, H(k.run_sub = 0), K::Runs, 7, 16384, 0, 0, 8, 31},
    {"mean run 8.0 in two passes", {100000, 0, 100000, 32768, true, 0, 31, 1000000, 56000000, 100}, H(), K::Runs, 7, 16384, 256, 391, 4, 31},
    {"mean run 34.3 in one pass", {100000, 0, 100000, 32768, true, 0, 31, 1000000, 240000000, 300}, H(k.run_sub = 0), K::Runs, 7, 16384, 0, 0, 32, 31},
    {"mean run 34.3 in two passes", {100000, 0, 100000, 32768, true, 0, 31, 1000000, 240000000, 300}, H(), K::Runs, 7, 16384, 256, 391, 32, 31},
    // the shapes of DESIGN.md: C3, its term shards T = 2 / 4 / 8, C5 at N = 2M and at full size
    {"C3", {100000, 0, 100000, 32768, true, 0, 31, 1000000, 100000000, 100}, H(), K::Runs, 7, 16384, 256, 391, 8, 31},
    {"C3, exact rendering", {100000, 0, 100000, 16384, false, 0, 62, 1000000, 100000000, 100}, H(), K::Runs, 7, 16384, 0, 0, 16, 62},
    {"C3 shard T = 2", {100000, 0, 50000, 65536, true, 0, 16, 1000000, 50000000, 70}, H(), K::Runs, 7, 16384, 256, 391, 8, 16},
    {"C3 shard T = 4", {100000, 25000, 50000, 65536, true, 0, 16, 1000000, 25000000, 45}, H(), K::Runs, 7, 16384, 256, 391, 8, 16},
    {"C3 shard T = 8", {100000, 12500, 25000, 65536, true, 0, 16, 1000000, 12500000, 30}, H(), K::Stream, 7, 16384, 256, 391, 4, 16},
    {"C5 at N = 2M", {1000000, 0, 1000000, 131072, true, 0, 16, 2000000, 400000000, 200}, H(), K::Bucketed, 123, 8192, 256, 3907, 4, 16},
    {"C5", {1000000, 0, 1000000, 131072, true, 0, 77, 10000000, 2000000000, 200}, H(), K::Bucketed, 123, 8192, 0, 0, 4, 23},
    {"C5, second batch", {1000000, 0, 1000000, 131072, true, 15, 31, 4000000, 800000000, 200}, H(), K::Atomic, 62, 16384, 0, 0, 4, 31},
};

struct Trace {
  const char *row, *text;
};
const Trace kTraces[] = {
    {"lds 47 workgroups, tile0 0", "[apss] build coarse tiles [0, 47): atomic, 1 ranges of 16384 terms, 0 lanes per row (mean run 50.00)\n"},
    {"one range", "[apss] build coarse tiles [0, 48): stream, 1 ranges of 16384 terms, 0 lanes per row (mean run 50.00)\n"},
    {"C3", "[apss] build coarse tiles [0, 31): runs, 7 ranges of 16384 terms, 8 lanes per row (mean run 14.29)\n"
           "[apss]   scatter through sub-ranges of 256 terms\n"},
    {"C3, exact rendering", "[apss] build exact tiles [0, 62): runs, 7 ranges of 16384 terms, 16 lanes per row (mean run 14.29)\n"
                            "[apss]   scatter through sub-ranges of 0 terms\n"},
    {"C5 at N = 2M", "[apss] build coarse tiles [0, 16): bucketed, 123 ranges of 8192 terms, 0 lanes per row (mean run 3.23)\n"},
};

}  // namespace

int main() {
  int failures = 0, traced = 0;
  for (const Row &r : kRows) {
    const BuildPlan p = apss::build_plan(r.s, r.k);
    if (p.kind != r.kind || p.n_ranges != r.n_ranges || p.range_terms != r.range_terms || p.run_sub != r.run_sub || p.n_sub != r.n_sub ||
        p.run_lanes != r.run_lanes || p.group_tiles != r.group_tiles) {
      ++failures;
      std::fprintf(stderr, "FAIL %s: kind %d, %d ranges of %d terms, run_sub %d, n_sub %d, %d lanes, groups of %lld tiles; expected %d, %d, %d, %d, %d, %d, %lld\n",
                   r.name, (int)p.kind, (int)p.n_ranges, (int)p.range_terms, (int)p.run_sub, (int)p.n_sub, p.run_lanes, (long long)p.group_tiles,
                   (int)r.kind, (int)r.n_ranges, (int)r.range_terms, (int)r.run_sub, (int)r.n_sub, r.run_lanes, (long long)r.group_tiles);
    }
    for (const Trace &t : kTraces) {
      if (std::strcmp(t.row, r.name)) continue;
      ++traced;
      const std::string got = apss::build_trace_text(r.s, p);
      if (got != t.text) {
        ++failures;
        std::fprintf(stderr, "FAIL trace of %s:\n%s-- expected:\n%s", r.name, got.c_str(), t.text);
      }
    }
  }
  if (traced != (int)(sizeof kTraces / sizeof kTraces[0])) {
    ++failures;
    std::fprintf(stderr, "FAIL: %d of the trace rows found\n", traced);
  }
  if (failures) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("build plan selftest ok: %d rows, %d traces\n", (int)(sizeof kRows / sizeof kRows[0]), traced);
  return 0;
}
