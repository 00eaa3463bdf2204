// apss_hip.hip -- C ABI (include/apss.h) over the HIP kernels of apss_kernels.hpp.
//
// One handle == one IndexingWorkerActor's state (vectorsStore + invertedIndex + similarityThreshold,
// IndexingWorkerActor.scala:21-25) resident in the HBM of one MI355X.  No CPU compute path exists here: every
// entry point either runs the HIP kernels or fails with APSS_E_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>

#include "../../include/apss.h"
#include "apss_kernels.hpp"
#include "apss_head.hpp"
#include "apss_even.hpp"
#include "apss_stage.hpp"
#include "apss_topk.hpp"
#include "apss_window.hpp"
#include "apss_remove.hpp"
#include "apss_query_stored.hpp"
#include "apss_top_pairs.hpp"
#include "apss_components.hpp"
#include "apss_components_repair.hpp"

#include <rocprim/device/device_radix_sort.hpp>

using namespace apss;

namespace {

thread_local std::string g_create_error;

// A list of (query row, candidate, score) pairs: three arrays that grow, swap and go together, so they share one capacity
struct PairList {
  DevBuf<int32_t> q, c;
  DevBuf<float> s;
  size_t cap() const { return q.cap; }
  int32_t ensure(apss_handle *h, size_t n, size_t keep = 0, bool exact = false);  // (grow-only, as the arrays' own ensure)
  void swap(PairList &o) {
    std::swap(q, o.q);
    std::swap(c, o.c);
    std::swap(s, o.s);
  }
  // where the filters append (the capacity they may fill is the site's to say)
  void as_candidates(ProbeArgs &a) const {
    a.res_q = q.p;
    a.res_c = c.p;
    a.res_s = s.p;
  }
  void as_in(ShardPruneArgs &x) const {
    x.in_q = q.p;
    x.in_c = c.p;
    x.in_s = s.p;
  }
  // the out_* fields of a kernel's arguments (the handle's own are adopt_list's to write)
  template <class A>
  void as_out(A &x) const {
    x.out_q = q.p;
    x.out_c = c.p;
    x.out_s = s.p;
  }
};

// Test and experiment hooks: ONE environment word, APSS_DEBUG, read once when a handle is created -- a comma-separated
// list of the tokens below.  Nothing else in the library reads the environment.
struct DebugCfg {
  BuildHooks build;            // what the build plan reads (apss_build_plan.hpp):
                               // build_lds      index build with LDS cursors even for a handful of tiles
                               // build_atomic   index build with global atomics even for small dims
                               // build_stream   LDS index build with the whole-tile streaming kernels (never the run-reading ones)
                               // build_runs     LDS index build with the run-reading kernels whatever the number of ranges and the mean run
                               // run_range=N    terms per range of the run-reading build (<= 16384; default kRunRange)
                               // run_lanes=L    its lanes per row (4 | 8 | 16 | 32; default: from the mean run length)
                               // run_sub=W      run-reading build: scatter in two passes through sub-ranges of W terms (a power of two >= 64; 0: one pass)
                               // no_bucket      large dims build with global atomics (never the bucketed LDS build)
  bool build_trace = false;    // build_trace    one line on stderr per index build: which kernels it took
  FilterHooks filter;          // what the filter plan reads (apss_filter_plan.hpp has each token): chunk8, window=U, no_acc8, no_planes, planes, flat_group=L, no_even, merge=L, merge_u=U, merge_single=U
  bool shard_exact = false;    // shard_exact    term-range shards run the single-pass exact kernel
  bool diag = false;           // diag           in-kernel cycle stamps of the single-pass kernel (stderr)
  bool force_general = false;  // force_general  as APSS_FLAG_FORCE_GENERAL
  bool exact_accum = false;    // exact_accum    as APSS_FLAG_EXACT_ACCUM, decided per probe
  int cx_tile = 0;             // cx_tile=N      rows per tile of the coarse index (multiple of 64, <= 65536)
  int chunks = 0;              // chunks=N       query chunks per tile (grid shape)
  int tiles_per_launch = 0;    // tiles_per_launch=N
  bool no_tail = false;        // no_tail        every insert extends the tile index at once (no tail of waiting rows)
  int seg_align = 0;           // seg_align=N    postings per aligned unit of the coarse index (16 | 32)
  int fold_w = 0;              // fold_w=N       columns of the dense head's folded block (128 | 256)
  bool no_sym = false;         // no_sym         as APSS_FLAG_NO_SYMMETRY
  int mix = 0;                 // mix=E          ONE head block of 256 columns: E terms with a column each, the others folded into 256 - E
  bool no_chain = false;       // no_chain       small batches take the exact pass with its own host round trips (as large ones do)
  bool no_append = false;      // no_append      a batch that lands in a partly filled tile rebuilds the whole tile (never appends to it)
  int res_cap = 0;             // res_cap=N      initial capacity of the candidate list (tests of the overflow -> regrow -> re-run path)
  bool head_bf16 = false;      // head_bf16      the dense-head block keeps bf16 rows (v_mfma_f32_32x32x16_bf16), never the INT8 rendering
  bool no_merge_prune = false; // no_merge_prune merged rounds hand every expanded pair to the exchange (no exact shard-rule test behind k_expand_merged)
  bool no_fused_ingest = false; // no_fused_ingest a plain batch is ingested by k_ingest_count + k_ingest_write too (never the one-pass k_ingest_plain)
  bool no_persist = false;     // no_persist     k_probe_even launches one workgroup per (tile, chunk) cell, never resident workgroups over a work list
  int persist_wgs = 0;         // persist_wgs=N  ... the persistent launch has N workgroups (default: as many as the chip holds at a time)
  int persist_fine = 0;        // persist_fine=R ... and the last items of its list are R rounds long (a power of two; default kPersistFine)
  int rm_grid = 0;             // rm_grid=N      at most N workgroups for k_rm_mark, k_rm_drop and k_rm_rows (tests of their grid-stride loops; default 4096 / 16384 / 4096),
                               //                and for k_qs_select, k_qs_ids and k_qs_slots (apss_query_stored.hpp; default 4096 each)
  int tp_grid = 0;             // tp_grid=N      at most N workgroups for the grid-stride kernels of the global top-K (apss_top_pairs.hpp; default kTpGridCap)
  int cc_grid = 0;             // cc_grid=N      at most N workgroups for k_cc_hook (apss_components.hpp; default kCcGridCap): a small list takes its loop's later trips
};

DebugCfg parse_debug_env() {
  DebugCfg d;
  const char *e = getenv("APSS_DEBUG");
  if (!e) return d;
  std::string str(e);
  size_t pos = 0;
  while (pos <= str.size()) {
    const size_t end = std::min(str.find(',', pos), str.size());
    const std::string tok = str.substr(pos, end - pos);
    pos = end + 1;
    const size_t eq = tok.find('=');
    const std::string key = tok.substr(0, eq);
    const int val = eq == std::string::npos ? 1 : atoi(tok.c_str() + eq + 1);
    if (key == "build_lds") d.build.build_lds = val != 0;
    else if (key == "build_atomic") d.build.build_atomic = val != 0;
    else if (key == "build_stream") d.build.build_stream = val != 0;
    else if (key == "build_runs") d.build.build_runs = val != 0;
    else if (key == "run_range") d.build.run_range = val;
    else if (key == "run_lanes") d.build.run_lanes = val;
    else if (key == "run_sub") d.build.run_sub = val;
    else if (key == "build_trace") d.build_trace = val != 0;
    else if (key == "chunk8") d.filter.chunk8 = val != 0;
    else if (key == "shard_exact") d.shard_exact = val != 0;
    else if (key == "diag") d.diag = val != 0;
    else if (key == "force_general") d.force_general = val != 0;
    else if (key == "exact_accum") d.exact_accum = val != 0;
    else if (key == "cx_tile") d.cx_tile = val;
    else if (key == "window") d.filter.window = val;
    else if (key == "chunks") d.chunks = val;
    else if (key == "tiles_per_launch") d.tiles_per_launch = val;
    else if (key == "no_tail") d.no_tail = val != 0;
    else if (key == "no_acc8") d.filter.no_acc8 = val != 0;
    else if (key == "no_planes") d.filter.no_planes = val != 0;
    else if (key == "planes") d.filter.planes = val != 0;
    else if (key == "no_even") d.filter.no_even = val != 0;
    else if (key == "flat_group") d.filter.flat_group = (int)val;
    else if (key == "seg_align") d.seg_align = val;
    else if (key == "fold_w") d.fold_w = val;
    else if (key == "mix") d.mix = val;
    else if (key == "no_sym") d.no_sym = val != 0;
    else if (key == "no_chain") d.no_chain = val != 0;
    else if (key == "no_append") d.no_append = val != 0;
    else if (key == "head_bf16") d.head_bf16 = val != 0;
    else if (key == "res_cap") d.res_cap = val;
    else if (key == "no_bucket") d.build.no_bucket = val != 0;
    else if (key == "merge") d.filter.merge = (int)val;
    else if (key == "merge_u") d.filter.merge_u = (int)val;
    else if (key == "no_merge_prune") d.no_merge_prune = val != 0;
    else if (key == "merge_single") d.filter.merge_single = (int)val;
    else if (key == "no_fused_ingest") d.no_fused_ingest = val != 0;
    else if (key == "no_persist") d.no_persist = val != 0;
    else if (key == "persist_wgs") d.persist_wgs = val;
    else if (key == "persist_fine") d.persist_fine = val;
    else if (key == "rm_grid") d.rm_grid = val;
    else if (key == "tp_grid") d.tp_grid = val;
    else if (key == "cc_grid") d.cc_grid = val;
    else if (key == "relayout_fail") {}  // (read by apss_group_create: a group's re-layout hook, nothing of a handle's)
    else if (!key.empty()) fprintf(stderr, "[apss] unknown APSS_DEBUG token '%s' ignored\n", key.c_str());
  }
  return d;
}

constexpr size_t kPinBytes = 256 << 10;   // pinned staging of a small batch / a small answer ...
constexpr size_t kPinScalars = 1024;      // ... + this much behind it for the small device-to-host reads:

// one member per readback, each in cache lines of its own (a read lands while the host works on another)
struct PinScalars {
  alignas(128) unsigned int ingest_flags[4];               // the flag words of an ingest kernel / of k_qs_gather
  alignas(128) unsigned long long chain_ctr[kCtrCount];    // the chained exact pass's counters
  alignas(128) unsigned long long attempt_ctr[kCtrCount];  // the filter's counters of one attempt
  alignas(512) unsigned long long removal_kept;            // pairs k_rm_drop kept
  alignas(128) int64_t stored_back[4];                     // apss_query_stored: the two scan totals, the two id counters
  alignas(128) unsigned long long top_pairs[kTpWords];     // the global top-K's state words
  alignas(128) unsigned long long components[kCcWords];    // apss_set_components: unions, components, singletons, largest
};
static_assert(sizeof(PinScalars) <= kPinScalars, "the scalar slots end inside the pinned reservation");
static_assert(offsetof(PinScalars, chain_ctr) == 128 && offsetof(PinScalars, attempt_ctr) == 256 && offsetof(PinScalars, removal_kept) == 512 &&
                  offsetof(PinScalars, stored_back) == 640 && offsetof(PinScalars, top_pairs) == 768,
              "every readback keeps the cache lines it had");

}  // namespace

struct apss_handle {
  apss_config cfg{};
  DebugCfg dbgcfg;
  int dev = 0;
  // (what the arrays below are counted in and run on stands in front of them: it is destroyed after them)
  size_t bytes_reserved = 0;  // device bytes the handle's arrays hold (apss_stats.hbm_bytes): every array grows against it
  DevStream own_stream;
  hipStream_t stream = nullptr;
  DevEvent ev0, ev1;
  std::string err;
  bool sharded = false;
  bool nonneg = true;    // every stored weight so far is >= 0
  bool q_nonneg = true;  // every weight of the staged query batch is >= 0 (decided per call: a signed query batch does not change the handle)
  bool no_acc8 = false;  // the 8-bit filter proved unusable on this handle's data: 16-bit accumulators until apss_clear
  uint32_t downgrades = 0;  // APSS_DOWNGRADE_* (apss_stats): permanent fallbacks this handle has taken since the last clear
  int64_t store_max_nnz = 0, q_max_nnz = 0;  // longest row of the store / of the staged query batch
  float store_max_norm2 = 0.f, q_max_norm2 = 0.f;  // largest squared row norm (bounds every partial score)
  int64_t store_nonempty = 0;  // stored rows with at least one indexed entry (each touches itself in a self-join)
  int64_t last_batch_nonempty = 0;
  int32_t cb = 16384;
  bool stored_rows = false;  // the rows being ingested passed this configuration's filters already (apss_insert_stored_dev)

  // store (CSR) -- vectorsStore, IWA:22
  int64_t n_rows = 0, nnz = 0;
  int64_t idx_rows = 0;  // rows [0, idx_rows) are in the tile index (and in W); rows [idx_rows, n_rows) wait in the tail (probe: k_tail_score)
  DevBuf<int64_t> rowptr, ext;
  DevBuf<int32_t> idx;
  DevBuf<uint32_t> erow;  // store row of every entry
  DevBuf<float> val, sub;  // sub: shard sub-norm per row (sharded only)
  // index (tile-major CSC) -- invertedIndex, IWA:25.  Two renderings of the same posting lists:
  //   ex: exact, 8-B postings, `cb` rows per tile      (k_probe_wave, k_probe, shard mode)
  //   cx: coarse, 4-B postings, up to 2*cb rows per tile (k_probe_coarse, the filter of the two-pass join)
  struct IndexSet {
    int32_t cb = 0;
    int32_t align = 0;
    bool coarse = false;
    int64_t n_tiles = 0, post_used = 0;
    DevBuf<uint2> seg;
    DevBuf<Posting> post;
    DevBuf<uint32_t> post_c;
    DevBuf<int64_t> base, total;
    DevBuf<uint32_t> scan_part;  // block sums of the segment-length scan (k_tile_scan_part)
    DevBuf<uint32_t> maxlen;   // [2] longest (tile, term) segment, number of long segments, over the builds since the rendering was last started from tile 0
    uint32_t max_seg = 0;      // host copies
    uint32_t long_segs = 0;
    DevBuf<unsigned long long> chunkw;  // [1] sum over (tile, term) of length x chunks (k_tile_scan)
    double round_chunks = 0.0;          // chunks an average stored row deals out per round (tile): chunkw / rows
    std::vector<int64_t> h_base;
    double build_ms = 0;
    int64_t built_rows = 0;  // the rendering covers store rows [0, built_rows) (an append needs to start exactly there)
  };
  IndexSet ex, cx;
  bool use_coarse = false;  // build and use the coarse index (non-sharded handles without APSS_FLAG_EXACT_ACCUM)
  int64_t n_tiles = 0;      // tiles of the exact rendering (apss_stats)
  int64_t ex_built_rows = 0;     // the exact rendering covers rows [0, ex_built_rows)
  DevBuf<float> tile_min, tile_min_c;  // shard mode: min positive sub-norm per exact / coarse tile
  // query staging (apss_query: batch not stored)
  DevBuf<int64_t> q_rowptr, q_ext;
  DevBuf<int32_t> q_idx;
  DevBuf<float> q_val, q_sub;
  // ingest scratch
  DevBuf<int64_t> s_keep, s_cnt, s_rowdst, s_nnzdst, in_rowptr, in_ext;
  DevBuf<int64_t> scan_tmp;  // block sums of a multi-block scan and their scan
  DevBuf<int32_t> in_idx;
  DevBuf<float> s_inv, s_sub, in_val;
  DevBuf<double> in_val64;
  DevBuf<unsigned long long> bk_cnt;  // bucketed LDS build (large dims): entries per (tile, term range) + cursors,
  DevBuf<int64_t> bk_base;            //   their exclusive scan,
  DevBuf<int32_t> bk_idx;             //   and the entries partitioned by (tile, range): term, store row, value
  DevBuf<uint32_t> bk_erow;
  DevBuf<float> bk_val;
  DevBuf<uint32_t> run_cut;           // run-reading LDS build: per-row range cuts of the rows being built (k_row_cuts)
  DevBuf<uint2> run_ent;              //   ... and the entries partitioned by (tile, sub-range) for its two-pass scatter
  // the same cuts as k_ingest_plain leaves them while it stores a plain batch: [store row][cut_ranges + 1], valid for the store
  // rows [cut_lo, cut_hi) of a rendering with cut_cb rows per tile and ranges of cut_rt terms (build_tiles takes them when they
  // cover the rows it builds, and computes its own otherwise)
  // (indexed by ABSOLUTE store row on purpose: build_tiles hands k_tile_runs `ing_cut + r0 * (ranges + 1)` whatever cut_lo is,
  // and an appended batch extends the table in place; a table that starts over at row cut_lo > 0 leaves the rows below unused --
  // (ranges + 1) x 4 B per store row, 32 MB at C3 -- and like every buffer of the handle it only grows)
  DevBuf<uint32_t> ing_cut;
  int64_t cut_lo = 0, cut_hi = 0;
  int32_t cut_cb = 0, cut_rt = 0, cut_ranges = 0;
  // ... and the sampled document frequencies of a batch that went into an empty store: valid for a head policy that looks at
  // exactly the store rows [0, df_rows) with this stride (choose_head)
  std::vector<uint32_t> df_host;
  int64_t df_rows = -1, df_stride = 0;
  DevBuf<uint2> app_seg;             // append build: the last tile's segment table and postings before the append
  DevBuf<char> app_post;
  DevBuf<int32_t> vq_first, vrow_q;  // virtual-row table of the last query batch (queries of > 512 terms)
  DevBuf<int64_t> vrow_ptr, vrow_np, vrow_first;
  // results of the last query-type call
  PairList res, fin;          // the filters' candidates; the exact pass's final list
  PairList res2;              // merged rounds (k_expand_merged): the second candidate list, swapped with res after the expansion
  DevBuf<float> q_prenorm;    // ... and the staged query weights divided by their rows' shard factors
  const int32_t *out_q = nullptr, *out_c = nullptr;  // where the last call's results live (res or fin)
  const float *out_s = nullptr;
  int64_t n_res = -1;
  const int64_t *res_q_ext = nullptr;      // ext ids of the last query batch (device)
  const int64_t *last_q_rowptr = nullptr;  // last query batch CSR (device), for apss_partial_scores_dev
  const int32_t *last_q_idx = nullptr;
  const float *last_q_val = nullptr;
  int64_t last_nq = 0;
  DevBuf<unsigned long long> counters, dbg, chain_ctr;
  DevBuf<unsigned int> flagword;
  // small messages (single vectors, batches of a few dozen: the reference's LoadGenerator sends ONE vector per message): the
  // batch crosses PCIe as one packed copy out of pinned memory and the answer comes back the same way
  PinBuf<char> pin;                // pinned host staging, kPinBytes + kPinScalars
  PinScalars own_scalars{};        // (without pinned memory: pageable copies of the scalar slots)
  PinScalars *scalars = &own_scalars;  // where the small device-to-host reads land: behind `pin`, or own_scalars
  DevBuf<char> pack;               // its device twin
  const int64_t *up_rowptr = nullptr, *up_ext = nullptr;  // where upload() left the batch (the in_* arrays, or views into `pack`)
  const int32_t *up_idx = nullptr;
  // dense-head block (apss_head.hpp): the KH most frequent terms live in W instead of the inverted index
  int32_t head_k = 0;                 // 0: no block
  bool head_fixed = false;            // the block's terms were set through apss_set_head_terms: no policy, kept across apss_clear
  // geometry of a head of more than 256 terms: ONE block of 256 columns -- the head_exact most frequent terms with a column
  // each, the others FOLDED into the remaining head_fold_w = 256 - head_exact columns.  (APSS_DEBUG=fold_w=128|256 keeps
  // round 3's first form for comparison: 256 columns with a term each + a second block of fold_w folded columns.)
  int32_t head_fold_w = 128;
  int32_t head_exact = 128;
  int32_t head_fold_user = 0;         // folded columns named by the caller for the terms it sets (apss_set_head_fold; 0: 128)
  bool merge_off = false;             // term shard: merged rounds (apss_even.hpp) reported too many candidates on this data: not again (until apss_clear)
  bool head_longseg = false;          // term shard with a block: its tail still has segments too long for the thin-round kernel (a
                                      // hint kept across apss_clear: the next first build goes straight to the layout that serves them)
  int32_t head_part = 0, head_parts = 1;  // this handle multiplies the candidate tiles t % head_parts == head_part of the block
  int64_t head_eval_rows = 0;         // store size when the head policy last looked at the term distribution
  bool head_blocked = false;          // a call needed the plain path: no block until the next apss_clear
  std::vector<int32_t> head_terms;    // the block's terms, in block order
  DevBuf<int32_t> head_pos;           // [dim] term -> column of the block | -1
  // tail view (apss_head.hpp): the rows without the block's entries -- index build input and the sparse filter's query rows
  struct TailView {
    DevBuf<int64_t> rowptr;
    DevBuf<int32_t> idx;
    DevBuf<float> val;
    DevBuf<uint32_t> erow;
    int64_t rows = 0, nnz = 0, max_nnz = 0, nonempty = 0, last_nonempty = 0;
  };
  TailView tv, qtv;                   // of the store rows [0, idx_rows); of the staged (outside) query batch
  DevBuf<int64_t> tv_cnt, tv_off;
  DevBuf<unsigned int> tv_sum;
  DevBuf<uint16_t> W, q_W;            // [rows x head_k] rows of the store / of a staged query batch: bf16, or INT8 in the first half
                                      // of the same reservation (head_i8: one byte per column, rounded up; apss_head.hpp)
  bool head_i8 = false;               // the block's rows are the INT8 rendering (decided when the block's first row is packed)
  float head_s = 0.f;                 // the INT8 scale S (units per 1.0): 127 / the largest row norm so far (head_fit_scale)
  DevBuf<unsigned int> head_ovf;      // [1] set by k_head_pack if an element ever exceeded 127 (cannot happen: checked, an error)
  DevBuf<uint32_t> df;
  DevBuf<unsigned long long> dedup_tab, head_ctr;
  PairList uq;                        // candidate list after k_pair_dedup
  int64_t head_nonempty = 0, last_batch_head_nonempty = 0;
  double head_sample_frac = 0.0;      // fraction of sampled pairs the dense filter passed when the policy last looked
  DevEvent ev2, ev3;
  // per-query top-k (apss_topk.hpp): the setting, the pass's buffers, what the last query-type call did
  int32_t top_k = 0;
  TopkWork topk;
  apss_topk_info tk{};
  // ... in windows of query rows (apss_window.hpp): the budget, the plan's buffers, the call's own output arrays (probe_inner may
  // rebuild or regrow anything else while earlier windows' kept lists wait there), what the last query-type call did
  int64_t top_k_window = 0;
  DevBuf<unsigned int> win_df;  // [dim] exact term counts of the store, recomputed at every windowed call
  DevBuf<int32_t> win_b;        // [nq] b(q), and behind it [nq] the rows' non-empty bits (stored batch of a handle with a head)
  PairList win;
  std::vector<int64_t> win_cuts;
  apss_topk_window_info tw{};
  // a windowed call's self-touch corrections: non-empty rows of the window being probed (-1: not in a window)
  int64_t win_nonempty = -1, win_head_nonempty = -1;
  // ... with each (query row, tile) round cut inside k_probe<2> (apss_set_top_k_tile_cut): the setting, the rows' uncut counts
  // of the probe that last ran (probe_inner: cut_ran, cut_uncut, cut_rounds), what the last query-type call did
  bool tile_cut = false, cut_ran = false;
  int64_t cut_uncut = 0, cut_rounds = 0;
  DevBuf<uint32_t> row_pairs;  // [nq]
  apss_topk_tile_cut_info tci{};
  int64_t probe_reruns = 0;    // probes that ran again because a list overflowed, since create
  // removal (apss_remove.hpp): one mark byte per slot -- slots [0, dead_rows) have one, rows stored since then are live and get
  // theirs (0) when the map is next needed --, the rows marked now, the sorted removal list and the sort's scratch, the filtered
  // final list of a query-type call, what the last calls did
  DevBuf<uint8_t> dead;
  int64_t dead_rows = 0, rm_marked = 0;
  DevBuf<int64_t> rm_ids, rm_sorted;
  DevBuf<char> rm_tmp;
  DevBuf<unsigned long long> rm_ctr;  // [1] rows newly marked / pairs kept
  PairList rm_out;
  DevEvent rm_ev0, rm_ev1;  // (made where they are first recorded: begin_timed / end_timed_read)
  double auto_compact = 0.0;
  apss_removal_info ri{};
  // stored rows as a query batch (apss_query_stored.hpp): the found bytes of the sorted id list (which lives in rm_sorted), the id
  // counters, the compact slot list, the events of the two phases, what the last call did
  DevBuf<uint8_t> qs_found;
  DevBuf<unsigned long long> qs_ctr;  // [2] distinct ids / distinct ids that selected nothing
  DevBuf<int32_t> qs_slots;
  DevEvent qs_ev[4];  // (made where they are first recorded)
  apss_stored_query_info qsi{};
  // global top-K (apss_top_pairs.hpp): the setting, the stage's buffers, what the last query-type call did
  int64_t top_pairs = 0;
  TpWork tp;
  apss_top_pairs_info tpi{};
  // components of the join (apss_components.hpp): the setting, the forest and its labels, what the last calls did (cci.on,
  // cci.complete, cci.resets are the structure's state; rows, the counts and unions_total are filled at a labelling)
  bool cc_on = false;
  CcWork cc;
  apss_components_info cci{};
  // ... across a removal and a compaction (apss_components_repair.hpp): the budget (0: off), the stage's event pair, what the last
  // calls did
  int64_t ccr_max = 0;
  DevEvent cr_ev0, cr_ev1;  // (made where they are first recorded)
  apss_components_repair_info ccri{};
  // persistent filter launches (apss_worklist.hpp): the work lists of the last call's launches, one behind the other in
  // pinned memory and on the device, kept until a call's keys differ; workgroups per CU of each instantiation as queried
  std::vector<apss::WorkListKey> wl_keys;
  std::vector<int64_t> wl_off, wl_fine;  // [launches + 1] first item of every launch's list; [launches] its cut pieces
  PinBuf<apss::ProbeItem> wl_pin;
  DevBuf<apss::ProbeItem> wl_dev;
  DevEvent wl_ev{kUntimed};              // the last upload out of wl_pin
  std::map<const void *, int> wl_per_cu;
  int n_cus = 0;
  // stats
  apss_stats st{};
};

namespace {

#define HIPCHK(h, expr)                                                                              \
  do {                                                                                               \
    hipError_t e_ = (expr);                                                                          \
    if (e_ != hipSuccess) {                                                                          \
      (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                                  \
      return e_ == hipErrorOutOfMemory ? APSS_E_NOMEM : APSS_E_DEVICE;                               \
    }                                                                                                \
  } while (0)

#define APSS_TRY(expr)          \
  do {                          \
    int32_t rc_ = (expr);       \
    if (rc_ != APSS_OK) return rc_; \
  } while (0)

int32_t fail(apss_handle *h, int32_t rc, const std::string &msg) {
  h->err = msg;
  return rc;
}

// grow-only device array; keeps the first `keep` elements.  (A failed growth leaves the array, and the reservation, as they were)
template <class T>
int32_t ensure(apss_handle *h, DevBuf<T> &b, size_t n, size_t keep = 0, bool exact = false) {
  HIPCHK(h, b.grow(exact ? kGrowHandleExact : kGrowHandle, n, keep, h->stream, &h->bytes_reserved));
  return APSS_OK;
}

int32_t PairList::ensure(apss_handle *h, size_t n, size_t keep, bool exact) {
  HIPCHK(h, grow_all(exact ? kGrowHandleExact : kGrowHandle, n, keep, h->stream, &h->bytes_reserved, q, c, s));
  return APSS_OK;
}

int32_t enter(apss_handle *h) {
  if (!h) return APSS_E_INVALID;
  hipError_t e = hipSetDevice(h->dev);
  if (e != hipSuccess) return fail(h, APSS_E_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
  return APSS_OK;
}

// ---- ingest: validate (+ optional normalise / admission / value prune / term-range filter) and append ----
// Source arrays are device pointers (batch-relative rowptr).  Destination: the store (to_store) or the query
// staging buffers.  *n_out / *nnz_out: rows / entries that survived.
// exclusive scan of n int64 (n + 1 outputs, out[n] = total) on the handle's stream; *launches (if given) += the kernels it launched
int32_t scan_i64(apss_handle *h, const int64_t *in, int64_t *out, int64_t n, int32_t *launches = nullptr) {
  if (n <= 4 * kScanBlock) {
    hipLaunchKernelGGL(k_scan_i64, dim3(1), dim3(1024), 0, h->stream, in, out, n);
    HIPCHK(h, hipGetLastError());
    if (launches) *launches += 1;
    return APSS_OK;
  }
  const int64_t nb = ceil_div(n, kScanBlock);
  APSS_TRY(ensure(h, h->scan_tmp, (size_t)(2 * nb + 1)));
  int64_t *sums = h->scan_tmp.p, *offs = h->scan_tmp.p + nb;
  hipLaunchKernelGGL(k_scan_sums, dim3((unsigned)nb), dim3(1024), 0, h->stream, in, sums, n);
  hipLaunchKernelGGL(k_scan_i64, dim3(1), dim3(1024), 0, h->stream, (const int64_t *)sums, offs, nb);
  hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)nb), dim3(1024), 0, h->stream, in, (const int64_t *)offs, out, n, nb);
  HIPCHK(h, hipGetLastError());
  if (launches) *launches += 3;
  return APSS_OK;
}

int32_t head_setup_rendering(apss_handle *h);
int32_t head_fit_scale(apss_handle *h, double norm2, unsigned char *W, int64_t packed_bytes);
inline void head_pack_rendering(const apss_handle *h, HeadPackArgs &p);

bool ingest_wants_cuts(const apss_handle *h, int64_t dst_row0, int64_t n, int64_t nnz, int32_t *cb, int32_t *rt, int32_t *n_ranges);
bool head_policy_due(const apss_handle *h, int64_t n_rows);

// what the flag words of an ingest kernel say about the batch: the error of a rejected batch (nothing of the handle has
// changed by then), or the batch's summaries folded into the handle's
int32_t take_ingest_flags(apss_handle *h, const unsigned int *flags_host, bool to_store) {
  if (flags_host[0] & 1u)
    return fail(h, APSS_E_INVALID, "malformed vector: indices must be strictly increasing and in [0, dim) "
                                   "(SparseVector.scala:75; vectorDim mismatch is the require of CommonUtils.scala:99)");
  if (flags_host[0] & 2u) return fail(h, APSS_E_INVALID, "non-finite value in a vector");
  if (to_store) h->nonneg = h->nonneg && !(flags_host[0] & 4u);
  else h->q_nonneg = !(flags_host[0] & 4u);
  float norm2;
  std::memcpy(&norm2, &flags_host[2], sizeof(float));
  if (to_store) {
    h->store_max_nnz = std::max<int64_t>(h->store_max_nnz, flags_host[1]);
    h->store_max_norm2 = std::max(h->store_max_norm2, norm2);
    h->store_nonempty += flags_host[3];
    h->last_batch_nonempty = flags_host[3];
  } else {
    h->q_max_nnz = flags_host[1];
    h->q_max_norm2 = norm2;
  }
  return APSS_OK;
}

// A PLAIN batch (no term range, normalise, prune or admission) in one pass, k_ingest_plain: every row and entry is kept, so the
// destination is sized before the launch and the flag word is read once, behind it.  A store batch also leaves the range cuts
// of its rows when the index build is expected to read runs, and the df sample when it is the store's first rows and the head
// policy will look at them.
int32_t ingest_plain(apss_handle *h, int64_t n, int64_t nnz, const int64_t *d_rowptr, const int32_t *d_idx, const float *d_val,
                     const int64_t *d_ext, bool to_store, int64_t *n_out, int64_t *nnz_out) {
  APSS_TRY(ensure(h, h->flagword, 4));
  const int64_t dst_row0 = to_store ? h->n_rows : 0, dst_nnz0 = to_store ? h->nnz : 0;
  DevBuf<int64_t> &o_rowptr = to_store ? h->rowptr : h->q_rowptr;
  DevBuf<int64_t> &o_ext = to_store ? h->ext : h->q_ext;
  DevBuf<int32_t> &o_idx = to_store ? h->idx : h->q_idx;
  DevBuf<float> &o_val = to_store ? h->val : h->q_val;
  APSS_TRY(ensure(h, o_rowptr, (size_t)(dst_row0 + n + 1), (size_t)(to_store ? dst_row0 + 1 : 0)));
  APSS_TRY(ensure(h, o_ext, (size_t)(dst_row0 + n), (size_t)dst_row0));
  APSS_TRY(ensure(h, o_idx, (size_t)(dst_nnz0 + nnz), (size_t)dst_nnz0));
  APSS_TRY(ensure(h, o_val, (size_t)(dst_nnz0 + nnz), (size_t)dst_nnz0));
  if (to_store) APSS_TRY(ensure(h, h->erow, (size_t)(dst_nnz0 + nnz), (size_t)dst_nnz0));
  HIPCHK(h, hipMemsetAsync(h->flagword.p, 0, 4 * sizeof(unsigned int), h->stream));
  if (dst_row0 == 0) HIPCHK(h, hipMemsetAsync(o_rowptr.p, 0, sizeof(int64_t), h->stream));

  IngestPlainArgs p{};
  IngestArgs &a = p.w.in;
  a.n = n;
  a.nnz = nnz;
  a.rowptr = d_rowptr;
  a.idx = d_idx;
  a.val = d_val;
  a.dim = h->cfg.dim;
  a.flags_out = h->flagword.p;
  p.w.dst_row0 = dst_row0;
  p.w.dst_nnz0 = dst_nnz0;
  p.w.o_rowptr = o_rowptr.p;
  p.w.o_idx = o_idx.p;
  p.w.o_val = o_val.p;
  p.w.o_ext = o_ext.p;
  p.w.o_erow = to_store ? h->erow.p : nullptr;
  p.w.ext = d_ext;
  // range cuts: appended to the table when it ends where this batch starts, in the same form; otherwise the table starts over
  int32_t cut_cb = 0, cut_rt = 0, cut_ranges = 0;
  const bool cuts = to_store && ingest_wants_cuts(h, dst_row0, n, nnz, &cut_cb, &cut_rt, &cut_ranges);
  bool cuts_extend = false;
  if (cuts) {
    cuts_extend = h->cut_hi > h->cut_lo && h->cut_hi == dst_row0 && h->cut_cb == cut_cb && h->cut_rt == cut_rt && h->cut_ranges == cut_ranges;
    if (!cuts_extend) h->cut_lo = h->cut_hi = 0;  // (the rows written below overwrite it)
    const size_t cw = (size_t)cut_ranges + 1;
    APSS_TRY(ensure(h, h->ing_cut, (size_t)(dst_row0 + n) * cw, cuts_extend ? (size_t)dst_row0 * cw : 0));
    p.cut = h->ing_cut.p;
    p.n_ranges = cut_ranges;
    p.range_terms = cut_rt;
    p.cb = cut_cb;
  }
  // df sample: the head policy would look at exactly this batch (choose_head: rows [0, n), the same stride)
  const bool sample = to_store && dst_row0 == 0 && head_policy_due(h, n);
  const int32_t dim = h->cfg.dim;
  if (to_store) h->df_rows = -1;
  if (sample) {
    APSS_TRY(ensure(h, h->df, (size_t)dim));
    HIPCHK(h, hipMemsetAsync(h->df.p, 0, (size_t)dim * sizeof(uint32_t), h->stream));
    p.df = h->df.p;
    p.df_stride = std::max<int64_t>(1, n / 65536);
    h->df_host.resize((size_t)dim);
  }
  const int threads = 256;
  const int64_t blocks = ceil_div(n * kGroup, threads);
  // (the workgroups loop over their rows: few workgroups = few same-address atomics on the batch summaries)
  hipLaunchKernelGGL(k_ingest_plain, dim3((unsigned)std::min<int64_t>(blocks, 4096)), dim3(threads), 0, h->stream, p);
  HIPCHK(h, hipGetLastError());
  unsigned int *flags_host = h->scalars->ingest_flags;
  HIPCHK(h, hipMemcpyAsync(flags_host, h->flagword.p, 4 * sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream));
  if (sample) HIPCHK(h, hipMemcpyAsync(h->df_host.data(), h->df.p, (size_t)dim * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (h->dbgcfg.diag)
    fprintf(stderr, "[apss diag] ingest fused: %lld %s rows at %lld, cuts %s, df sample %s\n", (long long)n, to_store ? "store" : "query",
            (long long)dst_row0, cuts ? (cuts_extend ? "appended" : "written") : "none", sample ? "taken" : "none");
  // a rejected batch commits nothing: the store's extent, its summaries and the cut table's are what they were, and what the
  // kernel wrote beyond them is dead
  APSS_TRY(take_ingest_flags(h, flags_host, to_store));
  if (cuts) {
    if (!cuts_extend) h->cut_lo = dst_row0;
    h->cut_hi = dst_row0 + n;
    h->cut_cb = cut_cb;
    h->cut_rt = cut_rt;
    h->cut_ranges = cut_ranges;
  }
  if (sample) {
    h->df_rows = n;
    h->df_stride = p.df_stride;
  }
  *n_out = n;
  *nnz_out = nnz;
  return APSS_OK;
}

int32_t ingest(apss_handle *h, int64_t n, int64_t nnz, const int64_t *d_rowptr, const int32_t *d_idx,
               const float *d_val, const int64_t *d_ext, bool to_store, int64_t *n_out, int64_t *nnz_out) {
  *n_out = 0;
  *nnz_out = 0;
  if (n == 0) return APSS_OK;
  // rows out of a store (apss_insert_stored_dev) were normalised, pruned and admitted when they first came in: a second pass
  // would change them (a pruned row re-normalised) or drop them (admission on the pruned sum)
  const uint32_t in_flags = h->stored_rows ? h->cfg.flags & ~(APSS_FLAG_VALUE_PRUNE | APSS_FLAG_ADMISSION | APSS_FLAG_NORMALIZE) : h->cfg.flags;
  const bool transform = h->sharded || (in_flags & (APSS_FLAG_VALUE_PRUNE | APSS_FLAG_ADMISSION | APSS_FLAG_NORMALIZE));
  if (!transform && !h->dbgcfg.no_fused_ingest) return ingest_plain(h, n, nnz, d_rowptr, d_idx, d_val, d_ext, to_store, n_out, nnz_out);
  if (h->dbgcfg.diag)
    fprintf(stderr, "[apss diag] ingest unfused: %lld %s rows at %lld (%s)\n", (long long)n, to_store ? "store" : "query",
            (long long)(to_store ? h->n_rows : 0), transform ? "transform" : "no_fused_ingest");
  APSS_TRY(ensure(h, h->s_keep, (size_t)n + 1));
  APSS_TRY(ensure(h, h->s_cnt, (size_t)n + 1));
  APSS_TRY(ensure(h, h->s_inv, (size_t)n));
  APSS_TRY(ensure(h, h->s_sub, (size_t)n));
  APSS_TRY(ensure(h, h->flagword, 4));
  HIPCHK(h, hipMemsetAsync(h->flagword.p, 0, 4 * sizeof(unsigned int), h->stream));

  IngestArgs a{};
  a.n = n;
  a.nnz = nnz;
  a.rowptr = d_rowptr;
  a.idx = d_idx;
  a.val = d_val;
  a.dim = h->cfg.dim;
  a.term_lo = h->cfg.term_lo;
  a.term_hi = h->cfg.term_hi;
  a.flags = in_flags;
  a.theta = (float)h->cfg.theta;
  a.index_threshold = (float)h->cfg.index_threshold;
  a.row_keep = h->s_keep.p;
  a.row_cnt = h->s_cnt.p;
  a.row_inv = h->s_inv.p;
  a.row_sub = h->s_sub.p;
  a.flags_out = h->flagword.p;
  const bool shard_head = h->sharded && h->head_k > 0;
  a.head_pos = shard_head ? h->head_pos.p : nullptr;
  const int threads = 256;
  const int64_t blocks = ceil_div(n * kGroup, threads);
  // (the workgroups loop over their rows: few workgroups = few same-address atomics on the batch summaries)
  hipLaunchKernelGGL(k_ingest_count<kGroup>, dim3((unsigned)std::min<int64_t>(blocks, 4096)), dim3(threads), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());

  // destination
  int64_t dst_row0 = to_store ? h->n_rows : 0, dst_nnz0 = to_store ? h->nnz : 0;
  int64_t kept_rows = n, kept_nnz = nnz;
  // (read back into pinned memory when the handle has it: a copy into pageable memory is staged by the runtime)
  unsigned int *flags_host = h->scalars->ingest_flags;
  if (transform) {
    APSS_TRY(ensure(h, h->s_rowdst, (size_t)n + 1));
    APSS_TRY(ensure(h, h->s_nnzdst, (size_t)n + 1));
    APSS_TRY(scan_i64(h, (const int64_t *)h->s_keep.p, h->s_rowdst.p, n));
    APSS_TRY(scan_i64(h, (const int64_t *)h->s_cnt.p, h->s_nnzdst.p, n));
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(&kept_rows, h->s_rowdst.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&kept_nnz, h->s_nnzdst.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(h, hipMemcpyAsync(flags_host, h->flagword.p, 4 * sizeof(unsigned int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  APSS_TRY(take_ingest_flags(h, flags_host, to_store));

  DevBuf<int64_t> &o_rowptr = to_store ? h->rowptr : h->q_rowptr;
  DevBuf<int64_t> &o_ext = to_store ? h->ext : h->q_ext;
  DevBuf<int32_t> &o_idx = to_store ? h->idx : h->q_idx;
  DevBuf<float> &o_val = to_store ? h->val : h->q_val;
  DevBuf<float> &o_sub = to_store ? h->sub : h->q_sub;
  APSS_TRY(ensure(h, o_rowptr, (size_t)(dst_row0 + kept_rows + 1), (size_t)(to_store ? dst_row0 + 1 : 0)));
  APSS_TRY(ensure(h, o_ext, (size_t)(dst_row0 + kept_rows), (size_t)dst_row0));
  APSS_TRY(ensure(h, o_idx, (size_t)(dst_nnz0 + kept_nnz), (size_t)dst_nnz0));
  APSS_TRY(ensure(h, o_val, (size_t)(dst_nnz0 + kept_nnz), (size_t)dst_nnz0));
  if (to_store) APSS_TRY(ensure(h, h->erow, (size_t)(dst_nnz0 + kept_nnz), (size_t)dst_nnz0));
  if (h->sharded) APSS_TRY(ensure(h, o_sub, (size_t)(dst_row0 + kept_rows), (size_t)dst_row0));
  if (dst_row0 == 0) HIPCHK(h, hipMemsetAsync(o_rowptr.p, 0, sizeof(int64_t), h->stream));

  IngestWriteArgs w{};
  w.in = a;
  w.dst_row0 = dst_row0;
  w.dst_nnz0 = dst_nnz0;
  w.o_rowptr = o_rowptr.p;
  w.o_idx = o_idx.p;
  w.o_val = o_val.p;
  w.o_ext = o_ext.p;
  w.o_sub = h->sharded ? o_sub.p : nullptr;
  w.o_erow = to_store ? h->erow.p : nullptr;
  w.ext = d_ext;
  if (transform) {
    w.row_dst = h->s_rowdst.p;
    w.nnz_dst = h->s_nnzdst.p;
  } else {
    // identity placement: row r -> r, entry k -> k (the batch rowptr is the entry scan)
    w.row_dst = nullptr;
    w.nnz_dst = d_rowptr;
  }
  hipLaunchKernelGGL(k_ingest_write, dim3((unsigned)blocks), dim3(threads), 0, h->stream, w);
  HIPCHK(h, hipGetLastError());
  if (shard_head) {
    // the rows of the dense-head block come from the batch as the caller handed it in (whole rows: the store keeps this
    // shard's term range only); rows map 1:1 (apss_set_head_terms refuses the admission filter on a shard)
    const int64_t kh = h->head_k;
    DevBuf<uint16_t> &o_W = to_store ? h->W : h->q_W;
    const int64_t rows_end = dst_row0 + kept_rows;
    const int64_t w_pad = to_store ? ceil_div(rows_end, kHeadQBlock) * kHeadQBlock + kHeadCTile : ceil_div(rows_end, kHeadCTile) * kHeadCTile;
    APSS_TRY(ensure(h, o_W, (size_t)(w_pad * kh), (size_t)(ceil_div(dst_row0, kHeadCTile) * kHeadCTile * kh)));
    APSS_TRY(ensure(h, h->head_ctr, 4));
    HIPCHK(h, hipMemsetAsync(h->head_ctr.p, 0, 4 * sizeof(unsigned long long), h->stream));
    if (to_store && dst_row0 == 0) APSS_TRY(head_setup_rendering(h));
    APSS_TRY(head_fit_scale(h, to_store ? (double)h->store_max_norm2 : std::max((double)h->store_max_norm2, (double)h->q_max_norm2),
                            reinterpret_cast<unsigned char *>(h->W.p), ceil_div(to_store ? dst_row0 : h->n_rows, kHeadCTile) * kHeadCTile * kh));
    HeadPackArgs p{};
    head_pack_rendering(h, p);
    p.rowptr = d_rowptr;
    p.idx = d_idx;
    p.val = d_val;
    p.row0 = 0;
    p.row1 = n;
    p.head_pos = h->head_pos.p;
    p.kh = (int32_t)kh;
    p.W = o_W.p;
    p.w_row0 = dst_row0;
    p.w_pad = w_pad;
    p.ratio_t = nullptr;  // k_ingest_count wrote this shard's ratio
    p.head_nonempty = reinterpret_cast<unsigned int *>(h->head_ctr.p);
    p.row_inv = (in_flags & APSS_FLAG_NORMALIZE) ? h->s_inv.p : nullptr;
    p.prune_above = (in_flags & APSS_FLAG_VALUE_PRUNE) ? (float)h->cfg.index_threshold : -INFINITY;
    p.fold_from = h->head_exact;
    p.part = h->head_part;  // (a stored query's product with itself is counted by the shard that owns its tile)
    p.n_parts = h->head_parts;
    hipLaunchKernelGGL(k_head_pack, dim3((unsigned)(ceil_div(w_pad, 8) - dst_row0 / 8)), dim3(512), 0, h->stream, p);
    HIPCHK(h, hipGetLastError());
    if (to_store) {
      unsigned int nz = 0;
      HIPCHK(h, hipMemcpyAsync(&nz, h->head_ctr.p, sizeof(nz), hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
      if (dst_row0 == 0) h->head_nonempty = 0;
      h->head_nonempty += nz;
      h->last_batch_head_nonempty = nz;
    }
  }
  *n_out = kept_rows;
  *nnz_out = kept_nnz;
  return APSS_OK;
}

// ---- index build for rows [row0, idx_rows): rebuild every tile of `ix` that contains one of them (build_tiles, below) ----
// One build's state: what it covers and its plan (apss_build_plan.hpp), then what each stage settles for the ones behind it.
struct Build {
  apss_handle::IndexSet &ix;
  DevBuf<float> &tmin;         // shard rule (`scaled`: the probe scales its threshold per query and tile): min positive sub-norm per tile
  bool scaled;
  BuildPlan plan;              // (an Append sets the kind alone: its stages read nothing else of the plan)
  int64_t tile0, n_tiles, r0;  // tiles [tile0, n_tiles), from the rows [r0, b.row1)  (Append: the one tile, from the batch's first row)
  bool cuts_on_hand;           // Runs: the cuts k_ingest_plain left while it stored the rows are in this build's form and cover its rows
  BuildArgs b;
  BucketArgs bk;
  double appended_ms;          // time of the append that went before this build
  dim3 row_grid(int lanes) const { return dim3((unsigned)ceil_div((b.row1 - r0) * lanes, 256)); }  // `lanes` lanes per row, workgroups of 256
  dim3 tile_grid(int64_t per_tile) const { return dim3((unsigned)((n_tiles - tile0) * per_tile)); }  // `per_tile` workgroups per tile
};

// the kernels' view of the build of tiles [bd.tile0, bd.n_tiles) from the rows [row0, row1)
void fill_build_args(apss_handle *h, Build &bd, int64_t row0, int64_t row1) {
  apss_handle::IndexSet &ix = bd.ix;
  BuildArgs &b = bd.b = BuildArgs{};
  // (a handle with a dense-head block builds from its tail view: the block's entries are not in the inverted index)
  b.rowptr = h->head_k ? h->tv.rowptr.p : h->rowptr.p;
  b.idx = h->head_k ? h->tv.idx.p : h->idx.p;
  b.val = h->head_k ? h->tv.val.p : h->val.p;
  b.row0 = bd.r0 = row0;
  b.row1 = row1;
  b.cb = (int32_t)ix.cb;
  b.dim = h->cfg.dim;
  b.tile_seg = ix.seg.p;
  b.seg_stride = (int64_t)h->cfg.dim;
  b.coarse = ix.coarse ? 1 : 0;
  b.seg_align = ix.align;
  b.erow = h->head_k ? h->tv.erow.p : h->erow.p;
  b.row_scale = bd.scaled && ix.coarse ? h->sub.p : nullptr;  // shard rule: postings normalised by |x_g| / |x| (k_probe_coarse)
  b.coarse_shift = ix.coarse && ix.cb <= 32768 ? 1 : 0;  // must agree with k_probe_coarse's SLOT2 (the 512-thread kernels)
  b.coarse_wide = ix.coarse && ix.cb > 65536 ? 1 : 0;     // ... and with its WIDE (131072-row tiles)
  b.tile_post_base = ix.base.p;
  b.post = ix.post.p;
  b.post_c = ix.post_c.p;
  b.term_lo = h->cfg.term_lo;
  b.term_hi = h->cfg.term_hi;
}

// The plan, the reservations and the clears of maxlen / chunkw of a build of whole tiles; the build's clock starts at its end.
int32_t begin_build(apss_handle *h, Build &bd) {
  apss_handle::IndexSet &ix = bd.ix;
  BuildArgs &b = bd.b;
  const int64_t cb = ix.cb, stride = (int64_t)h->cfg.dim, tile0 = bd.tile0, n_tiles = bd.n_tiles, r0 = tile0 * cb;
  APSS_TRY(ensure(h, ix.seg, (size_t)(n_tiles * stride), (size_t)(tile0 * stride)));
  APSS_TRY(ensure(h, ix.base, (size_t)n_tiles + 1, (size_t)tile0 + 1));
  APSS_TRY(ensure(h, ix.total, (size_t)n_tiles, 0));
  APSS_TRY(ensure(h, ix.maxlen, 2));
  APSS_TRY(ensure(h, ix.chunkw, 1));
  if (tile0 == 0) {
    HIPCHK(h, hipMemsetAsync(ix.maxlen.p, 0, 2 * sizeof(uint32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(ix.chunkw.p, 0, sizeof(unsigned long long), h->stream));
  }
  if (bd.scaled) APSS_TRY(ensure(h, bd.tmin, (size_t)n_tiles, (size_t)tile0));
  const int64_t build_nnz = h->head_k ? h->tv.nnz : h->nnz;  // entries of the rows [0, idx_rows) the index is built from
  const BuildShape shape{h->cfg.dim, h->cfg.term_lo, h->cfg.term_hi, cb, ix.coarse, tile0, n_tiles, h->idx_rows, build_nnz, h->store_max_nnz};
  const BuildPlan &p = bd.plan = build_plan(shape, h->dbgcfg.build);
  const bool runs = p.kind == BuildKind::Runs;
  if (p.kind == BuildKind::Atomic)  // (the LDS kernels write every length of their range)
    HIPCHK(h, hipMemsetAsync(ix.seg.p + tile0 * stride, 0, (size_t)((n_tiles - tile0) * stride) * sizeof(uint2), h->stream));
  fill_build_args(h, bd, r0, h->idx_rows);
  if (h->dbgcfg.build_trace) fputs(build_trace_text(shape, p).c_str(), stderr);
  bd.cuts_on_hand = runs && !h->head_k && h->cut_cb == (int32_t)cb && h->cut_rt == p.range_terms && h->cut_ranges == p.n_ranges &&
                    h->cut_lo <= r0 && h->cut_hi >= h->idx_rows && h->cut_hi > h->cut_lo;
  if (h->dbgcfg.diag && runs)
    fprintf(stderr, "[apss diag] build %s rows [%lld, %lld): cuts %s\n", ix.coarse ? "coarse" : "exact", (long long)r0, (long long)h->idx_rows,
            bd.cuts_on_hand ? "reused" : "computed");
  if (runs) {
    if (!bd.cuts_on_hand) APSS_TRY(ensure(h, h->run_cut, (size_t)((h->idx_rows - r0) * (p.n_ranges + 1))));
    b.range_terms = p.range_terms;
    b.run_cut = bd.cuts_on_hand ? h->ing_cut.p + r0 * (p.n_ranges + 1) : h->run_cut.p;
  }
  if (runs && p.run_sub) {  // its scatter in two passes: the entries partitioned by (tile, sub-range)
    APSS_TRY(ensure(h, h->bk_cnt, (size_t)((n_tiles - tile0) * p.n_sub) + 2));
    APSS_TRY(ensure(h, h->bk_base, (size_t)((n_tiles - tile0) * p.n_sub) + 2));
    APSS_TRY(ensure(h, h->run_ent, (size_t)build_nnz));
    while ((1 << b.sub_shift) < p.run_sub) ++b.sub_shift;
    b.n_sub = p.n_sub;
    b.sub_cnt = h->bk_cnt.p;
    b.sub_base = h->bk_base.p;
    b.o_ent = h->run_ent.p;
  }
  HIPCHK(h, h->ev0.record(h->stream));
  if (p.kind != BuildKind::Bucketed) return APSS_OK;
  // Bucketed: the scratch of the largest tile group (row extents are on the device: one small read), k_bucket_pass's arguments, the LDS kernels' view
  const int64_t nb = p.group_tiles * p.n_ranges;
  std::vector<int64_t> grp_e((size_t)ceil_div(n_tiles, p.group_tiles) + 1);  // entries before each group, and before the end
  for (size_t i = 0; i < grp_e.size(); ++i)
    HIPCHK(h, hipMemcpyAsync(&grp_e[i], b.rowptr + std::min<int64_t>(h->idx_rows, (int64_t)i * p.group_tiles * cb), sizeof(int64_t),
                             hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  int64_t max_e = 1;
  for (size_t i = 0; i + 1 < grp_e.size(); ++i) max_e = std::max(max_e, grp_e[i + 1] - grp_e[i]);
  APSS_TRY(ensure(h, h->bk_cnt, (size_t)(2 * nb + 2)));
  APSS_TRY(ensure(h, h->bk_base, (size_t)nb + 2));
  APSS_TRY(ensure(h, h->bk_idx, (size_t)max_e));
  APSS_TRY(ensure(h, h->bk_erow, (size_t)max_e));
  APSS_TRY(ensure(h, h->bk_val, (size_t)max_e));
  // (rowptr, idx, val, erow, row1, cb, n_ranges, range_terms, tile0, bucket_cnt, bucket_base, bucket_cur, o_idx, o_erow, o_val)
  bd.bk = BucketArgs{b.rowptr, b.idx, b.val, b.erow, h->idx_rows, (int32_t)cb, p.n_ranges, p.range_terms, 0, h->bk_cnt.p, h->bk_base.p,
                     h->bk_cnt.p + nb + 1, h->bk_idx.p, h->bk_erow.p, h->bk_val.p};
  b.idx = h->bk_idx.p;
  b.erow = h->bk_erow.p;
  b.val = h->bk_val.p;
  b.ent_base = h->bk_base.p;
  b.range_terms = p.range_terms;
  HIPCHK(h, h->ev0.record(h->stream));  // (the build's clock starts behind the reservations)
  return APSS_OK;
}

template <int MODE>
void launch_tile_runs(apss_handle *h, const Build &bd) {  // k_tile_runs with the plan's lanes per row
  const int l = bd.plan.run_lanes;
  const auto k = l == 4 ? k_tile_runs<MODE, 4> : (l == 8 ? k_tile_runs<MODE, 8> : (l == 16 ? k_tile_runs<MODE, 16> : k_tile_runs<MODE, 32>));
  hipLaunchKernelGGL(k, bd.tile_grid(bd.plan.n_ranges), dim3(1024), (size_t)bd.plan.range_terms * sizeof(uint32_t), h->stream, bd.b, bd.tile0, bd.plan.n_ranges);
}

// One pass of a bucketed build, count or scatter, over its tile groups: partition a group's entries by term range into the scratch arrays
// (k_bucket_pass: count, scan, scatter), then the pass's LDS kernel over the buckets.  A single group is bucketed once, by the count pass, for
// both (its buckets are still there); several groups are bucketed again for the scatter pass (twice 43 ms at N = 10M, against 573 ms).
int32_t for_bucket_groups(apss_handle *h, Build &bd, bool scatter) {
  const BuildPlan &p = bd.plan;
  for (int64_t g0 = 0; g0 < bd.n_tiles; g0 += p.group_tiles) {
    const int64_t gt = std::min<int64_t>(p.group_tiles, bd.n_tiles - g0);
    const dim3 bgrid((unsigned)(gt * kBucketSlices)), grid((unsigned)(gt * p.n_ranges));
    if (!scatter || p.group_tiles < bd.n_tiles) {
      HIPCHK(h, hipMemsetAsync(h->bk_cnt.p, 0, (size_t)(2 * (p.group_tiles * p.n_ranges) + 2) * sizeof(unsigned long long), h->stream));
      bd.bk.tile0 = g0;
      hipLaunchKernelGGL(k_bucket_pass<false>, bgrid, dim3(1024), 0, h->stream, bd.bk);
      APSS_TRY(scan_i64(h, reinterpret_cast<const int64_t *>(h->bk_cnt.p), h->bk_base.p, gt * p.n_ranges));
      hipLaunchKernelGGL(k_bucket_pass<true>, bgrid, dim3(1024), 0, h->stream, bd.bk);
      HIPCHK(h, hipGetLastError());
    }
    hipLaunchKernelGGL(scatter ? k_tile_scatter_lds : k_tile_hist_lds, grid, dim3(1024), 0, h->stream, bd.b, g0, p.n_ranges);
  }
  return APSS_OK;
}

// segment lengths into tile_seg[..].y  (Append: on top of the kept lengths -- build_tiles has saved the old segment table and postings)
int32_t count_segments(apss_handle *h, Build &bd) {
  switch (bd.plan.kind) {
  case BuildKind::Append:
  case BuildKind::Atomic: hipLaunchKernelGGL(k_tile_hist, bd.row_grid(kWave), dim3(256), 0, h->stream, bd.b); break;
  case BuildKind::Stream: hipLaunchKernelGGL(k_tile_hist_lds, bd.tile_grid(bd.plan.n_ranges), dim3(1024), 0, h->stream, bd.b, bd.tile0, bd.plan.n_ranges); break;
  case BuildKind::Bucketed: APSS_TRY(for_bucket_groups(h, bd, false)); break;
  case BuildKind::Runs:
    if (!bd.cuts_on_hand) hipLaunchKernelGGL(k_row_cuts, bd.row_grid(kGroup), dim3(256), 0, h->stream, bd.b, bd.plan.n_ranges, h->run_cut.p);
    launch_tile_runs<kRunHist>(h, bd);
    if (bd.plan.run_sub) {
      APSS_TRY(scan_i64(h, reinterpret_cast<const int64_t *>(h->bk_cnt.p), h->bk_base.p, (bd.n_tiles - bd.tile0) * bd.plan.n_sub));
      launch_tile_runs<kRunPartition>(h, bd);
    }
  }
  return APSS_OK;  // (place_segments checks these launches with its own)
}

// lengths -> aligned segment starts and tile totals (the tile scan: k_tile_scan_part + k_tile_scan_place), the ONE read-back, tile bases by a
// host prefix sum (a handful of values), the posting array.  An append keeps what describes the rendering as a whole: chunkw, long_segs,
// round_chunks -- its scan keeps no lengths, weighs no chunks and counts no long segments.
int32_t place_segments(apss_handle *h, Build &bd) {
  apss_handle::IndexSet &ix = bd.ix;
  const bool app = bd.plan.kind == BuildKind::Append, keep_len = !app && bd.plan.kind != BuildKind::Atomic;
  const int64_t tile0 = bd.tile0, n = bd.n_tiles - tile0, dim = h->cfg.dim;
  const int32_t n_blk = (int32_t)ceil_div(dim, kScanBlock);
  APSS_TRY(ensure(h, ix.scan_part, (size_t)(n * n_blk)));
  hipLaunchKernelGGL(k_tile_scan_part, bd.tile_grid(n_blk), dim3(1024), 0, h->stream, (const uint2 *)ix.seg.p, dim, h->cfg.dim, tile0, n_blk,
                     (uint32_t)ix.align, ix.scan_part.p, ix.maxlen.p, tile0 == 0 && !app ? ix.chunkw.p : nullptr, app ? 0u : 1u);
  hipLaunchKernelGGL(k_tile_scan_place, bd.tile_grid(n_blk), dim3(1024), 0, h->stream, ix.seg.p, dim, h->cfg.dim, tile0, n_blk,
                     (uint32_t)ix.align, keep_len ? 1u : 0u, (const uint32_t *)ix.scan_part.p, ix.total.p);
  HIPCHK(h, hipGetLastError());
  std::vector<int64_t> tot((size_t)n);
  uint32_t seg_stats[2] = {0, 0};
  unsigned long long chunk_w = 0;
  HIPCHK(h, hipMemcpyAsync(tot.data(), ix.total.p + tile0, tot.size() * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(seg_stats, ix.maxlen.p, sizeof(seg_stats), hipMemcpyDeviceToHost, h->stream));
  if (!app) HIPCHK(h, hipMemcpyAsync(&chunk_w, ix.chunkw.p, sizeof(chunk_w), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  ix.max_seg = seg_stats[0];
  if (!app) ix.long_segs = seg_stats[1];
  // (measured on a build from the first tile; an appended batch keeps the figure of the build before it)
  if (!app && tile0 == 0 && h->idx_rows > 0) ix.round_chunks = (double)chunk_w / (double)h->idx_rows;
  ix.h_base.resize((size_t)tile0 + 1);  // bases of the tiles that stay (a first build: the 0 of tile 0)
  for (size_t i = 0; i < tot.size(); ++i) ix.h_base.push_back(ix.h_base.back() + tot[i]);
  const int64_t base = ix.h_base[(size_t)tile0];
  ix.post_used = ix.h_base.back();
  APSS_TRY(ix.coarse ? ensure(h, ix.post_c, (size_t)ix.post_used + 64, (size_t)base) : ensure(h, ix.post, (size_t)ix.post_used + 64, (size_t)base));
  if (ix.coarse)  // the probe reads a zero word as "no posting": clear the padding between segments
    HIPCHK(h, hipMemsetAsync(ix.post_c.p + base, 0, (size_t)(ix.post_used - base + 64) * sizeof(uint32_t), h->stream));
  const int64_t up0 = app ? tile0 + 1 : tile0;  // (the appended tile's own base stays)
  HIPCHK(h, hipMemcpyAsync(ix.base.p + up0, ix.h_base.data() + up0, (size_t)(bd.n_tiles + 1 - up0) * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  bd.b.tile_post_base = ix.base.p;  // (the posting array may have moved)
  bd.b.post = ix.post.p;
  bd.b.post_c = ix.post_c.p;
  return APSS_OK;
}

// the postings into their segments; the cursor increments rebuild tile_seg[..].y
int32_t scatter_postings(apss_handle *h, Build &bd) {
  apss_handle::IndexSet &ix = bd.ix;
  switch (bd.plan.kind) {
  case BuildKind::Append: {  // the tile's old postings move to their segments' new starts (k_tile_shift), the new ones go behind them
    const int64_t base = ix.h_base[(size_t)bd.tile0];
    const char *old = h->app_post.p;
    // (seg_old, seg_new, old_c, old_x, new_c, new_x, dim)
    const ShiftArgs sa{h->app_seg.p, ix.seg.p + bd.tile0 * (int64_t)h->cfg.dim, ix.coarse ? (const uint32_t *)old : nullptr, ix.coarse ? nullptr : (const Posting *)old,
                       ix.coarse ? ix.post_c.p + base : nullptr, ix.coarse ? nullptr : ix.post.p + base, h->cfg.dim};
    hipLaunchKernelGGL(k_tile_shift, dim3((unsigned)ceil_div((int64_t)h->cfg.dim * kGroup, 256)), dim3(256), 0, h->stream, sa);
  }
    [[fallthrough]];
  case BuildKind::Atomic: hipLaunchKernelGGL(k_tile_scatter, bd.row_grid(kWave), dim3(256), 0, h->stream, bd.b); break;
  case BuildKind::Stream: hipLaunchKernelGGL(k_tile_scatter_lds, bd.tile_grid(bd.plan.n_ranges), dim3(1024), 0, h->stream, bd.b, bd.tile0, bd.plan.n_ranges); break;
  case BuildKind::Bucketed: APSS_TRY(for_bucket_groups(h, bd, true)); break;
  case BuildKind::Runs:  // (two passes: the partitioned entries, sub-range by sub-range)
    if (bd.plan.run_sub) hipLaunchKernelGGL(k_tile_place_sub, bd.tile_grid(bd.plan.n_sub), dim3(kPlaceBlock), 0, h->stream, bd.b, bd.tile0);
    else launch_tile_runs<kRunScatter>(h, bd);
  }
  return APSS_OK;
}

int32_t finish_build(apss_handle *h, Build &bd) {
  if (bd.scaled)
    hipLaunchKernelGGL(k_tile_min_sub, bd.tile_grid(1), dim3(1024), 0, h->stream, (const float *)h->sub.p, h->idx_rows, (int32_t)bd.ix.cb, bd.tmin.p, bd.tile0);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, h->ev1.record(h->stream));
  HIPCHK(h, hipEventSynchronize(h->ev1));  // (the host vector the tile bases were copied from lives on; the event gives the build its time)
  float ms = 0.f;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  bd.ix.build_ms = ms + bd.appended_ms;
  return APSS_OK;
}

int32_t build_tiles(apss_handle *h, apss_handle::IndexSet &ix, int64_t row0) {
  const int64_t cb = ix.cb, n_tiles = ceil_div(h->idx_rows, cb);
  Build bd{ix, ix.coarse ? h->tile_min_c : h->tile_min, h->sharded || h->head_k > 0};
  int64_t &tile0 = bd.tile0 = row0 / cb;
  const auto stages = [&]() -> int32_t {
    for (const auto stage : {count_segments, place_segments, scatter_postings, finish_build}) APSS_TRY(stage(h, bd));
    return APSS_OK;
  };
  if (row0 % cb != 0 && ix.built_rows == row0 && ix.n_tiles == tile0 + 1 && (int64_t)ix.h_base.size() == tile0 + 2 && !h->dbgcfg.no_append) {
    // the batch lands in the last, partly filled tile of an up-to-date rendering: the stages over that tile as an Append, the tiles beyond as ever
    const int64_t base = ix.h_base[(size_t)tile0];
    const size_t old_total = (size_t)(ix.h_base[(size_t)tile0 + 1] - base), elt = ix.coarse ? sizeof(uint32_t) : sizeof(Posting);
    if (bd.scaled) APSS_TRY(ensure(h, bd.tmin, (size_t)n_tiles, (size_t)tile0 + 1));
    APSS_TRY(ensure(h, ix.total, (size_t)n_tiles, (size_t)tile0 + 1));
    APSS_TRY(ensure(h, h->app_seg, (size_t)h->cfg.dim));
    APSS_TRY(ensure(h, h->app_post, std::max<size_t>(old_total, 1) * elt));
    bd.plan.kind = BuildKind::Append;
    bd.n_tiles = tile0 + 1;
    fill_build_args(h, bd, row0, std::min<int64_t>(h->idx_rows, (tile0 + 1) * cb));
    HIPCHK(h, h->ev0.record(h->stream));
    HIPCHK(h, hipMemcpyAsync(h->app_seg.p, ix.seg.p + tile0 * (int64_t)h->cfg.dim, (size_t)h->cfg.dim * sizeof(uint2), hipMemcpyDeviceToDevice, h->stream));
    if (old_total > 0)
      HIPCHK(h, hipMemcpyAsync(h->app_post.p, ix.coarse ? (const void *)(ix.post_c.p + base) : (const void *)(ix.post.p + base), old_total * elt,
                               hipMemcpyDeviceToDevice, h->stream));
    APSS_TRY(stages());
    bd.appended_ms = ix.build_ms;
    row0 = ++tile0 * cb;
    if (h->idx_rows <= row0) {
      ix.built_rows = h->idx_rows;
      return APSS_OK;
    }
  }
  ix.n_tiles = bd.n_tiles = n_tiles;
  ix.built_rows = h->idx_rows;
  if (n_tiles == tile0) return APSS_OK;
  APSS_TRY(begin_build(h, bd));
  return stages();
}

// Which renderings of the index a handle keeps: the coarse one (two-pass speed path) is built at insert time when the
// handle may use it; the exact one is built at insert time otherwise, or lazily by the first probe that needs it.
int32_t ensure_exact_index(apss_handle *h) {
  if (h->ex_built_rows < h->idx_rows || h->ex.n_tiles == 0) {
    APSS_TRY(build_tiles(h, h->ex, std::min(h->ex_built_rows, h->idx_rows)));
    h->ex_built_rows = h->idx_rows;
    h->st.build_ms += h->ex.build_ms;
  }
  return APSS_OK;
}

// rows per tile of the coarse rendering when the handle chooses them (no tile_rows, no cx_tile), for a store of `rows` rows of `nnz` entries
int32_t pick_cx_tile(const apss_handle *h, int64_t rows, int64_t nnz) {
  return pick_cx_tile(TileFacts{rows, nnz, h->store_max_nnz, h->store_max_norm2, h->sharded, h->head_k, h->head_longseg, h->nonneg, h->no_acc8,
                                h->cfg.theta, h->cfg.dim},
                      h->dbgcfg.filter);
}

// Will the index build that follows a plain store batch of n rows / nnz entries at row dst_row0 read runs (build_tiles), and in
// which form?  Decided before the batch's own summaries are known, so it is a forecast: build_tiles compares the form of the
// cuts on hand with the one it takes and computes its own when they differ.  (*rt and *n_ranges: the run form, on a true return only.)
bool ingest_wants_cuts(const apss_handle *h, int64_t dst_row0, int64_t n, int64_t nnz, int32_t *cb, int32_t *rt, int32_t *n_ranges) {
  if (h->head_k) return false;  // (the build reads the tail view, not the store)
  const int64_t rows = dst_row0 + n, entries = h->nnz + nnz;
  const apss_handle::IndexSet &ix = h->use_coarse ? h->cx : h->ex;
  *cb = ix.cb;
  if (h->use_coarse && ix.n_tiles == 0 && h->cfg.tile_rows == 0 && !h->dbgcfg.cx_tile)
    *cb = pick_cx_tile(h, rows, entries);
  if (*cb <= 0) return false;
  // build_tiles' own decision, for the tiles this batch is expected to (re)build and the store as it will be
  const BuildPlan plan = build_plan(BuildShape{h->cfg.dim, h->cfg.term_lo, h->cfg.term_hi, *cb, ix.coarse, std::min(h->idx_rows, dst_row0) / *cb,
                                               ceil_div(rows, *cb), rows, entries, h->store_max_nnz},
                                    h->dbgcfg.build);
  *rt = plan.range_terms;
  *n_ranges = plan.n_ranges;
  return plan.kind == BuildKind::Runs && plan.n_ranges <= 2 * kGroup - 1;  // (k_ingest_plain: two cut counts per lane)
}

// ---- dense-head block (apss_head.hpp) ----
constexpr int64_t kTailMaxRows = 1024;   // rows that may wait outside the tile index (scored pair by pair by k_tail_score; 4096 until the append build made folding them in cheap)
constexpr int64_t kTailMaxBatch = 64;    // a batch larger than this extends the index right away (256 until the append build)
constexpr int64_t kTailMaxPairs = 1 << 22;  // (queries x tail rows) a probe scores directly; beyond it the tail is folded in first
constexpr int32_t kHeadMaxTerms = kHeadBlock * (1 + kHeadMaxFold);   // 256 terms with a column each + 256 columns of kHeadMaxFold terms
// width of a W row holding n_terms head terms: one block of 64 | 128 | 256 columns, or 256 + a folded block of fold_w columns
inline int32_t head_width(int32_t n_terms, int32_t fold_w, int32_t exact = kHeadBlock, bool i8 = false) {
  // (INT8 rendering: a 64-column row would be 64 bytes, less than a 1-KiB DMA piece per wave and tile: 128 columns at least)
  return n_terms <= 64 ? (i8 ? 128 : 64) : (n_terms <= 128 ? 128 : (n_terms <= 256 ? 256 : exact + fold_w));
}
// column of the i-th head term (most frequent first): the first `exact` get a column each, the others fold into fold_w columns
inline int32_t head_column(int32_t i, int32_t fold_w, int32_t exact = kHeadBlock) { return i < exact ? i : exact + (i - exact) % fold_w; }
constexpr int64_t kHeadMinRows = 16384;  // below this a join is over before a GEMM pays for its set-up
constexpr double kHeadSparseRate = 8.0e11;  // posting visits / s of the sparse filter (measured, C3)
// seconds per (query, candidate) element of the head contraction, block width 64 / 128 / 256 (measured on random rows,
// profiles/r02_head_gemm.md: 1.65 PFLOP/s at 256; narrower blocks are bound by the epilogue's scan, not by the MFMAs)
constexpr double kHeadDenseCost[4] = {1.5e-13, 1.9e-13, 3.1e-13, 3.1e-13};  // (last: a head of more than 256 terms -- still ONE block of 256 columns)
// ... with the INT8 rendering (v_mfma_i32_32x32x32_i8, rows half as wide; round 4: C3-Zipf(1) at N = 1M 155 -> 88 ms, 1.75e-13 per
// element at 256 columns; a block of up to 64 terms takes 128 byte-wide columns)
constexpr double kHeadDenseCostI8[4] = {1.2e-13, 1.2e-13, 1.75e-13, 1.75e-13};
constexpr double kHeadFoldMaxRowTerms = 96.0;  // terms of the folded block a row may hold on average (chance pairs collide in m^2 / 256 columns)
constexpr double kHeadSurvivorCost = 2.5e-9;  // seconds per element the dense filter passes on (report + de-dup + exact re-score; measured in
                                              // round 3: 5.6e6 more survivors cost 5 ms, i.e. 0.9e-9 each; the sample's TRUE pairs count too)

// A plain handle decides for itself (choose_head) unless the block's terms were set through apss_set_head_terms; a term
// shard only ever takes the terms it was given -- the {H, T_1 .. T_T} partition of the shard rule must be the same on every
// shard of the join, so the caller that cut the term ranges names the block too.
inline bool head_allowed(const apss_handle *h) {
  return h->use_coarse && (!h->sharded || h->head_fixed) && (h->cfg.head_terms >= 0 || h->head_fixed) && h->cfg.theta > 0.0 &&
         !h->head_blocked && h->nonneg;
}
// the policy looks at the term distribution when the store has doubled since it last did (build_index)
bool head_policy_due(const apss_handle *h, int64_t n_rows) {
  return head_allowed(h) && !h->head_fixed && n_rows >= std::max<int64_t>(h->cfg.head_terms > 0 ? 1 : kHeadMinRows, 2 * h->head_eval_rows);
}

// Which rendering the block's rows take.  INT8 (rounded up: a sound filter for the non-negative weights a block needs anyway)
// for a single block of 128 | 256 columns; bf16 for the two-block experiment forms and on request (APSS_DEBUG=head_bf16).
inline bool head_wants_i8(const apss_handle *h) {
  return !h->dbgcfg.head_bf16 && !(h->dbgcfg.fold_w == 128 || h->dbgcfg.fold_w == 256);
}
// (re)decide the rendering for a block of width head_k whose FIRST row is about to be packed
int32_t head_setup_rendering(apss_handle *h) {
  h->head_i8 = h->head_k > 0 && h->head_k <= kHeadBlock && head_wants_i8(h);
  h->head_s = 0.f;
  APSS_TRY(ensure(h, h->head_ovf, 4));
  HIPCHK(h, hipMemsetAsync(h->head_ovf.p, 0, 4 * sizeof(unsigned int), h->stream));
  return APSS_OK;
}
// INT8 scale S (units per 1.0).  No element of a W row exceeds its row's norm (exact columns hold c_t |c| / |c_H| <= |c|, folded
// columns the L2 norm of their terms, scaled alike), so S = 127 / (the largest row norm) never overflows a byte.  A row with a
// larger norm than any before (un-normalised input, a stream) shrinks S for the WHOLE block -- one threshold serves every pair --
// and the `packed_bytes` of W packed so far are re-quantised in place (k_head_rescale: still upper bounds).
int32_t head_fit_scale(apss_handle *h, double norm2, unsigned char *W, int64_t packed_bytes) {
  if (!h->head_i8) return APSS_OK;
  const double need = 127.0 / (std::sqrt(std::max(norm2, 1e-30)) * 1.0005);
  if (h->head_s > 0.f && need >= (double)h->head_s) return APSS_OK;
  if (h->head_s > 0.f && packed_bytes > 0) {
    const double target = need / 1.25;  // (room for norms a quarter larger before the next pass over W)
    const uint32_t den = 65535u;
    const uint32_t num = (uint32_t)std::min<double>(den, std::ceil(target / (double)h->head_s * den));
    hipLaunchKernelGGL(k_head_rescale, dim3((unsigned)std::min<int64_t>(8192, ceil_div(packed_bytes, 16 * 256))), dim3(256), 0, h->stream, W,
                       packed_bytes / 16 * 16, num, den);
    HIPCHK(h, hipGetLastError());
    h->head_s = (float)target;
  } else {
    h->head_s = (float)need;
  }
  return APSS_OK;
}
inline void head_pack_rendering(const apss_handle *h, HeadPackArgs &p) {
  p.i8_scale = h->head_i8 ? h->head_s : 0.f;
  p.overflow = h->head_ovf.p;
}

// tail view of rows [row0, row1) of a CSR batch (absolute offsets), appended to `v` as its rows [dst_row0, ..)
int32_t build_tail_view(apss_handle *h, apss_handle::TailView &v, const int64_t *rowptr, const int32_t *idx, const float *val,
                        int64_t row0, int64_t row1, int64_t dst_row0, bool with_erow) {
  const int64_t n = row1 - row0;
  if (dst_row0 == 0) v.rows = v.nnz = v.max_nnz = v.nonempty = 0;
  v.last_nonempty = 0;
  APSS_TRY(ensure(h, v.rowptr, (size_t)(dst_row0 + n + 1), (size_t)(dst_row0 ? dst_row0 + 1 : 0)));
  if (dst_row0 == 0) HIPCHK(h, hipMemsetAsync(v.rowptr.p, 0, sizeof(int64_t), h->stream));
  if (n <= 0) return APSS_OK;
  APSS_TRY(ensure(h, h->tv_cnt, (size_t)n + 1));
  APSS_TRY(ensure(h, h->tv_off, (size_t)n + 1));
  APSS_TRY(ensure(h, h->tv_sum, 2));
  HIPCHK(h, hipMemsetAsync(h->tv_sum.p, 0, 2 * sizeof(unsigned int), h->stream));
  TailViewArgs a{};
  a.rowptr = rowptr;
  a.idx = idx;
  a.val = val;
  a.row0 = row0;
  a.row1 = row1;
  a.head_pos = h->head_pos.p;
  a.cnt = h->tv_cnt.p;
  a.summary = h->tv_sum.p;
  const unsigned blocks = (unsigned)ceil_div(n * kGroup, 256);
  hipLaunchKernelGGL(k_tailv_count, dim3(blocks), dim3(256), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  APSS_TRY(scan_i64(h, (const int64_t *)h->tv_cnt.p, h->tv_off.p, n));
  int64_t total = 0;
  unsigned int sum[2] = {0, 0};
  HIPCHK(h, hipMemcpyAsync(&total, h->tv_off.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(sum, h->tv_sum.p, sizeof(sum), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const int64_t nnz0 = v.nnz;
  APSS_TRY(ensure(h, v.idx, (size_t)std::max<int64_t>(nnz0 + total, 1), (size_t)nnz0));
  APSS_TRY(ensure(h, v.val, (size_t)std::max<int64_t>(nnz0 + total, 1), (size_t)nnz0));
  if (with_erow) APSS_TRY(ensure(h, v.erow, (size_t)std::max<int64_t>(nnz0 + total, 1), (size_t)nnz0));
  a.off = h->tv_off.p;
  a.dst_row0 = dst_row0;
  a.dst_nnz0 = nnz0;
  a.o_rowptr = v.rowptr.p;
  a.o_idx = v.idx.p;
  a.o_val = v.val.p;
  a.o_erow = with_erow ? v.erow.p : nullptr;
  hipLaunchKernelGGL(k_tailv_write, dim3(blocks), dim3(256), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  v.rows = dst_row0 + n;
  v.nnz = nnz0 + total;
  v.max_nnz = std::max<int64_t>(v.max_nnz, sum[0]);
  v.nonempty += sum[1];
  v.last_nonempty = sum[1];
  return APSS_OK;
}

// W rows, tail ratios and the masked term array for store rows [row0, n_rows)
int32_t head_pack_store(apss_handle *h, int64_t row0) {
  const int64_t kh = h->head_k;
  const int64_t rows_pad = ceil_div(h->idx_rows, kHeadQBlock) * kHeadQBlock + kHeadCTile;
  APSS_TRY(ensure(h, h->W, (size_t)(rows_pad * kh), (size_t)(ceil_div(row0, kHeadCTile) * kHeadCTile * kh)));  // (tiled: whole tiles)
  APSS_TRY(ensure(h, h->sub, (size_t)h->idx_rows, (size_t)row0));
  APSS_TRY(ensure(h, h->head_ctr, 4));
  HIPCHK(h, hipMemsetAsync(h->head_ctr.p, 0, 4 * sizeof(unsigned long long), h->stream));
  if (row0 == 0) APSS_TRY(head_setup_rendering(h));
  APSS_TRY(head_fit_scale(h, (double)h->store_max_norm2, reinterpret_cast<unsigned char *>(h->W.p), ceil_div(row0, kHeadCTile) * kHeadCTile * kh));
  {
    HeadPackArgs a{};
    head_pack_rendering(h, a);
    a.rowptr = h->rowptr.p;
    a.idx = h->idx.p;
    a.val = h->val.p;
    a.row0 = row0;
    a.row1 = h->idx_rows;
    a.head_pos = h->head_pos.p;
    a.kh = (int32_t)kh;
    a.W = h->W.p;
    a.w_row0 = row0;
    a.w_pad = rows_pad;  // the rows past the last one are zero rows: a GEMM tile or query block may read them
    a.ratio_t = h->sub.p;
    a.head_nonempty = reinterpret_cast<unsigned int *>(h->head_ctr.p);
    a.row_inv = nullptr;
    a.prune_above = -INFINITY;  // (the store holds the rows as they are scored)
    a.fold_from = h->head_exact;
    hipLaunchKernelGGL(k_head_pack, dim3((unsigned)(ceil_div(rows_pad, 8) - row0 / 8)), dim3(512), 0, h->stream, a);
  }
  HIPCHK(h, hipGetLastError());
  unsigned int nz = 0;
  HIPCHK(h, hipMemcpyAsync(&nz, h->head_ctr.p, sizeof(nz), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (row0 == 0) h->head_nonempty = 0;
  h->head_nonempty += nz;
  h->last_batch_head_nonempty = nz;
  return APSS_OK;
}

int32_t run_head(apss_handle *h, const ProbeArgs &a, int64_t nq, int64_t q_slot_base, const uint16_t *Wq, int64_t wq_rows,
                 float thr, double bound, int64_t n_cand);

// a query batch resident on the device: CSR rows (absolute offsets into idx / val) and their external ids
struct QueryRows {
  int64_t nq;
  const int64_t *rowptr;
  const int32_t *idx;
  const float *val;
  const int64_t *ext;
};

// ... as a query-type call hands it down: slot_first: slot of row 0 when the batch is rows of the store, else -1; max_nnz,
// max_norm2: the longest row and the largest squared row norm (of the whole batch, whatever rows of it are probed); nnz_end: the
// entries behind the offsets
struct QueryBatch : QueryRows {
  int64_t slot_first, max_nnz;
  float max_norm2;
  int64_t nnz_end;
  const int32_t *slots = nullptr;  // [nq] the slot of every row where the batch is a SELECTION of stored rows (apss_query_stored), else NULL
  bool absorb_only = false;        // the list is wanted by the components alone (a removal's re-join): no cut runs, nothing of it is kept
  // rows [r0, r1) as a batch of their own (a window): the offsets stay absolute
  QueryBatch rows(int64_t r0, int64_t r1) const {
    return QueryBatch{{r1 - r0, rowptr + r0, idx, val, ext + r0}, slot_first < 0 ? -1 : slot_first + r0, max_nnz, max_norm2, nnz_end,
                      slots ? slots + r0 : nullptr, absorb_only};
  }
};

// the last query-type call's results and batch are gone (they may point into arrays that are about to be rewritten or
// reallocated): apss_fetch_results / apss_partial_scores_dev answer APSS_E_STATE until the next query-type call
void forget_last_call(apss_handle *h) {
  h->n_res = -1;
  h->res_q_ext = nullptr;
  h->last_q_rowptr = nullptr;
  h->last_q_idx = nullptr;
  h->last_q_val = nullptr;
  h->last_nq = 0;
}

// the batch the handle's results speak of (apss_fetch_results looks its ids up, apss_partial_scores_dev reads its rows)
void name_last_batch(apss_handle *h, const QueryRows &q) {
  h->res_q_ext = q.ext;
  h->last_q_rowptr = q.rowptr;
  h->last_q_idx = q.idx;
  h->last_q_val = q.val;
  h->last_nq = q.nq;
}

// (q, c, s)[0, n) is the call's list from here on: the ONE writer of where the results live, how many there are, and the statistic
void adopt_list(apss_handle *h, const int32_t *q, const int32_t *c, const float *s, int64_t n) {
  h->out_q = q;
  h->out_c = c;
  h->out_s = s;
  h->n_res = n;
  h->st.result_pairs = n;
}
inline void adopt_list(apss_handle *h, const PairList &l, int64_t n) { adopt_list(h, l.q.p, l.c.p, l.s.p, n); }

// k_rescore's arguments: the pairs (cand_q, cand_c) of query rows and store slots are re-scored from the fp32 store, and those
// that reach theta go to h->fin, counted at out_count.  n_pairs_dev (chained launch): the pair count is read on the device
RescoreArgs rescore_args(const apss_handle *h, const int32_t *cand_q, const int32_t *cand_c, int64_t n_pairs, const unsigned long long *n_pairs_dev,
                         const QueryRows &q, float theta, unsigned long long *out_count) {
  RescoreArgs r{};
  r.n_pairs = n_pairs;
  r.n_pairs_dev = n_pairs_dev;
  r.q_row = cand_q;
  r.c_slot = cand_c;
  r.q_rowptr = q.rowptr;
  r.q_idx = q.idx;
  r.q_val = q.val;
  r.c_rowptr = h->rowptr.p;
  r.c_idx = h->idx.p;
  r.c_val = h->val.p;
  r.theta = theta;
  h->fin.as_out(r);
  r.out_count = out_count;
  return r;
}
inline dim3 rescore_grid(int64_t pairs) { return dim3((unsigned)std::max<int64_t>(1, ceil_div(pairs, (int64_t)kRescorePairs * kRescoreTrips))); }

// k_tail_score's arguments: every (query, waiting row) pair, exactly; appended to h->fin behind its first out_base pairs
TailArgs tail_args(const apss_handle *h, const QueryRows &q, int64_t tail_n, float theta, int64_t out_base, unsigned long long *counters) {
  TailArgs t{};
  t.nq = q.nq;
  t.n_tail = tail_n;
  t.q_rowptr = q.rowptr;
  t.q_idx = q.idx;
  t.q_val = q.val;
  t.q_ext = q.ext;
  t.c_rowptr = h->rowptr.p;
  t.c_idx = h->idx.p;
  t.c_val = h->val.p;
  t.c_ext = h->ext.p;
  t.tail0 = h->idx_rows;
  t.theta = theta;
  h->fin.as_out(t);
  t.out_base = out_base;
  t.counters = counters;
  return t;
}

// How selective is the dense filter on THIS data: the block's first rows (at most 8192) against its first 512 as queries,
// stored and re-scored.  Returns the fraction of (q, c != q) elements the filter passes that do NOT reach theta.  (Rows arrive in no
// particular order in the reference's stream -- ShardRegion routing is random, CommonUtils.scala:28-40 -- so a prefix is a
// sample.)
int32_t head_sample_selectivity(apss_handle *h, double *frac) {
  *frac = 0.0;
  const int64_t kh = h->head_k;
  const int64_t S = std::min<int64_t>(h->idx_rows, 8192), Q = std::min<int64_t>(S, 512);
  const int64_t rows_pad = ceil_div(h->idx_rows, kHeadQBlock) * kHeadQBlock + kHeadCTile;
  APSS_TRY(ensure(h, h->W, (size_t)(rows_pad * kh), 0));
  APSS_TRY(ensure(h, h->sub, (size_t)h->idx_rows, 0));
  APSS_TRY(ensure(h, h->head_ctr, 4));
  APSS_TRY(ensure(h, h->counters, kCtrCount));
  HIPCHK(h, hipMemsetAsync(h->head_ctr.p, 0, 4 * sizeof(unsigned long long), h->stream));
  APSS_TRY(head_setup_rendering(h));
  APSS_TRY(head_fit_scale(h, (double)h->store_max_norm2, nullptr, 0));
  HeadPackArgs p{};
  head_pack_rendering(h, p);
  p.rowptr = h->rowptr.p;
  p.idx = h->idx.p;
  p.val = h->val.p;
  p.row0 = 0;
  p.row1 = S;
  p.head_pos = h->head_pos.p;
  p.kh = (int32_t)kh;
  p.W = h->W.p;
  p.w_row0 = 0;
  p.w_pad = ceil_div(S, kHeadQBlock) * kHeadQBlock;
  p.ratio_t = h->sub.p;
  p.head_nonempty = nullptr;
  p.row_inv = nullptr;
  p.prune_above = -INFINITY;
  p.fold_from = h->head_exact;
  hipLaunchKernelGGL(k_head_pack, dim3((unsigned)ceil_div(p.w_pad, 8)), dim3(512), 0, h->stream, p);
  HIPCHK(h, hipGetLastError());
  // the sample's survivors are STORED and re-scored exactly: what counts against the block is what it passes in excess -- a
  // pair that reaches theta is a survivor of every filter (the sample of a batch with planted near-duplicates holds 3e-5 of
  // them: counted against the block they vetoed a head that halves the step of C3 with Zipf(0.5) terms)
  constexpr size_t kSampleCap = 1 << 20;
  APSS_TRY(h->res.ensure(h, kSampleCap));
  ProbeArgs a{};
  a.q_ext = h->ext.p;
  h->res.as_candidates(a);
  a.res_cap = kSampleCap;
  a.counters = h->head_ctr.p + 2;
  const double bound = (double)h->store_max_norm2 * 1.0001 + 1e-6;  // |q||c| <= the largest squared row norm
  APSS_TRY(run_head(h, a, Q, -1, h->W.p, p.w_pad, (float)(h->cfg.theta - 0.0080 * bound - 1e-5), bound, S));
  unsigned long long c[4];
  HIPCHK(h, hipMemcpyAsync(c, h->head_ctr.p, sizeof(c), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const double pairs = (double)Q * (double)S - (double)Q;
  unsigned long long n_true = 0;
  if (c[2] > 0 && c[2] <= kSampleCap) {
    APSS_TRY(h->fin.ensure(h, (size_t)c[2]));
    HIPCHK(h, hipMemsetAsync(h->head_ctr.p, 0, sizeof(unsigned long long), h->stream));
    // (the sample's queries are the store's first rows)
    const RescoreArgs r = rescore_args(h, h->res.q.p, h->res.c.p, (int64_t)c[2], nullptr, QueryRows{S, h->rowptr.p, h->idx.p, h->val.p, h->ext.p}, (float)h->cfg.theta, h->head_ctr.p);
    hipLaunchKernelGGL(k_rescore, rescore_grid(r.n_pairs), dim3(kRescoreBlock), 0, h->stream, r);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(&n_true, h->head_ctr.p, sizeof(n_true), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  *frac = pairs > 0 ? (double)(c[2] - std::min(n_true, c[2])) / pairs : 0.0;
  return APSS_OK;
}

// Look at the store's term distribution (sampled document frequencies) and decide which terms, if any, go to the
// dense block: term t costs df_t^2 posting visits in the inverted index and 2 * N^2 flop as a column of the
// contraction (half of that for a stored batch: the product is symmetric).  *changed: the block's term set differs.
int32_t choose_head(apss_handle *h, bool *changed) {
  *changed = false;
  const int64_t n = h->n_rows;
  const int32_t dim = h->cfg.dim;
  h->head_eval_rows = n;
  const int64_t stride = std::max<int64_t>(1, n / 65536);
  const int64_t sampled = ceil_div(n, stride);
  std::vector<uint32_t> df;
  // the sample k_ingest_plain took while it stored these very rows, or one taken now
  const bool delivered = h->df_rows == n && h->df_stride == stride && h->df_host.size() == (size_t)dim;
  if (delivered) {
    df.swap(h->df_host);
  } else {
    APSS_TRY(ensure(h, h->df, (size_t)dim));
    HIPCHK(h, hipMemsetAsync(h->df.p, 0, (size_t)dim * sizeof(uint32_t), h->stream));
    hipLaunchKernelGGL(k_df_sample, dim3((unsigned)ceil_div(sampled * kWave, 256)), dim3(256), 0, h->stream,
                       (const int64_t *)h->rowptr.p, (const int32_t *)h->idx.p, n, stride, h->df.p);
    HIPCHK(h, hipGetLastError());
    df.resize((size_t)dim);
    HIPCHK(h, hipMemcpyAsync(df.data(), h->df.p, (size_t)dim * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  h->df_rows = -1;
  if (h->dbgcfg.diag) fprintf(stderr, "[apss diag] head policy: df sample of %lld rows %s\n", (long long)n, delivered ? "reused" : "computed");
  std::vector<int32_t> order((size_t)dim);
  for (int32_t t = 0; t < dim; ++t) order[(size_t)t] = t;
  const size_t top = (size_t)std::min<int32_t>(dim, kHeadMaxTerms);
  const auto more_frequent = [&](int32_t x, int32_t y) { return df[(size_t)x] != df[(size_t)y] ? df[(size_t)x] > df[(size_t)y] : x < y; };
  bool hopeless = false;
  if (h->cfg.head_terms == 0) {
    // before sorting anything: no head of kHeadMaxTerms terms can save more visits than min(all terms', that many of the most
    // frequent one's) -- on uniform data (C3: every benchmark step re-evaluates after its apss_clear) that is below the
    // cheapest block's cost and the 3 ms of sorting 100k terms are not spent
    double s2_all = 0.0, f_max = 0.0;
    for (int32_t t = 0; t < dim; ++t) {
      const double f = (double)df[(size_t)t] / (double)sampled;
      s2_all += f * f;
      f_max = std::max(f_max, f);
    }
    // (per block size: k terms save at most min(all terms', k x the most frequent one's) visits against THAT block's cost -- a
    // single comparison with the cheapest block's cost stopped holding on C3 when the INT8 rendering made that block cheaper)
    const double *cost = head_wants_i8(h) ? kHeadDenseCostI8 : kHeadDenseCost;
    const double terms_of[4] = {64.0, 128.0, 256.0, (double)top};
    hopeless = true;
    for (int ki = 0; ki < 4; ++ki)
      if (std::min(s2_all, terms_of[ki] * f_max * f_max) / kHeadSparseRate >= 1.5 * 0.5 * cost[ki]) hopeless = false;
  }
  if (!hopeless) {
    std::nth_element(order.begin(), order.begin() + (ptrdiff_t)top - 1, order.end(), more_frequent);
    std::sort(order.begin(), order.begin() + (ptrdiff_t)top, more_frequent);
  }
  int32_t k = 0;
  double best_gain = 0.0;  // seconds per N^2 pairs the chosen block is expected to save
  double gain256 = 0.0;    // ... and a plain 256-term block, the fall-back when the folded block proves unselective
  if (h->cfg.head_terms > 0) {
    k = std::min(h->cfg.head_terms <= 256 ? head_width(h->cfg.head_terms, 0) : h->cfg.head_terms, kHeadMaxTerms);  // terms wanted
  } else if (n >= kHeadMinRows && !hopeless) {
    double best = 0.0, s2 = 0.0;
    size_t i = 0;
    int ki = 0;
    double m_fold = 0.0;  // average number of folded-block terms per row
    for (int32_t kk : {64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768}) {
      if (kk > kHeadMaxTerms || (size_t)kk > top + 255) break;
      for (; i < std::min<size_t>(top, (size_t)kk); ++i) {
        const double f = (double)df[(size_t)order[i]] / (double)sampled;
        s2 += f * f;
        if (i >= (size_t)h->head_exact) m_fold += f;
      }
      if (m_fold > kHeadFoldMaxRowTerms) break;
      // per N^2 pairs of a stored batch: df_t^2 = f_t^2 N^2 visits saved; half of the product computed (symmetric).  A head
      // of more than 256 terms costs ONE more contraction however many terms fold into it
      const double save = s2 / kHeadSparseRate, cost = 0.5 * (head_wants_i8(h) ? kHeadDenseCostI8 : kHeadDenseCost)[std::min(ki++, 3)];
      if (save >= 1.5 * cost && kk == kHeadBlock) gain256 = save - cost;
      if (save >= 1.5 * cost && save - cost > best) {
        best = save - cost;
        k = kk;
      }
    }
    best_gain = best;
  }
  if (std::min(k, kHeadBlock) > dim) k = 0;
  std::vector<int32_t> terms;
  for (size_t i = 0; i < std::min<size_t>(top, (size_t)k); ++i)
    if (df[(size_t)order[i]] > 0) terms.push_back(order[i]);
  const int32_t old_k = h->head_k;
  const std::vector<int32_t> old_terms = h->head_terms;
  auto upload_columns = [&]() -> int32_t {
    std::vector<int32_t> pos((size_t)dim, -1);
    for (size_t i = 0; i < h->head_terms.size(); ++i) pos[(size_t)h->head_terms[i]] = head_column((int32_t)i, h->head_fold_w, h->head_exact);
    APSS_TRY(ensure(h, h->head_pos, (size_t)dim));
    HIPCHK(h, hipMemcpyAsync(h->head_pos.p, pos.data(), (size_t)dim * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));  // `pos` goes out of scope
    return APSS_OK;
  };
  for (;;) {
    k = terms.empty() ? 0 : head_width((int32_t)terms.size(), h->head_fold_w, h->head_exact, head_wants_i8(h));  // from here on: the width of a W row
    const bool differs = k != old_k || terms != old_terms;
    h->head_k = k;
    h->head_terms = terms;
    if (k && differs) APSS_TRY(upload_columns());
    if (!(k && differs && h->cfg.head_terms == 0)) break;  // (a block that is already in use has passed the test below)
    // the visit count says yes; now the other side of the ledger: every element the dense filter passes is reported,
    // de-duplicated and re-scored (measured: ~10 ns each).  At a low threshold on strongly skewed data that can be a
    // fraction of a percent of N^2 -- more than the posting visits saved (C2: theta = 0.5).  Measure it on a sample.
    double frac = 0.0;
    APSS_TRY(head_sample_selectivity(h, &frac));
    h->head_sample_frac = frac;
    if (frac * kHeadSurvivorCost <= 0.5 * best_gain) break;
    if (terms.size() > (size_t)kHeadBlock && gain256 > 0.0) {  // the folded block passes too much here: try the 256 terms alone
      terms.resize((size_t)kHeadBlock);
      best_gain = gain256;
      continue;
    }
    h->head_k = 0;
    h->head_terms.clear();
    break;
  }
  *changed = h->head_k != old_k || h->head_terms != old_terms;
  return APSS_OK;
}

int32_t build_index(apss_handle *h, int64_t row0) {
  h->st.build_ms = 0;
  row0 = std::min(row0, h->idx_rows);  // rows waiting in the tail are folded in with this batch
  h->idx_rows = h->n_rows;
  if (head_allowed(h)) {
    if (head_policy_due(h, h->n_rows)) {
      bool changed = false;
      APSS_TRY(choose_head(h, &changed));
      if (changed) {  // every tile's posting lists change with the term set: rebuild from the first row
        row0 = 0;
        h->cx.n_tiles = 0;
        h->ex_built_rows = 0;
      }
    }
    if (h->head_k) {
      h->cx.cb = std::min(h->cx.cb, 65536);  // the sparse half runs a 512-thread shard-rule kernel
      if (!h->sharded) APSS_TRY(head_pack_store(h, row0));  // (a term shard's W and ratios: ingest, from the caller's whole rows)
      const int64_t tv0 = row0 == h->tv.rows ? row0 : 0;  // (append, or start over when the view is not exactly the rows before)
      APSS_TRY(build_tail_view(h, h->tv, h->rowptr.p, h->idx.p, h->val.p, tv0, h->idx_rows, tv0, true));
    }
  } else if (h->head_k && h->sharded) {
    // a shard cannot leave the partition its peers were given: the block's terms are in no shard's index
    return fail(h, APSS_E_UNSUPPORTED, "a term shard with a dense-head block needs non-negative weights (apss_set_head_terms)");
  } else if (h->head_k) {  // e.g. a negative weight arrived: back to the plain index
    h->downgrades |= APSS_DOWNGRADE_HEAD;
    h->head_k = 0;
    h->head_terms.clear();
    row0 = 0;
    h->cx.n_tiles = 0;
    h->ex_built_rows = 0;
  }
  if (h->use_coarse) {
    if (h->cx.n_tiles == 0 && h->cfg.tile_rows == 0 && !h->dbgcfg.cx_tile && h->idx_rows > 0) {
      h->cx.cb = pick_cx_tile(h, h->n_rows, h->nnz);
    }
    APSS_TRY(build_tiles(h, h->cx, row0));
    h->st.build_ms += h->cx.build_ms;
    if (h->head_k && h->cfg.tile_rows == 0 && !h->dbgcfg.cx_tile) {
      if (h->cx.cb > 32768 && h->cx.max_seg > (uint32_t)kLongLenW) {
        h->head_longseg = true;
        h->cx.cb = 32768;
        h->cx.n_tiles = 0;
        APSS_TRY(build_tiles(h, h->cx, 0));
        h->st.build_ms += h->cx.build_ms;
      } else if (h->cx.cb <= 32768 && h->head_longseg && row0 == 0 && 2 * h->cx.max_seg <= (uint32_t)kLongLenW) {
        h->head_longseg = false;  // (this data would have fitted: the next first build tries the wide tiles again)
      }
    }
    h->ex_built_rows = std::min(h->ex_built_rows, row0 / h->ex.cb * h->ex.cb);  // exact tiles from here on are stale
  } else {
    h->ex_built_rows = std::min(h->ex_built_rows, row0);
    APSS_TRY(ensure_exact_index(h));
  }
  h->n_tiles = ceil_div(h->idx_rows, h->ex.cb);
  return APSS_OK;
}

// An instantiation of a probe kernel (every one takes ProbeArgs as its one argument): its address and its workgroup size.
// Enough to ask for its occupancy, to set its attributes and to launch it; fn == null: no such instantiation
struct KernelRef {
  const void *fn;
  int block;
};
template <class F>
const void *kernel_addr(F *f) { return reinterpret_cast<const void *>(f); }

int32_t launch_ref(apss_handle *h, const KernelRef &k, dim3 grid, size_t lds, const ProbeArgs &a) {
  void *args[] = {const_cast<ProbeArgs *>(&a)};
  (void)hipLaunchKernel(k.fn, grid, dim3(k.block), args, lds, h->stream);
  HIPCHK(h, hipGetLastError());
  return APSS_OK;
}

// the general kernel k_probe<MODE, BLOCK, FX, CUT>: theta > 0 with 1024 threads; theta <= 0 with either block, with or without
// the per-round cut
template <int MODE, int BLOCK, bool CUT>
KernelRef gen_ref(bool fx) { return {fx ? kernel_addr(&k_probe<MODE, BLOCK, true, CUT>) : kernel_addr(&k_probe<MODE, BLOCK, false, CUT>), BLOCK}; }
KernelRef gen_kernel(int mode, int block, bool fx, bool cut) {
  if (mode == 0 && block == kProbeBlock && !cut) return gen_ref<0, kProbeBlock, false>(fx);
  if (mode == 1 && block == kProbeBlock && !cut) return gen_ref<1, kProbeBlock, false>(fx);
  if (mode == 2 && block == kProbeBlock) return cut ? gen_ref<2, kProbeBlock, true>(fx) : gen_ref<2, kProbeBlock, false>(fx);
  if (mode == 2 && block == 512) return cut ? gen_ref<2, 512, true>(fx) : gen_ref<2, 512, false>(fx);
  return {nullptr, 0};
}
// the single-pass exact kernel k_probe_wave: shapes A (8 waves x 64-chunk window) and C (8 waves x 40-chunk window)
template <int U, int LC, int SC>
KernelRef wave_ref(bool sharded, bool diag) {
  if (sharded) return {diag ? kernel_addr(&k_probe_wave<512, U, LC, SC, true, true>) : kernel_addr(&k_probe_wave<512, U, LC, SC, true, false>), 512};
  return {diag ? kernel_addr(&k_probe_wave<512, U, LC, SC, false, true>) : kernel_addr(&k_probe_wave<512, U, LC, SC, false, false>), 512};
}
KernelRef wave_kernel(char variant, bool sharded, bool diag) {
  return variant == 'A' ? wave_ref<8, 256, 1024>(sharded, diag) : wave_ref<5, 128, 512>(sharded, diag);
}
// k_probe / k_probe_wave keep their LDS in a dynamic array: one workgroup per (tile, chunk) cell
int32_t launch_exact(apss_handle *h, const KernelRef &k, const ProbeArgs &a, size_t lds) {
  if (!k.fn) return fail(h, APSS_E_UNSUPPORTED, "no probe kernel for this combination of options");
  HIPCHK(h, hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return launch_ref(h, k, dim3((unsigned)((int64_t)a.n_tiles * a.n_chunks)), lds, a);
}
// theta <= 0 (every touched candidate is an answer): the round is a chain of barriers and latencies (SQ counters, round 4:
// 73 % of the wave-cycles waiting, LDS issue 0.39, VALU 0.34), and the 1024-thread workgroup over a 16384-row tile holds 93 KB
// of LDS: ONE workgroup per CU.  512 threads over tiles of <= 8192 rows hold 58 KB: two per CU
inline int gen_block(int mode, int cb) { return mode == 2 && cb <= 8192 ? 512 : kProbeBlock; }

// ---- the filter kernel's instantiations, in the order of the tables' walk (filter_variant_index, apss_filter_plan.hpp):
// THE lookup of a variant's instantiation (fn == null: not listed)
KernelRef cx_kernel(const CxVariant &v) {
  static const KernelRef refs[] = {
#define X(U) {kernel_addr(&k_probe_planes<U>), 512},
      APSS_EVEN_PLANES_VARIANTS(X)
#undef X
#define X(U, A8) {kernel_addr(&k_probe_even_merged<U, A8>), 512},
      APSS_EVEN_MERGE_VARIANTS(X)
#undef X
#define X(B, U, SH, SG, A8) {kernel_addr(&k_probe_even<B, U, (B <= 512 ? 128 : 256), SH, SG, A8>), B},
      APSS_EVEN_VARIANTS(X)
#undef X
#define X(B, U, SH, CH, VR, SG, LP, A8) \
  {kernel_addr(&k_probe_coarse<B, U, (B <= 512 ? 128 : 256), (B <= 512 ? 512 : 1024), SH, CH, VR, SG, LP, A8>), B},
      APSS_CX_VARIANTS(X)
#undef X
  };
  const int i = filter_variant_index(v);
  return i < 0 ? KernelRef{nullptr, 0} : refs[i];
}

// workgroups of a k_probe_even instantiation that the chip holds at a time: the occupancy query (the kernels' LDS is static,
// so the query sees it: two per CU for the 512-thread ones, one for the 1024-thread ones) x the CUs; asked once per instantiation
int32_t even_resident_slots(apss_handle *h, const CxVariant &v, int *slots) {
  const void *kern = v.even ? cx_kernel(v).fn : nullptr;
  if (!kern) return fail(h, APSS_E_UNSUPPORTED, "no filter kernel for this combination of options");
  if (h->n_cus == 0) HIPCHK(h, hipDeviceGetAttribute(&h->n_cus, hipDeviceAttributeMultiprocessorCount, h->dev));
  auto it = h->wl_per_cu.find(kern);
  if (it == h->wl_per_cu.end()) {
    int per_cu = 0;
    HIPCHK(h, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, v.block, 0));
    it = h->wl_per_cu.emplace(kern, std::max(per_cu, 1)).first;
  }
  *slots = it->second * h->n_cus;
  return APSS_OK;
}

// persist_wgs > 0 (k_probe_even only): a.items holds the launch's work list and that many workgroups take its items
// (the filter kernels keep their LDS in static arrays: no dynamic bytes)
int32_t launch_cx(apss_handle *h, const CxVariant &v, const ProbeArgs &a, int64_t persist_wgs = 0) {
  const KernelRef k = cx_kernel(v);
  if (!k.fn) return fail(h, APSS_E_UNSUPPORTED, "no filter kernel for this combination of options");
  const dim3 grid((unsigned)(persist_wgs > 0 ? persist_wgs : (int64_t)a.n_tiles * a.n_chunks));
  return launch_ref(h, k, grid, 0, a);
}

// ---- dense-head filter of one query batch (apss_head.hpp): appends its candidates to the sparse filter's list ----
int32_t run_head(apss_handle *h, const ProbeArgs &a, int64_t nq, int64_t q_slot_base, const uint16_t *Wq, int64_t wq_rows,
                 float thr, double bound, int64_t n_cand) {
  // INT8 rendering: integer products, int32 sums -- the only slack is the fp32 arithmetic that made the rows (k_head_pack)
  const bool i8 = h->head_i8;
  const double s2 = (double)h->head_s * (double)h->head_s;
  const int32_t thr_i = i8 ? (int32_t)std::max(1.0, std::floor(s2 * (h->cfg.theta - 2e-5 * (1.0 + bound)))) : 0;
  const float inv_s2 = i8 ? (float)(1.0 / s2) : 0.f;
  const int kt = h->head_k;                        // width of a W row
  const int kh = std::min(kt, kHeadBlock);        // width of the first block
  const int n_blocks = kt > kHeadBlock ? 2 : 1;
  const int fold_w = kt - kHeadBlock;             // width of the folded block (128 | 256) when there is one
  if (nq <= 2 * kGemvQ) {
    HeadGemvArgs g{};
    g.Wq = Wq;
    g.Wc = h->W.p;
    g.n_rows = n_cand;
    g.q_slot_base = q_slot_base;
    g.nq = (int32_t)nq;
    g.kh = kh;
    g.kt = kt;
    g.part = h->head_part;
    g.n_parts = h->head_parts;
    g.q_ext = a.q_ext;
    g.c_ext = h->ext.p;
    g.thr = i8 ? (float)thr_i : thr;
    g.i8 = i8 ? 1 : 0;
    g.inv_s2 = inv_s2;
    g.res_q = a.res_q;
    g.res_c = a.res_c;
    g.res_s = a.res_s;
    g.res_cap = a.res_cap;
    g.counters = a.counters;
    g.head_pairs = h->head_ctr.p + 1;
    const int64_t blocks = std::min<int64_t>(2048, std::max<int64_t>(1, ceil_div(n_cand, 256 * (int64_t)h->head_parts)));
    for (int b = 0; b < n_blocks; ++b) {
      g.chunk0 = b * (kHeadBlock / 8);
      g.kh = b ? fold_w : kh;
      g.head_pairs = h->head_ctr.p + (b == 0 ? 1 : 3);  // (pairs sharing a term of the FIRST block: the statistic; the others' counts are dropped)
      hipLaunchKernelGGL(k_head_gemv, dim3((unsigned)blocks), dim3(256), 0, h->stream, g);
    }
    HIPCHK(h, hipGetLastError());
    h->st.head_flops = 2.0 * kt * (double)nq * (double)n_cand / (double)h->head_parts;
    return APSS_OK;
  }
  HeadGemmArgs g{};
  g.Wq = Wq;
  g.Wc = h->W.p;
  g.wq_rows = wq_rows;
  g.n_rows = n_cand;
  g.q_slot_base = q_slot_base;
  g.nq = (int32_t)nq;
  const int64_t qs0 = q_slot_base >= 0 ? q_slot_base : 0;
  g.qblock0 = qs0 / kHeadQBlock * kHeadQBlock;
  g.n_qblocks = (int32_t)(ceil_div(qs0 + nq, kHeadQBlock) - qs0 / kHeadQBlock);
  const int64_t ct = head_tile_rows(kh);
  g.n_ctiles = (int32_t)ceil_div(n_cand, ct);
  // candidate panels: enough workgroups to fill the chip several times over, a multiple of 8 (= XCDs) so that every
  // workgroup of an XCD streams panels of one residue class, and long enough to amortise the A-fragment load
  g.part = h->head_part;
  g.n_parts = h->head_parts;
  const int64_t my_ctiles = std::max<int64_t>(1, g.n_ctiles / g.n_parts);  // (this handle's share of the candidate tiles)
  int64_t panels = 8;
  while (panels * g.n_qblocks < 2048 && my_ctiles / (2 * panels) >= 32) panels *= 2;
  panels = std::max<int64_t>(1, std::min<int64_t>(panels, my_ctiles));
  g.n_panels = (int32_t)panels;
  g.q_ext = a.q_ext;
  g.c_ext = h->ext.p;
  g.thr = thr;
  g.thr_i = thr_i;
  g.inv_s2 = inv_s2;
  g.res_q = a.res_q;
  g.res_c = a.res_c;
  g.res_s = a.res_s;
  g.res_cap = a.res_cap;
  g.counters = a.counters;
  g.head_pairs = h->head_ctr.p + 1;
  g.kt = kt;
  // one launch multiplies a group of query blocks sized for about a second of matrix-core time (4e12 elements): a join of ten
  // million rows becomes a sequence of launches of bounded duration instead of one kernel that runs for a quarter of a minute
  const int64_t all_qblocks = g.n_qblocks, first_qblock0 = g.qblock0;
  const int64_t per_launch = std::max<int64_t>(1, (int64_t)(4e12 / ((double)kHeadQBlock * (double)ct * (double)my_ctiles)));
  for (int b = 0; b < n_blocks; ++b) {  // (block 1: the folded terms -- the same contraction, no pair statistic)
    g.chunk0 = b * (kHeadBlock / 8);
    for (int64_t q0 = 0; q0 < all_qblocks; q0 += per_launch) {
      g.n_qblocks = (int32_t)std::min<int64_t>(per_launch, all_qblocks - q0);
      g.qblock0 = first_qblock0 + q0 * kHeadQBlock;
      const dim3 grid((unsigned)((int64_t)g.n_qblocks * g.n_panels));
      // (three tile buffers + the barrier in mid-tile pay at KH = 256 only: 0.69 vs 0.67 of the bf16 peak; narrow blocks are
      // bound by their epilogue and lose with it: profiles/r03_head_gemm.md)
      // (the folded block has no positive count in its epilogue: there the three-buffer pipeline pays at 128 columns too,
      // 0.60 -> 0.68 of the peak at N = 1M)
      // INT8 rendering (one block of 128 | 256 byte-wide columns): v_mfma_i32_32x32x32_i8
      if (i8 && kh == 128) hipLaunchKernelGGL((k_head_gemm<128, true, 3, 8, true>), grid, dim3(512), 0, h->stream, g);
      else if (i8) hipLaunchKernelGGL((k_head_gemm<256, true, 3, 8, true>), grid, dim3(512), 0, h->stream, g);
      else if (b > 0 && fold_w == 128) hipLaunchKernelGGL((k_head_gemm<128, false, 3>), grid, dim3(512), 0, h->stream, g);
      else if (b > 0) hipLaunchKernelGGL((k_head_gemm<256, false, 3>), grid, dim3(512), 0, h->stream, g);
      else if (kh == 64) hipLaunchKernelGGL((k_head_gemm<64, true, 2>), grid, dim3(512), 0, h->stream, g);
      else if (kh == 128) hipLaunchKernelGGL((k_head_gemm<128, true, 2>), grid, dim3(512), 0, h->stream, g);
      else hipLaunchKernelGGL((k_head_gemm<256, true, 3>), grid, dim3(512), 0, h->stream, g);
    }
  }
  g.n_qblocks = (int32_t)all_qblocks;
  g.qblock0 = first_qblock0;
  HIPCHK(h, hipGetLastError());
  // multiplied elements: every (query block, candidate tile) the grid does not skip, at MFMA granularity
  double tiles = 0;
  for (int64_t b = 0; b < g.n_qblocks; ++b) {
    const int64_t hi = q_slot_base >= 0 ? std::min<int64_t>(g.n_ctiles, (g.qblock0 + (b + 1) * kHeadQBlock) / ct) : g.n_ctiles;
    tiles += hi > g.part ? (double)ceil_div(hi - g.part, g.n_parts) : 0.0;  // the tiles t < hi with t % n_parts == part
  }
  h->st.head_flops = 2.0 * kt * tiles * (double)ct * (double)kHeadQBlock;
  return APSS_OK;
}

// ---- probe the whole index with a query batch resident on the device ----
// q_head: rows of the batch in the dense-head block (null when the handle has none): the store's W for a stored batch,
// the staged q_W otherwise.
// Queries of more terms than a round of the filter takes (512) are cut into parts that share the accumulators: part v covers
// elements vrow_ptr[v] .. vrow_ptr[v + 1]) of query vrow_q[v]; vq_first[q] is query q's first part.
int32_t cut_long_queries(apss_handle *h, const int64_t *s_rowptr, int64_t nq, int vrow_part, ProbeArgs &a) {
  // queries of more terms than a round takes: cut them into parts that share the accumulators
  APSS_TRY(ensure(h, h->vrow_np, (size_t)nq + 1));
  APSS_TRY(ensure(h, h->vrow_first, (size_t)nq + 2));
  APSS_TRY(ensure(h, h->vq_first, (size_t)nq + 1));
  hipLaunchKernelGGL(k_vrow_count, dim3((unsigned)ceil_div(nq, 256)), dim3(256), 0, h->stream, s_rowptr, nq, vrow_part, h->vrow_np.p);
  APSS_TRY(scan_i64(h, (const int64_t *)h->vrow_np.p, h->vrow_first.p, nq));
  HIPCHK(h, hipGetLastError());
  int64_t nv = 0;
  HIPCHK(h, hipMemcpyAsync(&nv, h->vrow_first.p + nq, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  APSS_TRY(ensure(h, h->vrow_ptr, (size_t)nv + 1));
  APSS_TRY(ensure(h, h->vrow_q, (size_t)nv + 1));
  hipLaunchKernelGGL(k_vrow_fill, dim3((unsigned)ceil_div(nq + 1, 256)), dim3(256), 0, h->stream, s_rowptr, nq, vrow_part,
                     (const int64_t *)h->vrow_first.p, h->vq_first.p, h->vrow_ptr.p, h->vrow_q.p);
  HIPCHK(h, hipGetLastError());
  a.vq_first = h->vq_first.p;
  a.vrow_ptr = h->vrow_ptr.p;
  a.vrow_q = h->vrow_q.p;
  return APSS_OK;
}

// The exact pass of the two-pass join: the filters' survivors (h->res, h->n_res of them; with a dense-head block a pair may
// be there twice) are re-scored from the fp32 store and pruned at theta (k_rescore); then the rows that still wait outside the
// index are scored against every query, pair by pair (k_tail_score).  Leaves the final list in h->fin / h->n_res.
int32_t exact_pass(apss_handle *h, bool hybrid, double theta, const QueryRows &q, int64_t tail_n) {
  float ms = 0.f;
  // exact pass: re-score what the filter(s) let through from the fp32 store and prune at theta
  int64_t n_cand = h->n_res;
  h->st.filter_survivors = n_cand;
  h->n_res = 0;
  const int32_t *cand_q = h->res.q.p, *cand_c = h->res.c.p;
  if (hybrid && n_cand > 0) {
    // a pair that passed both filters is in the list twice
    uint64_t tab = 1024;
    while (tab < (uint64_t)n_cand * 2) tab <<= 1;
    APSS_TRY(ensure(h, h->dedup_tab, (size_t)tab, 0, true));
    APSS_TRY(h->uq.ensure(h, (size_t)n_cand, 0, true));
    HIPCHK(h, hipMemsetAsync(h->dedup_tab.p, 0xff, (size_t)tab * sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(h->counters.p, 0, sizeof(unsigned long long), h->stream));
    hipLaunchKernelGGL(k_pair_dedup, dim3((unsigned)ceil_div(n_cand, 256)), dim3(256), 0, h->stream,
                       (const int32_t *)h->res.q.p, (const int32_t *)h->res.c.p, (const float *)h->res.s.p, n_cand,
                       h->dedup_tab.p, tab - 1, h->uq.q.p, h->uq.c.p, h->uq.s.p, h->counters.p);
    HIPCHK(h, hipGetLastError());
    unsigned long long nu = 0;
    HIPCHK(h, hipMemcpyAsync(&nu, h->counters.p, sizeof(nu), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    n_cand = (int64_t)nu;
    cand_q = h->uq.q.p;
    cand_c = h->uq.c.p;
  }
  if (n_cand > 0) {
    APSS_TRY(h->fin.ensure(h, (size_t)n_cand, 0, true));
    HIPCHK(h, hipMemsetAsync(h->counters.p, 0, sizeof(unsigned long long), h->stream));
    HIPCHK(h, h->ev0.record(h->stream));
    // (a launch may not have 2^32 threads or more: 16 lanes per pair -> at most 2^27 pairs per launch)
    for (int64_t p0 = 0; p0 < n_cand; p0 += (1LL << 27)) {
      const RescoreArgs r = rescore_args(h, cand_q + p0, cand_c + p0, std::min<int64_t>(1LL << 27, n_cand - p0), nullptr, q, (float)theta, h->counters.p);
      hipLaunchKernelGGL(k_rescore, rescore_grid(r.n_pairs), dim3(kRescoreBlock), 0, h->stream, r);
      HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, h->ev1.record(h->stream));
    unsigned long long nfin = 0;
    HIPCHK(h, hipMemcpyAsync(&nfin, h->counters.p, sizeof(nfin), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
    h->st.rescore_ms = ms;
    h->n_res = (int64_t)nfin;
  }
  if (tail_n > 0) {
    // the rows that wait outside the index: every (query, tail row) pair, exactly (k_tail_score)
    const int64_t pairs = q.nq * tail_n;
    APSS_TRY(h->fin.ensure(h, (size_t)(h->n_res + pairs), (size_t)h->n_res));
    HIPCHK(h, hipMemsetAsync(h->counters.p, 0, kCtrCount * sizeof(unsigned long long), h->stream));
    const TailArgs t = tail_args(h, q, tail_n, (float)theta, h->n_res, h->counters.p);
    hipLaunchKernelGGL(k_tail_score, dim3((unsigned)ceil_div(pairs * kGroup, 256)), dim3(256), 0, h->stream, t);
    HIPCHK(h, hipGetLastError());
    unsigned long long tc[kCtrCount];
    HIPCHK(h, hipMemcpyAsync(tc, h->counters.p, sizeof(tc), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->n_res += (int64_t)tc[kCtrResults];
    h->st.posting_visits += (int64_t)tc[kCtrVisits];
    h->st.device_posting_visits += (int64_t)tc[kCtrVisits];
    h->st.candidate_pairs += (int64_t)tc[kCtrCands];
  }
  adopt_list(h, h->fin, h->n_res);
  return APSS_OK;
}

int32_t pack_query_head(apss_handle *h, const int64_t *rowptr, const int32_t *idx, const float *val, int64_t nq);

// ---- a query-type call over the index: ONE pass (probe_pass) is the stages below, in the order of their device work ----
constexpr int32_t kProbeAgain = 1;    // a stage latched a downgrade and rebuilt the index: the call runs again from the very top
constexpr int32_t kAttemptAgain = 2;  // the candidate list was grown: the attempt runs again

// single-pass exact kernels (k_probe_wave, k_probe): which one, its shape, its dynamic LDS
struct ExactKernel {
  bool wave, fx, cut;  // k_probe_wave | k_probe with signed fixed point (else fp32 atomics), with the per-round cut
  char variant;        // k_probe_wave's shape: 'A' | 'C'
  int block, u, longcap, survcap;
  size_t lds;
};

// the rows the SPARSE filter stages (s_*), the longest indexed row, the postings in the inverted index
struct StagedRows {
  const int64_t *rowptr;
  const int32_t *idx;
  const float *val;
  int64_t max_nnz, nnz_end;
  int64_t c_max_nnz, idx_nnz;
};

// what choose_path decides: the scales and the kernel family
struct ProbePath {
  double theta, bound, fx_scale;
  int mode;
  bool forced_general;
  double cx_shared, cx_scale, cx_theta, a8_scale;  // (cx_scale as launched: a8_scale when that is > 0; cx_theta: theta in its units)
  double byte_scale;  // acc8_scale of this call's norms and row lengths (0: its sums do not fit a byte): a8_scale where the tiles take 8-bit sums, k_probe_planes' scale
  bool coarse_path, cx_signed, shard_rule, hybrid, head_outside;
  float head_thr;
  int64_t tail_n, q_slot_base;
  const float *q_sub;
};

// one pass's state: probe_inner's batch, then what each stage settles for the ones behind it
struct Probe {
  QueryBatch q;
  StagedRows s;
  ProbePath p;
  ProbeArgs a;
  CxVariant cxv;
  ExactKernel xk;
  int64_t total_tiles, tiles_per_launch;
  bool chain, persist;
  int persist_slots;
};

// what one attempt's launches count and leave in the counters: read back in one go
struct AttemptCounts {
  int64_t n_launches = 0, thin_launches = 0;
  unsigned long long *c, *cc;  // the filter's counters; the chained exact pass's (the handle's scalar slots)
  unsigned long long sparse_results = 0, head_c[4] = {0, 0, 0, 0};
};

inline apss_handle::IndexSet &probe_index(apss_handle *h, const ProbePath &p) { return p.coarse_path ? h->cx : h->ex; }

int32_t reset_call(apss_handle *h, const Probe &pr) {
  name_last_batch(h, pr.q);
  h->n_res = 0;
  h->st.posting_visits = h->st.candidate_pairs = h->st.result_pairs = 0;
  h->st.device_posting_visits = 0;
  h->st.symmetric = 0;
  h->st.symmetric_declined = APSS_SYM_NOT_WHOLE;
  h->st.query_chunk = 0;
  h->st.filter_tile_rows = 0;
  h->st.probe_ms = 0;
  h->st.probe_launches = 0;
  h->st.thin_launches = 0;
  h->st.queries_per_round = 1;
  h->st.probe_kernel[0] = 0;
  h->cut_ran = false;
  h->cut_uncut = h->cut_rounds = 0;
  h->st.head_pairs = h->st.head_survivors = 0;
  h->st.head_ms = h->st.head_flops = 0;
  h->st.head_terms = h->head_k ? (int64_t)h->head_terms.size() : 0;
  h->st.head_columns = (uint32_t)h->head_k;
  h->st.head_int8 = h->head_k && h->head_i8 ? 1 : 0;
  APSS_TRY(ensure(h, h->counters, kCtrCount));
  h->st.filter_survivors = 0;
  h->st.rescore_ms = 0;
  return APSS_OK;
}

// What the SPARSE filter stages: the query rows themselves -- or, on a handle with a dense-head block, their tail view
// (the rows without the block's entries; a stored batch's was made when it was indexed, an outside batch's is made here).
// Exact rescoring, the waiting rows' direct scoring and apss_partial_scores_dev keep reading the whole rows.
int32_t stage_rows(apss_handle *h, Probe &pr) {
  StagedRows &s = pr.s;
  s = StagedRows{pr.q.rowptr, pr.q.idx, pr.q.val, pr.q.max_nnz, pr.q.nnz_end, 0, 0};
  if (h->head_k > 0) {
    const bool stored = pr.q.slot_first >= 0 && pr.q.slot_first < h->idx_rows;
    if (!stored) APSS_TRY(build_tail_view(h, h->qtv, pr.q.rowptr, pr.q.idx, pr.q.val, 0, pr.q.nq, 0, false));
    const apss_handle::TailView &v = stored ? h->tv : h->qtv;
    s.rowptr = stored ? v.rowptr.p + pr.q.slot_first : v.rowptr.p;
    s.idx = v.idx.p;
    s.val = v.val.p;
    s.max_nnz = v.max_nnz;
    s.nnz_end = v.nnz;
  }
  s.c_max_nnz = h->head_k > 0 ? h->tv.max_nnz : h->store_max_nnz;  // longest indexed row
  s.idx_nnz = h->head_k > 0 ? std::max<int64_t>(h->tv.nnz, 1) : h->nnz;  // postings in the inverted index
  return APSS_OK;
}

// k_probe_planes passed too much: back to k_probe_even's 16-bit sums, for good; the call runs again on the index as it is
int32_t drop_planes(apss_handle *h) {
  h->no_acc8 = true;
  h->downgrades |= APSS_DOWNGRADE_ACC8;
  return kProbeAgain;
}

// back to 16-bit accumulators over smaller tiles, for good; the call runs again
int32_t drop_acc8(apss_handle *h, bool shard_rule) {
  h->cx.cb = shard_rule ? 32768 : 65536;
  h->cx.n_tiles = 0;
  h->no_acc8 = true;
  h->downgrades |= APSS_DOWNGRADE_ACC8;
  APSS_TRY(build_index(h, 0));
  return kProbeAgain;
}

// The scales, and which of the three kernel families takes the call: the two-pass join (coarse filter + exact rescoring), the
// single-pass exact speed kernel, the general kernel.  Three of the downgrades that run the call again are decided here.
int32_t choose_path(apss_handle *h, Probe &pr) {
  ProbePath &p = pr.p;
  const double theta = p.theta = h->cfg.theta;
  if (!(theta > 0.0)) p.mode = 2;
  else if (!h->nonneg || (pr.q.slot_first < 0 && !h->q_nonneg) || (h->cfg.flags & APSS_FLAG_FORCE_SCAN)) p.mode = 1;
  else p.mode = 0;

  // every partial score must fit the fixed-point accumulators: by Cauchy-Schwarz a partial sum of non-negative
  // products is at most |q| * |c| <= the product of the largest row norms
  const double bound = p.bound = std::sqrt((double)pr.q.max_norm2) * std::sqrt((double)h->store_max_norm2) * 1.0001 + 1e-6;
  p.fx_scale = bound < 3.9 ? 1073741824.0 : (bound < 15.6 ? 268435456.0 : 0.0);
  p.forced_general = (h->cfg.flags & APSS_FLAG_FORCE_GENERAL) || h->dbgcfg.force_general;

  // ---- path 1: two-pass join (coarse filter + exact rescoring) ----
  // accumulator units per 1.0: a 16-bit sum holds S * |q||c| (fp16 weights: + 2^-11) plus one unit per shared term
  // S = the largest power of two that fits (2^15 for unit-norm input); un-normalised input gets a smaller one as long as
  // the threshold in units stays well above the round-up bias (one unit per shared term), else the filter passes too much
  const double cx_shared = p.cx_shared = (double)std::min<int64_t>(pr.s.max_nnz, pr.s.c_max_nnz);
  const Scale16 s16 = acc16_scale(bound, cx_shared, theta);
  double cx_scale = s16.scale;
  const double cx_theta = filter_threshold(theta, cx_scale);
  const bool cx_selective = s16.selective;
  const bool cx_fp16_ok = std::sqrt((double)h->store_max_norm2) < 60000.0;  // a weight never exceeds its row's norm
  // the shard rule (term-range shards, and the sparse half of a handle with a dense-head block) scales the threshold
  // down per query and tile: the kernel clamps it at 1, which only admits more
  const bool hybrid_wanted = h->head_k > 0;
  p.head_thr = (float)(theta - 0.0080 * bound - 1e-5);
  // weights of either sign with theta > 0 go through the filter too (it then sums positive products only: an upper bound of
  // the partial score, under the shard rule as much as without it -- the rule's ratios are norms); a handle with a
  // dense-head block (and long queries over 65536-row tiles) has no such instantiation and keeps the general kernel
  const bool shard_rule = p.shard_rule = h->sharded || hybrid_wanted;
  p.cx_signed = p.mode == 1 && !(h->cfg.flags & APSS_FLAG_FORCE_SCAN) && !hybrid_wanted &&
                (h->cx.cb <= 32768 || pr.s.max_nnz <= 512) && !h->dbgcfg.filter.chunk8 && !h->dbgcfg.filter.window;
  // 65536-row tiles (term shards; the sparse regime of a plain handle): the 8-bit filter -- 65536 candidates in 64 KB, two
  // 512-thread workgroups per CU -- if this call's norms and row lengths leave room for its sums
  const bool big_shard_tiles = shard_rule && h->cx.cb > 32768;
  p.byte_scale = p.mode == 0 && pr.s.max_nnz <= 512 ? acc8_scale(bound, cx_shared, theta) : 0.0;
  const double a8_scale = p.a8_scale = h->cx.cb >= 65536 && !h->dbgcfg.filter.no_acc8 && !h->no_acc8 && !h->dbgcfg.filter.chunk8 ? p.byte_scale : 0.0;
  // not this time (a long row, a large norm, signed weights): back to 16-bit accumulators over smaller tiles, for good
  if ((big_shard_tiles || h->cx.cb > 65536) && !(a8_scale > 0)) return drop_acc8(h, shard_rule);
  if (a8_scale > 0) cx_scale = a8_scale;
  p.cx_scale = cx_scale;
  p.cx_theta = filter_threshold(theta, cx_scale);
  p.coarse_path = h->use_coarse && (p.mode == 0 || p.cx_signed) && (cx_selective || a8_scale > 0) && cx_fp16_ok && !p.forced_general && pr.q.nq < (1LL << 30) &&
                  !(shard_rule && h->cx.cb > 32768 && !(a8_scale > 0)) &&
                  !h->dbgcfg.exact_accum && cx_scale > 0 && cx_theta < 65000.0 && (shard_rule || cx_theta - 2 >= 1.0) &&
                  std::min(pr.s.c_max_nnz * (int64_t)h->cx.cb, pr.s.idx_nnz) + (int64_t)kSegAlignC * h->cfg.dim < (1LL << 27);
  // rows waiting in the tail are scored pair by pair after the join over the index; that needs the two-pass path's final
  // list and a bounded number of pairs -- otherwise they are folded into the index first
  p.tail_n = h->n_rows - h->idx_rows;
  if (p.tail_n > 0 && (!(p.coarse_path && !h->sharded) || pr.q.nq * p.tail_n > kTailMaxPairs)) {
    APSS_TRY(build_index(h, h->idx_rows));
    return kProbeAgain;
  }
  // a stored batch that still waits in the tail is not in the index: for the join over the index it is an outside batch
  p.q_slot_base = pr.q.slot_first >= 0 && pr.q.slot_first < h->idx_rows ? pr.q.slot_first : -1;
  if (hybrid_wanted && !(p.coarse_path && p.mode == 0 && (h->head_i8 || p.head_thr >= 0.5 * theta))) {  // (the INT8 rows carry no rounding bound)
    // this call cannot take the hybrid path (signed or very long queries, norms out of range ...): the dense block's
    // terms go back into the inverted index, for good, and the call runs as on a handle without a block
    if (h->sharded)  // (a shard cannot leave the partition its peers were given)
      return fail(h, APSS_E_UNSUPPORTED, "this call needs the plain index (signed weights, norms out of the filter's range, theta <= 0): "
                                         "not available on a term shard with a dense-head block");
    h->head_blocked = true;
    h->downgrades |= APSS_DOWNGRADE_HEAD;
    APSS_TRY(build_index(h, 0));
    return kProbeAgain;
  }
  p.hybrid = hybrid_wanted;
  // the batch's rows of the dense-head block and its tail ratios: the store's were packed when it was indexed; an outside
  // batch (or one waiting in the tail) is packed here
  // A stored batch meets the block's candidates as a TRIANGLE (k_head_gemm skips the tiles above a query block; the block that
  // owns them reports the mirrored pair): right only when the batch is the store's last rows.  A window of a windowed call
  // (apss_window.hpp) has stored rows behind it that are no queries of its own: its rows are packed and multiplied as an
  // outside batch's, against every candidate tile (the pair of a row with itself is dropped by external id there)
  p.head_outside = p.hybrid && h->win_nonempty >= 0 && p.q_slot_base >= 0 && !h->sharded;
  if (p.hybrid && (p.q_slot_base < 0 || p.head_outside) && !h->sharded) APSS_TRY(pack_query_head(h, pr.q.rowptr, pr.q.idx, pr.q.val, pr.q.nq));  // (a shard's ingest packed them)
  p.q_sub = !shard_rule ? nullptr : (p.q_slot_base >= 0 ? h->sub.p + p.q_slot_base : h->q_sub.p);
  return APSS_OK;
}

// the kernels' arguments but the candidate list: store, staged rows, query chunks, the index rendering of the path
int32_t fill_probe_args(apss_handle *h, Probe &pr) {
  ProbeArgs &a = pr.a;
  a = ProbeArgs{};
  a.seg_stride = (int64_t)h->cfg.dim;
  a.ext_id = h->ext.p;
  a.c_scale = pr.p.shard_rule ? h->sub.p : nullptr;
  a.n_rows = h->idx_rows;
  a.q_rowptr = pr.s.rowptr;
  a.q_idx = pr.s.idx;
  a.q_val = pr.s.val;
  a.q_ext = pr.q.ext;
  a.q_scale = pr.p.shard_rule ? pr.p.q_sub : nullptr;
  a.nq = (int32_t)pr.q.nq;
  a.nq_rows = (int32_t)pr.q.nq;
  a.q_nnz_end = pr.s.nnz_end;
  // ~2 workgroups per CU per tile in flight at once, tiles swept one after another (tile-major grid) so the
  // chip works on one tile's postings at a time and they stay in L2 / Infinity Cache
  // ... that is the whole-store join (a million queries: 1024 chunks of ~1000 rounds each).  A streamed batch has few queries:
  // 1024 chunks would give a workgroup ONE round (B = 1024) for the price of its set-up (64 KB of accumulators cleared, the
  // tile's descriptors fetched) -- measured on C3 streamed in batches of 1024: probe kernels 655 ms at 1024 chunks, 143 ms at
  // 128.  So: as few chunks as still fill the chip eight times over with the tiles there are, never fewer than nq / 256.
  int64_t want_chunks = 1024;
  if (h->idx_rows > 0) {
    const int64_t tiles_now = std::max<int64_t>(1, ceil_div(h->idx_rows, h->use_coarse ? h->cx.cb : h->ex.cb));
    // (eight workgroups per resident slot: with four, the last, partly filled wave of workgroups cost a fifth of the launch.
    // That was the grid launch, which k_probe_coarse, k_probe_wave and k_probe keep.  k_probe_even's launch is persistent --
    // resident workgroups over a work list of these (tile, chunk) cells, the last ones cut finer: see prepare_work_lists -- and a
    // chunk there is the unit a workgroup's set-up is paid for, no longer the unit the end of the launch is ragged by.)
    want_chunks = std::min<int64_t>(1024, std::max<int64_t>(ceil_div(4096, tiles_now), ceil_div(pr.q.nq, 256)));
  }
  if (h->dbgcfg.chunks > 0) want_chunks = h->dbgcfg.chunks;
  a.q_chunk = (int32_t)std::max<int64_t>(1, ceil_div(pr.q.nq, want_chunks));
  a.n_chunks = (int32_t)ceil_div(pr.q.nq, a.q_chunk);
  a.q_slot_base = pr.p.q_slot_base;
  a.theta = (float)pr.p.theta;
  a.counters = h->counters.p;
  a.cx_scale = (float)pr.p.cx_scale;
  a.cx_theta = (float)pr.p.cx_theta;

  if (!pr.p.coarse_path) APSS_TRY(ensure_exact_index(h));
  const apss_handle::IndexSet &ix = probe_index(h, pr.p);
  a.tile_seg = ix.seg.p;
  a.post = h->ex.post.p;
  a.post_c = h->cx.post_c.p;
  a.tile_post_base = ix.base.p;
  a.tile_scale = pr.p.shard_rule ? (pr.p.coarse_path ? h->tile_min_c.p : h->tile_min.p) : nullptr;
  a.cb = ix.cb;
  a.n_tiles = (int32_t)ix.n_tiles;
  return APSS_OK;
}

// Which single-pass kernel takes the call if the two-pass join does not, and the fixed-point scale both count in
int32_t choose_exact_kernel(apss_handle *h, Probe &pr) {
  // ---- path 2: single-pass exact speed kernel (k_probe_wave); kernel shapes: A = 8 waves x 64-chunk window, one
  // workgroup per CU at 32768-row tiles; C = 8 waves x 40-chunk window, TWO workgroups per CU at <= 16384-row tiles
  pr.xk.variant = h->ex.cb <= 16384 ? 'C' : 'A';
  const int wave_block = 512;
  pr.xk.u = pr.xk.variant == 'A' ? 8 : 5;
  pr.xk.longcap = pr.xk.variant == 'A' ? 256 : 128;
  pr.xk.survcap = pr.xk.variant == 'A' ? 1024 : 512;
  // chunk descriptors pack (first posting * 8 + count - 1) into 32 bits: a tile's postings must number < 2^28
  pr.xk.wave = !pr.p.coarse_path && pr.p.mode == 0 && pr.p.fx_scale > 0 && pr.q.max_nnz <= wave_block && !pr.p.forced_general &&
               h->store_max_nnz * (int64_t)h->ex.cb + (int64_t)kSegAlign * h->cfg.dim < (1LL << 28);
  // ---- path 3: general kernel (k_probe): signed fixed point when the norms are bounded, else fp32 atomics ----
  pr.xk.fx = !pr.p.coarse_path && !pr.xk.wave && pr.p.fx_scale > 0;
  pr.xk.block = pr.xk.wave ? wave_block : gen_block(pr.p.mode, h->ex.cb);
  // the per-round cut (apss_set_top_k_tile_cut): only where the uncut list is the problem, k_probe<2> of a plain handle
  // (not while rows are marked removed: a round's k-th score could belong to one of them)
  pr.xk.cut = h->tile_cut && h->top_k > 0 && !h->sharded && !pr.p.coarse_path && !pr.xk.wave && pr.p.mode == 2 && h->rm_marked == 0;
  if (pr.xk.cut) {
    APSS_TRY(ensure(h, h->row_pairs, (size_t)pr.q.nq));
    pr.a.row_pairs = h->row_pairs.p;
    pr.a.cut_k = h->top_k;
  }
  const double scale_used = pr.xk.wave ? pr.p.fx_scale : pr.p.fx_scale / 2;
  pr.a.fx_scale = (float)scale_used;
  pr.a.theta_fx = (uint32_t)std::min(4294967295.0, std::max(1.0, std::ceil(pr.p.theta * scale_used)));
  pr.a.theta_fxi = (int32_t)std::max(-2147483647.0, std::min(2147483647.0, std::ceil(pr.p.theta * scale_used)));
  // (the filter kernels keep their LDS in static arrays: no dynamic allocation)
  pr.xk.lds = pr.p.coarse_path ? 0
              : pr.xk.wave     ? probe_wave_lds_bytes(h->ex.cb, wave_block, pr.xk.u, pr.xk.longcap, pr.xk.survcap)
                               : probe_lds_bytes(h->ex.cb, pr.xk.block, pr.p.mode);
  return APSS_OK;
}

// The filter kernel's instantiation (plan_filter, apss_filter_plan.hpp), with as many query rows per round as merge_rows_log2
// allows.  A fuse behind its estimate: a merged launch that reports more than two rounds per query row turns merging off for
// the handle (merge_off).
// (Term shards only, with or without a dense-head block -- power-law C5's 8 x 1 shard at N = 2M: tail filter 39.5 -> 24.0 ms.  The
// sparse half of a PLAIN handle with a block was tried: its rounds take 4-5 window steps, two rows do not fit one window.)
int32_t plan_merged_rounds(apss_handle *h, Probe &pr) {
  const ProbePath &p = pr.p;
  const FilterHooks &hooks = h->dbgcfg.filter;
  pr.cxv = CxVariant{};
  if (!p.coarse_path) return APSS_OK;
  const int max_merge_log2 = h->sharded && p.mode == 0 && !p.cx_signed && !h->merge_off
                                 ? merge_rows_log2(pr.q.nq, pr.s.nnz_end, h->cfg.term_lo, h->cfg.term_hi, p.a8_scale > 0, p.bound, p.cx_shared, p.theta, hooks) : 0;
  const FilterFacts f{p.a8_scale > 0, p.shard_rule, p.cx_signed, p.hybrid, pr.s.max_nnz, pr.s.nnz_end, pr.q.nq, pr.s.idx_nnz, max_merge_log2, p.byte_scale, pr.a.q_chunk,
                      h->cx.cb, h->cx.max_seg, h->cx.long_segs, h->cx.n_tiles, h->cx.round_chunks, h->n_rows, h->cfg.dim, h->cfg.term_lo, h->cfg.term_hi, h->no_acc8};
  std::string diag;
  const FilterPlan plan = plan_filter(f, hooks, h->dbgcfg.diag ? &diag : nullptr);
  if (!diag.empty()) fputs(diag.c_str(), stderr);
  if (!plan.listed) return fail(h, APSS_E_UNSUPPORTED, "no filter kernel for this combination of options");
  pr.cxv = plan.v;
  pr.a.flat_waves = plan.flat_waves;
  pr.a.flat_group_log2 = plan.flat_group_log2;
  pr.a.merge_log2 = plan.merge_log2;
  // the threshold in the units of byte sums (two planes: as a term shard's 8-bit filter takes it) or of a round's M rows
  if (plan.v.planes || plan.merge_log2 > 0) {
    const double S = plan.v.planes ? p.byte_scale : merged_scale(p.a8_scale > 0, p.bound, p.cx_shared, p.theta, plan.merge_log2);
    pr.a.cx_scale = (float)S;
    pr.a.cx_theta = (float)filter_threshold(p.theta, S);
  }
  return APSS_OK;
}

// ---- SYMMETRIC whole-store join: the batch IS the indexed store (query row v = stored row v: apss_self_join, or
// insert-and-query into an empty handle), so the pair (q, c) and the pair (c, q) share their terms and their score.  The
// filter runs a (query tile S, candidate tile T) workgroup only for T <= S and k_mirror_survivors adds the other direction
// of every survivor with T < S; both directions are then re-scored exactly, as without the symmetry: same result list,
// half the rounds.  Needs query chunks that do not straddle a tile (q_chunk | cb).  The reference finds both directions by
// probing twice (IndexingWorkerActor.scala:123-134); posting_visits / candidate_pairs keep counting what IT visits (the
// kernels count a tile pair below the diagonal twice: both statistics are symmetric in the two tiles), and
// device_posting_visits says what the kernels visited.
void decide_symmetry(apss_handle *h, Probe &pr) {
  const apss_handle::IndexSet &ix = probe_index(h, pr.p);
  uint32_t sym_declined = APSS_SYM_RAN;  // why not (apss_stats.symmetric_declined)
  if (h->dbgcfg.no_sym || (h->cfg.flags & APSS_FLAG_NO_SYMMETRY)) sym_declined = APSS_SYM_FLAG;
  else if (!(pr.p.q_slot_base == 0 && pr.q.nq == h->idx_rows && pr.q.nq == h->n_rows && pr.p.tail_n == 0)) sym_declined = APSS_SYM_NOT_WHOLE;
  else if (!pr.p.coarse_path) sym_declined = APSS_SYM_PATH;
  else if (pr.cxv.vrows) sym_declined = APSS_SYM_LONG_ROWS;
  else if (ix.n_tiles <= 1) sym_declined = APSS_SYM_ONE_TILE;
  else {
    int64_t qc = 1;
    while (qc < pr.a.q_chunk) qc <<= 1;
    if (qc <= ix.cb && ix.cb % qc == 0) {
      pr.a.tri = 1;
      pr.a.q_chunk = (int32_t)qc;
      pr.a.n_chunks = (int32_t)ceil_div(pr.q.nq, qc);
    } else {
      sym_declined = APSS_SYM_CHUNK;
    }
  }
  h->st.symmetric_declined = sym_declined;
  h->st.query_chunk = pr.a.q_chunk;
  h->st.filter_tile_rows = ix.cb;
  h->st.queries_per_round = 1 << pr.a.merge_log2;
}

// merged rounds: from here on the launch counts ROUNDS, and the rows' weights are staged divided by their shard factors
int32_t stage_merged_rows(apss_handle *h, Probe &pr) {
  // a chunk is a whole number of rounds (a symmetric join's power of two stays one)
  const int64_t M = 1LL << pr.a.merge_log2;
  const int64_t qc = ceil_div(pr.a.q_chunk, M) * M;
  pr.a.q_chunk = (int32_t)(qc / M);
  pr.a.n_chunks = (int32_t)ceil_div(pr.q.nq, qc);
  pr.a.nq = (int32_t)ceil_div(pr.q.nq, M);
  APSS_TRY(ensure(h, h->q_prenorm, (size_t)pr.s.nnz_end));
  hipLaunchKernelGGL(k_prenorm_rows, dim3((unsigned)ceil_div(pr.q.nq * kGroup, 256)), dim3(256), 0, h->stream, pr.s.rowptr, pr.s.val, pr.p.q_sub, pr.q.nq, h->q_prenorm.p);
  HIPCHK(h, hipGetLastError());
  pr.a.q_val = h->q_prenorm.p;
  return APSS_OK;
}

// ---- streamed batches (single-vector messages up to a few tens of thousands of rows): the exact pass is CHAINED behind the filter on the stream --
// k_rescore takes its pair count from the filter's counter on the device, k_tail_score appends to the same list -- and the
// call synchronises ONCE, reading all counters together (a host round trip costs as much as these kernels do)
constexpr int64_t kChainMaxQueries = 65536;

// tiles per launch, the candidate list's first reservation, whether the exact pass is chained
int32_t size_launches(apss_handle *h, Probe &pr) {
  // one launch sweeps a group of tiles sized for roughly 2e11 posting visits (a few hundred ms): a very large join
  // becomes a sequence of launches of bounded duration instead of one kernel that runs for tens of seconds
  const int64_t total_tiles = pr.total_tiles = probe_index(h, pr.p).n_tiles;
  int64_t tiles_per_launch = std::max<int64_t>(1, total_tiles);
  if (total_tiles > 0) {
    const double per_tile = (double)pr.s.nnz_end * ((double)pr.s.idx_nnz / (double)total_tiles / (double)h->cfg.dim) + 1.0;
    tiles_per_launch = (int64_t)std::min<double>((double)total_tiles, std::max(1.0, std::floor(2e11 / per_tile)));
    if (h->dbgcfg.tiles_per_launch > 0) tiles_per_launch = h->dbgcfg.tiles_per_launch;
    tiles_per_launch = std::min<int64_t>(tiles_per_launch, std::max<int64_t>(1, 2000000000LL / std::max(1, pr.a.n_chunks)));
  }
  pr.tiles_per_launch = tiles_per_launch;
  // room for two hits per query up front -- and, with a dense-head block, for what its filters passed on the policy's sample
  // (a narrow folded block passes a few pairs per million: 1e8 of them at N = 1e7): growing means running the whole probe again
  int64_t want_cap = std::min<int64_t>(2 * pr.q.nq, 1LL << 28);
  if (pr.p.hybrid && h->head_sample_frac > 0.0)
    want_cap = std::min<int64_t>(want_cap + (int64_t)(1.5 * h->head_sample_frac * (double)pr.q.nq * (double)h->idx_rows), 1LL << 30);
  else if (pr.p.hybrid && h->sharded)  // (a shard was given its head: no sample of its own; power-law C5 measured ~1 per query and shard)
    want_cap = std::min<int64_t>(want_cap + 6 * pr.q.nq, 1LL << 30);
  if (h->res.cap() < (size_t)want_cap) {
    const size_t cap0 = (size_t)(h->dbgcfg.res_cap > 0 ? h->dbgcfg.res_cap : std::max<int64_t>(1 << 20, want_cap));  // (res_cap: test hook, forces the regrowth path)
    APSS_TRY(h->res.ensure(h, cap0, 0, true));
  }
  if (pr.p.hybrid) APSS_TRY(ensure(h, h->head_ctr, 4));
  pr.chain = pr.p.coarse_path && !h->sharded && !pr.p.hybrid && !pr.a.tri && pr.q.nq <= kChainMaxQueries && !h->dbgcfg.no_chain;
  if (pr.chain) APSS_TRY(ensure(h, h->chain_ctr, kCtrCount));
  return APSS_OK;
}

// ---- k_probe_even: PERSISTENT launches (apss_even.hpp, apss_worklist.hpp).  One work list per launch of the call, built
// here, one behind the other, and kept in the handle with their keys: a call whose launches have the keys of the last
// call's (a join repeated, a stream of equal batches) uploads nothing.  The lists go up asynchronously from pinned memory.
// (A list of millions of cells -- a join of tens of millions of rows in small chunks -- is not worth its upload: grid launch.)
constexpr int kPersistFine = 128;  // rounds per item at the end of a list (profiles/persist_filter.md has the sweep)
constexpr int64_t kPersistMaxCells = 1LL << 22;
int32_t prepare_work_lists(apss_handle *h, Probe &pr) {
  pr.persist_slots = 0;
  pr.persist = pr.p.coarse_path && pr.cxv.even && !h->dbgcfg.no_persist && pr.total_tiles > 0 && pr.total_tiles * (int64_t)pr.a.n_chunks <= kPersistMaxCells;
  if (!pr.persist) return APSS_OK;
  APSS_TRY(even_resident_slots(h, pr.cxv, &pr.persist_slots));
  int fine = 1;
  while (2 * fine <= (h->dbgcfg.persist_fine > 0 ? h->dbgcfg.persist_fine : kPersistFine)) fine *= 2;
  std::vector<apss::WorkListKey> keys;
  for (int64_t t0 = 0; t0 < pr.total_tiles; t0 += pr.tiles_per_launch) {
    apss::WorkListKey k;
    k.q_slot_base = pr.a.merge_log2 > 0 ? pr.p.q_slot_base : -1;  // (decides own_tile, which only merged launches have)
    k.nq = pr.a.nq;
    k.nq_rows = pr.a.nq_rows;
    k.q_chunk = pr.a.q_chunk;
    k.n_chunks = pr.a.n_chunks;
    k.cb = pr.a.cb;
    k.tri = pr.a.tri;
    k.merge_log2 = pr.a.merge_log2;
    k.tile0 = (int32_t)t0;
    k.n_tiles = (int32_t)std::min<int64_t>(pr.tiles_per_launch, pr.total_tiles - t0);
    k.fine = fine;
    k.slots = h->dbgcfg.persist_wgs > 0 ? h->dbgcfg.persist_wgs : pr.persist_slots;
    keys.push_back(k);
  }
  if (keys == h->wl_keys && h->wl_dev.p) return APSS_OK;
  std::vector<apss::ProbeItem> items;
  h->wl_keys.clear();  // (nothing is cached while this fails half way)
  h->wl_off.assign(1, 0);
  h->wl_fine.clear();
  for (const apss::WorkListKey &k : keys) {
    h->wl_fine.push_back(apss::build_work_list(k, items));
    h->wl_off.push_back((int64_t)items.size());
  }
  if (h->wl_ev.made()) HIPCHK(h, hipEventSynchronize(h->wl_ev));  // the last upload has left the pinned buffer
  if (items.size() > h->wl_pin.cap) {
    const size_t cap = std::max<size_t>(items.size() + items.size() / 2, 4096);
    HIPCHK(h, h->wl_pin.grow(kGrowStage, cap, 0, nullptr, nullptr));
  }
  APSS_TRY(ensure(h, h->wl_dev, std::max<size_t>(items.size(), 1)));
  if (!items.empty()) {
    std::memcpy(h->wl_pin.p, items.data(), items.size() * sizeof(apss::ProbeItem));
    HIPCHK(h, hipMemcpyAsync(h->wl_dev.p, h->wl_pin.p, items.size() * sizeof(apss::ProbeItem), hipMemcpyHostToDevice, h->stream));
  }
  HIPCHK(h, h->wl_ev.record(h->stream));
  h->wl_keys = keys;
  return APSS_OK;
}

// ---- one attempt: the launches over the whole index with the candidate list as it is ----
// the lists the attempt fills, the counters at zero
int32_t begin_attempt(apss_handle *h, Probe &pr) {
  // chained: room for everything the candidate list can hold + every (query, waiting row) pair
  // (sized for the longest tail there can be, once: the tail grows by a row per message)
  if (pr.chain) APSS_TRY(h->fin.ensure(h, h->res.cap() + (size_t)(pr.q.nq * std::max<int64_t>(pr.p.tail_n, kTailMaxRows))));
  if (pr.a.merge_log2 > 0) APSS_TRY(h->res2.ensure(h, h->res.cap(), 0, true));  // (k_expand_merged writes the pairs out of place)
  pr.a.dbg = nullptr;
  h->res.as_candidates(pr.a);
  pr.a.res_cap = h->res.cap();
  HIPCHK(h, hipMemsetAsync(h->counters.p, 0, kCtrCount * sizeof(unsigned long long), h->stream));
  if (pr.xk.cut) HIPCHK(h, hipMemsetAsync(h->row_pairs.p, 0, (size_t)pr.q.nq * sizeof(uint32_t), h->stream));  // (every attempt: a re-run counts afresh)
  HIPCHK(h, h->ev0.record(h->stream));
  return APSS_OK;
}

// the instantiation this call launches, spelled as rocprofv3 prints it (apss_stats.probe_kernel)
void name_probe_kernel(apss_handle *h, const Probe &pr) {
  auto tf = [](bool b) { return b ? "true" : "false"; };
  char *nm = h->st.probe_kernel;
  const size_t cap = sizeof(h->st.probe_kernel);
  if (pr.p.coarse_path && pr.cxv.even)
    // (k_probe_planes<U> to rocprofv3; here it reads as what it is, the plain 512-thread instantiation with one more flag)
    if (pr.cxv.planes) snprintf(nm, cap, "k_probe_even<512, %d, 128, false, false, true, planes>", pr.cxv.u);
    else if (pr.cxv.merge) snprintf(nm, cap, "k_probe_even_merged<%d, %s>", pr.cxv.u, tf(pr.cxv.acc8));
    else snprintf(nm, cap, "k_probe_even<%d, %d, %d, %s, %s, %s>", pr.cxv.block, pr.cxv.u, pr.cxv.block <= 512 ? 128 : 256, tf(pr.cxv.shard), tf(pr.cxv.sgn), tf(pr.cxv.acc8));
  else if (pr.p.coarse_path)
    snprintf(nm, cap, "k_probe_coarse<%d, %d, %d, %d, %s, %d, %s, %s, %s, %s>", pr.cxv.block, pr.cxv.u, pr.cxv.block <= 512 ? 128 : 256,
             pr.cxv.block <= 512 ? 512 : 1024, tf(pr.cxv.shard), pr.cxv.chunk, tf(pr.cxv.vrows), tf(pr.cxv.sgn), tf(pr.cxv.longpf), tf(pr.cxv.acc8));
  else if (pr.xk.wave)
    snprintf(nm, cap, "k_probe_wave<%d, %d, %d, %d, %s, %s>", pr.xk.block, pr.xk.u, pr.xk.longcap, pr.xk.survcap, tf(h->sharded), tf(h->dbgcfg.diag));
  else if (pr.xk.cut)
    snprintf(nm, cap, "k_probe<%d, %d, %s, true>", pr.p.mode, pr.xk.block, tf(pr.xk.fx));
  else
    snprintf(nm, cap, "k_probe<%d, %d, %s>", pr.p.mode, pr.xk.block, tf(pr.xk.fx));
}

// diagnostic build of k_probe_wave: in-kernel cycle stamps per round segment (shares only; never a benchmark number)
int32_t launch_wave_diag(apss_handle *h, Probe &pr) {
  APSS_TRY(ensure(h, h->dbg, 8));
  HIPCHK(h, hipMemsetAsync(h->dbg.p, 0, 8 * sizeof(unsigned long long), h->stream));
  pr.a.dbg = h->dbg.p;
  APSS_TRY(launch_exact(h, wave_kernel(pr.xk.variant, h->sharded, true), pr.a, pr.xk.lds));
  unsigned long long d[8];
  HIPCHK(h, hipMemcpyAsync(d, h->dbg.p, sizeof(d), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  unsigned long long tot = 0;
  for (int k = 0; k < 7; ++k) tot += d[k];
  fprintf(stderr, "[apss diag] stage+flatten %.1f%% | atomics %.1f%% | longs/rest %.1f%% | barrier G %.1f%% | survivors %.1f%% | "
                  "re-zero %.1f%% | barrier U %.1f%% | cycles/round/wave %.0f\n",
          100.0 * d[0] / tot, 100.0 * d[1] / tot, 100.0 * d[2] / tot, 100.0 * d[3] / tot, 100.0 * d[4] / tot,
          100.0 * d[5] / tot, 100.0 * d[6] / tot, (double)tot / ((double)pr.a.n_tiles * pr.a.nq * (pr.xk.block / kWave)));
  return APSS_OK;
}

// one launch per group of tiles
int32_t launch_tile_groups(apss_handle *h, Probe &pr, AttemptCounts &n) {
  for (int64_t t0 = 0; t0 < pr.total_tiles; t0 += pr.tiles_per_launch, ++n.n_launches) {
    pr.a.tile0 = (int32_t)t0;
    pr.a.n_tiles = (int32_t)std::min<int64_t>(pr.tiles_per_launch, pr.total_tiles - t0);
    if (pr.p.coarse_path && pr.persist) {
      // (the work counter is zero behind the attempt's memset; a later launch of the call starts it again)
      if (n.n_launches > 0) HIPCHK(h, hipMemsetAsync(h->counters.p + kCtrWork, 0, sizeof(unsigned long long), h->stream));
      const int64_t n_items = h->wl_off[n.n_launches + 1] - h->wl_off[n.n_launches];
      pr.a.items = h->wl_dev.p + h->wl_off[n.n_launches];
      pr.a.n_items = (int32_t)n_items;
      pr.a.work_ctr = h->counters.p + kCtrWork;
      // never more workgroups than items
      const int64_t wgs = std::min<int64_t>(n_items, h->dbgcfg.persist_wgs > 0 ? h->dbgcfg.persist_wgs : pr.persist_slots);
      if (h->dbgcfg.diag)
        fprintf(stderr, "[apss diag] persist: items %lld fine %lld workgroups %lld\n", (long long)n_items, (long long)h->wl_fine[n.n_launches], (long long)wgs);
      if (wgs > 0) APSS_TRY(launch_cx(h, pr.cxv, pr.a, wgs));
      n.thin_launches += 1;
    } else if (pr.p.coarse_path) {
      APSS_TRY(launch_cx(h, pr.cxv, pr.a));
      n.thin_launches += pr.cxv.even ? 1 : 0;
    } else if (pr.xk.wave && h->dbgcfg.diag) {
      APSS_TRY(launch_wave_diag(h, pr));
    } else if (pr.xk.wave) {
      APSS_TRY(launch_exact(h, wave_kernel(pr.xk.variant, h->sharded, false), pr.a, pr.xk.lds));
    } else {
      APSS_TRY(launch_exact(h, gen_kernel(pr.p.mode, pr.xk.block, pr.xk.fx, pr.xk.cut), pr.a, pr.xk.lds));
    }
  }
  return APSS_OK;
}

// merged rounds: (round, candidate) -> the round's (query row, candidate) pairs
int32_t expand_merged_rounds(apss_handle *h, Probe &pr) {
  hipLaunchKernelGGL(k_counter_move, dim3(1), dim3(1), 0, h->stream, h->counters.p, (int)kCtrResults, (int)kCtrPre);
  hipLaunchKernelGGL(k_expand_merged, dim3((unsigned)std::min<int64_t>(1024, ceil_div(pr.q.nq / 4 + 4096, 256))), dim3(256), 0, h->stream, (const int32_t *)pr.a.res_q, (const int32_t *)pr.a.res_c, (const float *)pr.a.res_s,
                     (const unsigned long long *)(h->counters.p + kCtrPre), (uint64_t)pr.a.res_cap, pr.a.merge_log2, pr.q.nq, pr.q.ext, (const int64_t *)h->ext.p,
                     h->res2.q.p, h->res2.c.p, h->res2.s.p, h->counters.p + kCtrResults, h->counters.p + kCtrOver);
  HIPCHK(h, hipGetLastError());
  h->res.swap(h->res2);
  h->res.as_candidates(pr.a);
  pr.a.res_cap = std::min(h->res.cap(), h->res2.cap());
  if (!(h->sharded && !h->dbgcfg.no_merge_prune)) return APSS_OK;
  // ... and only those of them that pass the shard rule on their EXACT partial score stay (k_shard_prune): the exchange
  // gets no more candidates than without merging
  hipLaunchKernelGGL(k_counter_move, dim3(1), dim3(1), 0, h->stream, h->counters.p, (int)kCtrResults, (int)kCtrPre);
  ShardPruneArgs sp{};
  h->res.as_in(sp);
  sp.n_in = h->counters.p + kCtrPre;
  sp.cap = pr.a.res_cap;
  sp.q_rowptr = pr.s.rowptr;
  sp.q_idx = pr.s.idx;
  sp.q_val = pr.s.val;
  sp.q_sub = pr.p.q_sub;
  sp.c_rowptr = h->head_k ? h->tv.rowptr.p : h->rowptr.p;
  sp.c_idx = h->head_k ? h->tv.idx.p : h->idx.p;
  sp.c_val = h->head_k ? h->tv.val.p : h->val.p;
  sp.c_sub = h->sub.p;
  sp.theta = (float)pr.p.theta;
  h->res2.as_out(sp);
  sp.counter = h->counters.p + kCtrResults;
  sp.over = h->counters.p + kCtrOver;
  // (a grid for what a shard usually reports -- a fraction of a pair per query row; the kernel strides over whatever the counter holds)
  const int64_t grid_pairs = std::min<int64_t>((int64_t)pr.a.res_cap, pr.q.nq / 4 + 4096);
  hipLaunchKernelGGL(k_shard_prune, dim3((unsigned)std::min<int64_t>(2048, ceil_div(grid_pairs, kPrunePairs * 4))), dim3(kPruneBlock), 0, h->stream, sp);
  HIPCHK(h, hipGetLastError());
  h->res.swap(h->res2);
  h->res.as_candidates(pr.a);
  return APSS_OK;
}

// a symmetric join: the other direction of every survivor
int32_t mirror_survivors(apss_handle *h, const Probe &pr) {
  HIPCHK(h, hipMemcpyAsync(h->counters.p + kCtrSnap, h->counters.p + kCtrResults, sizeof(unsigned long long), hipMemcpyDeviceToDevice, h->stream));
  hipLaunchKernelGGL(k_mirror_survivors, dim3(1024), dim3(256), 0, h->stream, pr.a.res_q, pr.a.res_c, pr.a.res_s,
                     (const unsigned long long *)(h->counters.p + kCtrSnap), (uint64_t)pr.a.res_cap, (int32_t)pr.a.cb, h->counters.p + kCtrResults);
  HIPCHK(h, hipGetLastError());
  return APSS_OK;
}

// The exact pass CHAINED behind the filter (exact_pass is the same pass with its own host round trips): the pair count is read
// on the device, the grid is sized for what such a batch usually passes, both kernels count in chain_ctr and append to ONE list
int32_t chained_exact_pass(apss_handle *h, const Probe &pr, AttemptCounts &n) {
  HIPCHK(h, hipMemsetAsync(h->chain_ctr.p, 0, kCtrCount * sizeof(unsigned long long), h->stream));
  const RescoreArgs r = rescore_args(h, h->res.q.p, h->res.c.p, (int64_t)pr.a.res_cap, h->counters.p + kCtrResults, pr.q, (float)pr.p.theta, h->chain_ctr.p + kCtrResults);
  // (the kernel strides over whatever the counter holds)
  const int64_t grid_pairs = std::min<int64_t>((int64_t)pr.a.res_cap, 64 * pr.q.nq + 4096);
  hipLaunchKernelGGL(k_rescore, rescore_grid(grid_pairs), dim3(kRescoreBlock), 0, h->stream, r);
  if (pr.p.tail_n > 0) {
    const TailArgs t = tail_args(h, pr.q, pr.p.tail_n, (float)pr.p.theta, 0, h->chain_ctr.p);  // (out_base 0: appends through the same counter as k_rescore)
    hipLaunchKernelGGL(k_tail_score, dim3((unsigned)ceil_div(pr.q.nq * pr.p.tail_n * kGroup, 256)), dim3(256), 0, h->stream, t);
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(n.cc, h->chain_ctr.p, kCtrCount * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  return APSS_OK;
}

// the dense half: same candidate list, same counter
int32_t launch_head(apss_handle *h, const Probe &pr, AttemptCounts &n) {
  HIPCHK(h, hipMemcpyAsync(&n.sparse_results, h->counters.p + kCtrResults, sizeof(n.sparse_results), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemsetAsync(h->head_ctr.p, 0, 4 * sizeof(unsigned long long), h->stream));
  HIPCHK(h, h->ev2.record(h->stream));
  const bool stored = pr.p.q_slot_base >= 0 && !pr.p.head_outside;
  APSS_TRY(run_head(h, pr.a, pr.q.nq, stored ? pr.p.q_slot_base : -1, stored ? h->W.p : h->q_W.p, stored ? (int64_t)(h->W.cap / h->head_k) : ceil_div(pr.q.nq, kHeadCTile) * kHeadCTile, pr.p.head_thr, pr.p.bound, h->idx_rows));
  HIPCHK(h, h->ev3.record(h->stream));
  HIPCHK(h, hipMemcpyAsync(n.head_c, h->head_ctr.p, sizeof(n.head_c), hipMemcpyDeviceToHost, h->stream));
  return APSS_OK;
}

// the call's one synchronisation: every counter of the attempt is on the host behind it
int32_t read_counters(apss_handle *h, AttemptCounts &n) {
  HIPCHK(h, hipMemcpyAsync(n.c, h->counters.p, kCtrCount * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return APSS_OK;
}

int32_t account_counters(apss_handle *h, const Probe &pr, const AttemptCounts &n) {
  const bool tri = pr.a.tri != 0;
  float ms = 0.f;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  h->st.probe_ms += ms;
  h->st.probe_launches += n.n_launches;
  h->st.thin_launches += n.thin_launches;
  h->st.posting_visits = (int64_t)n.c[kCtrVisits];
  h->st.device_posting_visits = (int64_t)(tri ? n.c[kCtrDevVisits] : n.c[kCtrVisits]);
  h->st.symmetric = tri ? 1u : 0u;
  h->st.candidate_pairs = (int64_t)n.c[kCtrCands];
  // the speed paths count a stored query's touch of its own slot; it is not a (q, c != q) pair
  if ((pr.xk.wave || pr.p.coarse_path) && pr.p.q_slot_base >= 0)
    h->st.candidate_pairs -= h->win_nonempty >= 0 ? h->win_nonempty  // (a window of the batch: its own non-empty rows)
                             : h->head_k > 0 ? ((pr.p.q_slot_base == 0 && pr.q.nq == h->n_rows) ? h->tv.nonempty : h->tv.last_nonempty)
                                             : ((pr.p.q_slot_base == 0 && pr.q.nq == h->n_rows) ? h->store_nonempty : h->last_batch_nonempty);
  if (pr.p.hybrid) {
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev2, h->ev3));
    h->st.head_ms += ms;
    // positive elements of the contraction, minus a stored query's product with itself
    int64_t self = 0;
    if (pr.p.q_slot_base >= 0)
      self = h->win_head_nonempty >= 0 ? h->win_head_nonempty
                                       : (pr.p.q_slot_base == 0 && pr.q.nq == h->n_rows) ? h->head_nonempty : h->last_batch_head_nonempty;
    h->st.head_pairs = (int64_t)n.head_c[1] - self;
    h->st.head_survivors = (int64_t)(n.c[kCtrResults] - n.sparse_results);
    // a pair sharing head AND tail terms is scored by both filters; the distinct count lies between max and sum
    h->st.candidate_pairs = std::max(h->st.candidate_pairs, h->st.head_pairs);
  }
  h->st.result_pairs = (int64_t)n.c[kCtrResults];
  // (kCtrPre: the rounds the filter reported, or -- with the shard-rule test behind it -- the pairs they expanded to)
  if (pr.a.merge_log2 > 0 && (int64_t)n.c[kCtrPre] > (2 * pr.q.nq + 100000) * (h->sharded && !h->dbgcfg.no_merge_prune ? (1LL << pr.a.merge_log2) : 1LL))
    h->merge_off = true;  // (this call's list is right, the filter just passed too much)
  return APSS_OK;
}

// the result list overflowed (or a list on the way to it did: kCtrOver): grow to what the run asked for; the (idempotent) probe
// is repeated
int32_t grow_candidates(apss_handle *h, const Probe &pr, const AttemptCounts &n) {
  const size_t asked = (size_t)std::max(n.c[kCtrResults], n.c[kCtrOver]);
  size_t need = asked + asked / 8 + 1024;
  if (pr.a.tri) {
    // a symmetric run whose FILTER overflowed mirrored only what the list held: the counter under-reports.  What the run
    // needs is known all the same: the filter's own count (kCtrSnap, taken before the mirror) twice over, plus what the
    // dense half appended -- asked for at once, instead of one more overflow per stage (each retry is a whole probe)
    const size_t snap = (size_t)n.c[kCtrSnap];
    const size_t head_part = pr.p.hybrid && n.c[kCtrResults] > n.sparse_results ? (size_t)(n.c[kCtrResults] - n.sparse_results) : 0;
    need = std::max(need, 2 * snap + head_part + (2 * snap + head_part) / 8 + 1024);
  }
  APSS_TRY(h->res.ensure(h, need, 0, true));
  ++h->probe_reruns;
  return kAttemptAgain;
}

// the attempt's list held everything: the call's final list and its last statistics
int32_t finish_call(apss_handle *h, const Probe &pr, const AttemptCounts &n) {
  if (pr.chain) {  // the exact pass has run already: its list is final
    h->st.filter_survivors = (int64_t)n.c[kCtrResults];
    h->st.posting_visits += (int64_t)n.cc[kCtrVisits];
    h->st.device_posting_visits += (int64_t)n.cc[kCtrVisits];
    h->st.candidate_pairs += (int64_t)n.cc[kCtrCands];
    adopt_list(h, h->fin, (int64_t)n.cc[kCtrResults]);
    return APSS_OK;
  }
  adopt_list(h, h->res, (int64_t)n.c[kCtrResults]);
  if (pr.xk.cut) {  // (kCtrPre, kCtrSnap: the uncut total and the rounds cut -- words k_probe<2> leaves alone otherwise)
    h->cut_ran = true;
    h->cut_uncut = (int64_t)n.c[kCtrPre];
    h->cut_rounds = (int64_t)n.c[kCtrSnap];
  }
  if (pr.p.coarse_path && h->sharded) h->st.filter_survivors = h->n_res;  // a shard's survivors are its candidates (phase 2 scores them)
  if (pr.p.coarse_path && !h->sharded) APSS_TRY(exact_pass(h, pr.p.hybrid, pr.p.theta, pr.q, pr.p.tail_n));
  return APSS_OK;
}

// One attempt.  APSS_OK: the call is finished; kAttemptAgain: the list was grown; kProbeAgain: the 8-bit filter was dropped
int32_t run_attempt(apss_handle *h, Probe &pr) {
  AttemptCounts n;
  n.cc = h->scalars->chain_ctr;
  n.c = h->scalars->attempt_ctr;
  APSS_TRY(begin_attempt(h, pr));
  name_probe_kernel(h, pr);
  APSS_TRY(launch_tile_groups(h, pr, n));
  if (pr.a.merge_log2 > 0) APSS_TRY(expand_merged_rounds(h, pr));
  if (pr.a.tri) APSS_TRY(mirror_survivors(h, pr));
  HIPCHK(h, h->ev1.record(h->stream));
  for (int k = 0; k < kCtrCount; ++k) n.cc[k] = 0;
  if (pr.chain) APSS_TRY(chained_exact_pass(h, pr, n));
  if (pr.p.hybrid) APSS_TRY(launch_head(h, pr, n));
  APSS_TRY(read_counters(h, n));
  APSS_TRY(account_counters(h, pr, n));
  // the 8-bit filter turned out unselective on this data (skewed terms: chance pairs share dozens of them, and every
  // shared term adds its unit of round-up): correct, but the survivors would swamp the exact pass.  Back to 16-bit
  // accumulators, for good, and run the call again.
  if (pr.cxv.acc8 && (int64_t)n.c[kCtrResults] > std::max<int64_t>(64 * pr.q.nq, 4000000)) return pr.cxv.planes ? drop_planes(h) : drop_acc8(h, pr.p.shard_rule);
  if (std::max(n.c[kCtrResults], n.c[kCtrOver]) > pr.a.res_cap) return grow_candidates(h, pr, n);
  return finish_call(h, pr, n);
}

// One pass of the call.  kProbeAgain: a downgrade was latched and the index rebuilt (no room for 8-bit sums, waiting rows folded
// into the index, dense head blocked, 8-bit filter unselective) -- the call runs again
int32_t probe_pass(apss_handle *h, Probe &pr) {
  APSS_TRY(reset_call(h, pr));
  if (pr.q.nq == 0 || h->n_rows == 0 || pr.q.nnz_end <= 0 || h->nnz == 0) return APSS_OK;  // nothing can share a term
  if (pr.q.nq > 0x7fffffffLL) return fail(h, APSS_E_INVALID, "query batch too large");
  APSS_TRY(stage_rows(h, pr));
  APSS_TRY(choose_path(h, pr));
  APSS_TRY(fill_probe_args(h, pr));
  APSS_TRY(choose_exact_kernel(h, pr));
  APSS_TRY(plan_merged_rounds(h, pr));
  decide_symmetry(h, pr);
  if (pr.a.merge_log2 > 0) APSS_TRY(stage_merged_rows(h, pr));
  const int vrow_part = 512;
  if (pr.p.coarse_path && pr.s.max_nnz > vrow_part) APSS_TRY(cut_long_queries(h, pr.s.rowptr, pr.q.nq, vrow_part, pr.a));
  APSS_TRY(size_launches(h, pr));
  APSS_TRY(prepare_work_lists(h, pr));
  for (int attempt = 0; attempt < 3; ++attempt) {
    const int32_t rc = run_attempt(h, pr);
    if (rc != kAttemptAgain) return rc;
  }
  return fail(h, APSS_E_STATE, "result buffer kept overflowing");
}

// Every repeat follows a one-way latch (no_acc8, head_blocked, idx_rows == n_rows): at most three of them
// (*n_results, where the caller wants it, is zero from here on: what an error return leaves; probe writes the call's count)
int32_t probe_inner(apss_handle *h, const QueryBatch &batch, int64_t *n_results) {
  if (n_results) *n_results = 0;
  Probe pr{batch};
  for (int pass = 0; pass < 4; ++pass) {
    const int32_t rc = probe_pass(h, pr);
    if (rc != kProbeAgain) return rc;
  }
  return fail(h, APSS_E_STATE, "the call kept downgrading the index");
}

// ---- the list stages behind the join (apss_stage.hpp): each takes the call's list where adopt_list left it and adopts its own ----
// One stage that owns its device memory and reports a hipError_t -- or, through *bad, that its own counts disagree: its arrays
// grow against the handle's reservation (`mem`), and a failure takes the call's list with it
template <class F>
int32_t run_stage(apss_handle *h, const char *what, StageMem &mem, F fn) {
  mem.ledger = &h->bytes_reserved;
  const char *bad = nullptr;
  const hipError_t e = fn(&bad);
  if (e == hipSuccess) return APSS_OK;
  h->n_res = -1;
  h->err = std::string(what) + ": " + (bad ? bad : hipGetErrorString(e));
  return bad ? APSS_E_STATE : e == hipErrorOutOfMemory ? APSS_E_NOMEM : APSS_E_DEVICE;
}

// The cut of one final list (the call's, or a window's): the kept list is adopted, *info says what was done.
int32_t cut_final_list(apss_handle *h, int64_t nq, apss_topk_info *info) {
  // (a probe that cut its rounds: the list is what it emitted, the rows' uncut counts say what the call found)
  APSS_TRY(run_stage(h, "per-query top-k", h->topk.mem, [&](const char **) {
    return topk_run(h->topk, h->stream, h->out_q, h->out_c, h->out_s, h->n_res, nq, h->ext.p, h->n_rows, h->top_k, info,
                    h->cut_ran ? h->row_pairs.p : nullptr, h->cut_uncut);
  }));
  if (h->n_res > 0) adopt_list(h, h->topk.out_q.p, h->topk.out_c.p, h->topk.out_s.p, info->kept);
  return APSS_OK;
}

// Windows of a query-type call (apss_window.hpp): b(q) on the device, the greedy cuts on the host.  Fills h->win_cuts and the
// planning fields of h->tw; b (and, with `bits`, the rows' non-empty bits behind it) is left in `hb`.
int32_t plan_windows(apss_handle *h, const QueryBatch &batch, const int64_t *sv_rowptr, std::vector<int32_t> &hb) {
  const int32_t dim = h->cfg.dim;
  const int64_t nq = batch.nq;
  APSS_TRY(ensure(h, h->win_df, (size_t)dim));
  APSS_TRY(ensure(h, h->win_b, (size_t)(2 * nq)));
  HIPCHK(h, hipMemsetAsync(h->win_df.p, 0, (size_t)dim * sizeof(unsigned int), h->stream));
  HIPCHK(h, begin_timed(h->stream, h->ev0));
  if (h->nnz >= (1LL << 40)) return fail(h, APSS_E_UNSUPPORTED, "windowed top-k: more than 2^40 stored entries");  // (k_win_df's grid)
  if (h->nnz > 0) {
    hipLaunchKernelGGL(k_win_df, dim3((unsigned)ceil_div(h->nnz, kTopkBlock)), dim3(kTopkThreads), 0, h->stream, (const int32_t *)h->idx.p, h->nnz, dim,
                       h->win_df.p);
    ++h->tw.plan_launches;
  }
  hipLaunchKernelGGL(k_win_bound, dim3((unsigned)ceil_div(nq * kWinWave, kWinThreads)), dim3(kWinThreads), 0, h->stream, batch.rowptr, batch.idx, nq,
                     (const unsigned int *)h->win_df.p, dim, h->n_rows, sv_rowptr, h->win_b.p, h->win_b.p + nq);
  ++h->tw.plan_launches;
  HIPCHK(h, hipGetLastError());
  hb.resize((size_t)(sv_rowptr ? 2 * nq : nq));
  float ms = 0.f;
  HIPCHK(h, end_timed_read(h->stream, h->ev0, h->ev1, {{hb.data(), h->win_b.p, hb.size() * sizeof(int32_t)}}, &ms));
  h->tw.plan_ms = ms;
  // a window: the longest run of rows from its start whose bounds sum to <= max_pairs; a row over the budget is a window of one
  const int64_t budget = h->top_k_window;
  h->win_cuts.assign(1, 0);
  int64_t sum = 0;
  for (int64_t q = 0; q < nq; ++q) {
    const int64_t b = hb[(size_t)q];
    h->tw.bound_total += b;
    if (q > h->win_cuts.back() && sum + b > budget) {
      h->win_cuts.push_back(q);
      sum = 0;
    }
    sum += b;
    h->tw.bound_window_max = std::max(h->tw.bound_window_max, sum);
    if (b > budget) ++h->tw.single_row_over;
  }
  h->win_cuts.push_back(nq);
  h->tw.windows = (int32_t)(h->win_cuts.size() - 1);
  h->tw.rows_window_min = nq;
  for (size_t w = 0; w + 1 < h->win_cuts.size(); ++w) {
    const int64_t rows = h->win_cuts[w + 1] - h->win_cuts[w];
    h->tw.rows_window_min = std::min(h->tw.rows_window_min, rows);
    h->tw.rows_window_max = std::max(h->tw.rows_window_max, rows);
  }
  return APSS_OK;
}

// the statistics of a windowed call that are sums over its windows
template <class F>
void for_summed_stats(apss_stats &a, const apss_stats &b, F f) {
  f(a.posting_visits, b.posting_visits);
  f(a.device_posting_visits, b.device_posting_visits);
  f(a.candidate_pairs, b.candidate_pairs);
  f(a.filter_survivors, b.filter_survivors);
  f(a.probe_launches, b.probe_launches);
  f(a.thin_launches, b.thin_launches);
  f(a.probe_ms, b.probe_ms);
  f(a.rescore_ms, b.rescore_ms);
  f(a.head_ms, b.head_ms);
  f(a.head_flops, b.head_flops);
  f(a.head_pairs, b.head_pairs);
  f(a.head_survivors, b.head_survivors);
}

// ---- removal (apss_remove.hpp) ----
// every slot of the store gets its mark byte: rows stored since the map was last extended are live
int32_t rm_extend(apss_handle *h) {
  if (h->dead_rows >= h->n_rows && h->dead.p) return APSS_OK;
  APSS_TRY(ensure(h, h->dead, (size_t)std::max<int64_t>(h->n_rows, 1), (size_t)h->dead_rows));
  if (h->n_rows > h->dead_rows)
    HIPCHK(h, hipMemsetAsync(h->dead.p + h->dead_rows, 0, (size_t)(h->n_rows - h->dead_rows), h->stream));
  h->dead_rows = h->n_rows;
  return APSS_OK;
}

// the most workgroups of k_rm_mark / k_rm_drop / k_rm_rows (they loop over the rest); APSS_DEBUG=rm_grid=N: N, a test hook that
// makes a small store take their loops' later trips
int64_t rm_grid_cap(const apss_handle *h, int64_t cap) { return h->dbgcfg.rm_grid > 0 ? h->dbgcfg.rm_grid : cap; }

// The final list of a query-type call (or of one window) without the pairs that touch a marked row: the filtered list is
// adopted.  Runs only while rows are marked; q_slot_first >= 0: the query rows are stored rows from that slot on.
int32_t drop_removed(apss_handle *h, int64_t q_slot_first) {
  if (h->rm_marked <= 0 || h->n_res <= 0) return APSS_OK;
  APSS_TRY(rm_extend(h));
  APSS_TRY(h->rm_out.ensure(h, (size_t)h->n_res));
  APSS_TRY(ensure(h, h->rm_ctr, 1));
  HIPCHK(h, hipMemsetAsync(h->rm_ctr.p, 0, sizeof(unsigned long long), h->stream));
  RmDropArgs a{};
  a.in_q = h->out_q;
  a.in_c = h->out_c;
  a.in_s = h->out_s;
  a.n = h->n_res;
  a.dead = h->dead.p;
  a.rows = h->n_rows;
  a.q_slot_first = q_slot_first;
  h->rm_out.as_out(a);
  a.kept = h->rm_ctr.p;
  HIPCHK(h, begin_timed(h->stream, h->rm_ev0));
  const int64_t blocks = ceil_div(h->n_res, (int64_t)kRmThreads * kRmItems);
  hipLaunchKernelGGL(k_rm_drop, dim3((unsigned)std::min<int64_t>(blocks, rm_grid_cap(h, 16384))), dim3(kRmThreads), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  unsigned long long *kept = &h->scalars->removal_kept;
  float ms = 0.f;
  HIPCHK(h, end_timed_read(h->stream, h->rm_ev0, h->rm_ev1, {{kept, h->rm_ctr.p, sizeof(*kept)}}, &ms));
  if ((int64_t)*kept > h->n_res) return fail(h, APSS_E_STATE, "the removal filter kept more pairs than it was given");
  h->ri.pairs_dropped += h->n_res - (int64_t)*kept;
  h->ri.drop_ms += ms;
  ++h->ri.drop_launches;
  adopt_list(h, h->rm_out, (int64_t)*kept);
  return APSS_OK;
}

// ---- components of the join (apss_components.hpp) ----
// every slot a singleton again and complete as an un-joined store is: nothing is launched (cc_extend initialises the slots when the
// structure is next used).  counted: a reset the caller did not ask for (removal, compaction, a failed stage)
void reset_components(apss_handle *h, bool counted) {
  cc_reset(h->cc);
  h->cci.complete = h->n_rows == 0;
  if (counted) ++h->cci.resets;
}

// one launch sequence of the stage: the reservation follows it, a failure leaves the structure reset
template <class F>
int32_t components_stage(apss_handle *h, F fn) {
  const int32_t rc = run_stage(h, "components", h->cc.mem, [&](const char **) { return fn(); });
  if (rc != APSS_OK) reset_components(h, true);
  return rc;
}

// The list of `batch` (the call's, or one window's) behind the removal filter goes into the forest: launches only.  probe() has
// said whether the batch is rows of the store
int32_t absorb_components(apss_handle *h, const QueryBatch &batch) {
  if (h->cci.declined != APSS_CC_RAN) return APSS_OK;
  if (h->cut_ran) {  // (the probe cut its rounds: what it left is not every pair)
    h->cci.declined = APSS_CC_TILE_CUT;
    return APSS_OK;
  }
  if (h->n_res <= 0) return APSS_OK;
  APSS_TRY(components_stage(h, [&] {
    return cc_hook(h->cc, h->stream, h->out_q, h->out_c, h->n_res, batch.slot_first, batch.slots, batch.nq, h->n_rows,
                   h->dbgcfg.cc_grid > 0 ? h->dbgcfg.cc_grid : kCcGridCap, &h->cci.hook_launches, &h->cci.hook_ms);
  }));
  h->cci.pairs_absorbed += h->n_res;
  return APSS_OK;
}

// label[] and the counts are those of parent[] (the lazy half of the stage: ONE synchronisation when something changed)
int32_t label_components(apss_handle *h) {
  h->cci.label_launches = 0;
  if (!h->cc.dirty && h->cci.rows == h->n_rows) return APSS_OK;
  const bool marks = h->rm_marked > 0 && h->dead.p;
  unsigned long long *w = h->scalars->components;
  APSS_TRY(components_stage(h, [&] {
    return cc_label(h->cc, h->stream, h->n_rows, marks ? h->dead.p : nullptr, marks ? h->dead_rows : 0, w, &h->cci.label_launches, &h->cci.label_ms,
                    &h->cci.hook_ms);
  }));
  h->cci.rows = h->n_rows;
  h->cci.rows_live = h->n_rows - h->rm_marked;
  h->cci.unions_total = (int64_t)w[0];
  h->cci.components = (int64_t)w[1];
  h->cci.singletons = (int64_t)w[2];
  h->cci.largest = (int64_t)w[3];
  return APSS_OK;
}

// What the join of `batch` (the call's, or one window's) left, finished: while rows are marked removed, ONE filter of that list
// (apss_remove.hpp); then, with apss_set_components, the list's pairs hooked into the components (apss_components.hpp: launches
// only); then, with apss_set_top_k, ONE pass of the per-query top-k over it (apss_topk.hpp), reported in *info.
int32_t finish_list(apss_handle *h, const QueryBatch &batch, apss_topk_info *info) {
  APSS_TRY(drop_removed(h, batch.slot_first));
  if (h->cc_on) APSS_TRY(absorb_components(h, batch));
  info->pairs_over_theta = info->kept = h->n_res;
  if (batch.absorb_only) {  // (the forest has the list: nobody reads it, so no cut selects from it and a window keeps none of it)
    info->kept = 0;
    adopt_list(h, h->out_q, h->out_c, h->out_s, 0);
    return APSS_OK;
  }
  if (h->top_k <= 0 || h->sharded) return APSS_OK;
  return cut_final_list(h, batch.nq, info);
}

// A query-type call's list: the join (probe_inner runs its pass again after a downgrade or a rebuild; what it leaves is the final
// list of its rows) and finish_list -- once over the whole batch, or, with apss_set_top_k_window, window by window over the query
// rows (apss_window.hpp), the kept lists concatenated.
int32_t probe_lists(apss_handle *h, const QueryBatch &batch, int64_t *n_results) {
  const int64_t nq = batch.nq;
  h->tk = apss_topk_info{};
  h->tw = apss_topk_window_info{};
  h->tw.max_pairs = h->top_k_window;
  h->win_cuts.clear();
  h->tci = apss_topk_tile_cut_info{};
  h->tci.prefix_bits = 16;
  h->tci.declined = !h->tile_cut ? APSS_TILE_CUT_OFF
                    : h->top_k <= 0 ? APSS_TILE_CUT_NO_K
                    : h->rm_marked > 0 ? APSS_TILE_CUT_REMOVED  // (choose_exact_kernel: a round's k-th score could be a marked row's)
                                       : APSS_TILE_CUT_PATH;
  h->ri.pairs_dropped = 0;
  h->ri.drop_ms = 0;
  h->ri.drop_launches = 0;
  auto note_cut = [h]() {  // after a probe_inner: what its probe emitted and cut (the sum over a call's windows)
    h->tci.pairs_emitted += h->n_res;
    h->tci.rounds_cut += h->cut_rounds;
    if (h->cut_ran) {
      h->tci.applied = 1;
      h->tci.declined = APSS_TILE_CUT_RAN;
    }
  };
  const bool windowed = h->top_k > 0 && h->top_k_window > 0 && !h->sharded && nq <= 0x7fffffffLL && nq * h->n_rows > h->top_k_window;
  if (!windowed) {
    APSS_TRY(probe_inner(h, batch, n_results));
    note_cut();
    return finish_list(h, batch, &h->tk);
  }
  // ---- the plan.  A stored batch of a handle with a dense-head block: the rows' tail view tells which of them the sparse
  // filter / the block see at all (the per-window self-touch corrections); a batch the view does not cover (it waits outside the
  // index) is corrected by its rows with any entry at all, should a window fold it in: candidate_pairs stays a lower bound
  h->n_res = -1;  // (the last call's list may live in buffers the windows reuse: gone from here on, also when the plan fails)
  const bool bits = h->head_k > 0 && batch.slot_first >= 0 && batch.slot_first + nq <= h->tv.rows && h->tv.rowptr.p;
  std::vector<int32_t> hb;
  APSS_TRY(plan_windows(h, batch, bits ? h->tv.rowptr.p + batch.slot_first : nullptr, hb));
  const int64_t kept_max = [&] {
    int64_t s = 0;
    for (int64_t q = 0; q < nq; ++q) s += std::min<int64_t>(hb[(size_t)q], h->top_k);
    return s;
  }();
  APSS_TRY(h->win.ensure(h, (size_t)std::max<int64_t>(kept_max, 1), 0, true));
  if (h->dbgcfg.res_cap <= 0) {
    // no window overflows its candidate list: the bound holds for the filters' survivors too (twice with a dense-head block,
    // whose two filters may both pass a pair)
    const size_t need = (size_t)std::max<int64_t>(1, h->tw.bound_window_max * (h->head_k > 0 ? 2 : 1));
    APSS_TRY(h->res.ensure(h, need, 0, true));
  }
  apss_stats sum{};
  apss_topk_info tk{};
  tk.k = h->top_k;
  int64_t n_out = 0;
  int32_t rc = APSS_OK;
  for (size_t w = 0; w + 1 < h->win_cuts.size() && rc == APSS_OK; ++w) {
    const int64_t r0 = h->win_cuts[w], r1 = h->win_cuts[w + 1];
    h->win_nonempty = h->win_head_nonempty = 0;
    for (int64_t q = r0; q < r1; ++q) {
      const int32_t ne = bits ? hb[(size_t)(nq + q)] : (hb[(size_t)q] > 0 ? 3 : 0);
      h->win_nonempty += ne & 1;
      h->win_head_nonempty += (ne >> 1) & 1;
    }
    const int64_t reruns = h->probe_reruns;
    const QueryBatch window = batch.rows(r0, r1);
    rc = probe_inner(h, window, nullptr);
    if (rc != APSS_OK) break;
    if (h->probe_reruns > reruns) ++h->tw.overflow_reruns;
    note_cut();
    h->tw.pairs_window_max = std::max(h->tw.pairs_window_max, h->n_res);
    for_summed_stats(sum, h->st, [](auto &s, const auto &v) { s += v; });
    apss_topk_info one{};
    rc = finish_list(h, window, &one);  // (the window's list loses its removed rows before its cut)
    if (rc != APSS_OK) break;
    tk.pairs_over_theta += one.pairs_over_theta;
    tk.kept += one.kept;
    tk.queries_cut += one.queries_cut;
    tk.longest_segment = std::max(tk.longest_segment, one.longest_segment);
    tk.select_ms += one.select_ms;
    tk.select_launches += one.select_launches;
    if (h->n_res > 0) {
      if (n_out + h->n_res > (int64_t)h->win.cap()) {  // (cannot happen: a row keeps at most min(b, k) pairs)
        rc = fail(h, APSS_E_STATE, "a window kept more pairs than its rows' bounds allow");
        break;
      }
      hipLaunchKernelGGL(k_win_append, dim3((unsigned)std::min<int64_t>(4096, ceil_div(h->n_res, kWinThreads))), dim3(kWinThreads), 0, h->stream,
                         h->out_q, h->out_c, h->out_s, h->n_res, (int32_t)r0, h->win.q.p + n_out, h->win.c.p + n_out, h->win.s.p + n_out);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) {
        rc = fail(h, APSS_E_DEVICE, std::string("k_win_append: ") + hipGetErrorString(e));
        break;
      }
      n_out += h->n_res;
    }
  }
  h->win_nonempty = h->win_head_nonempty = -1;
  if (rc == APSS_OK) {
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) rc = fail(h, APSS_E_DEVICE, std::string("windowed top-k: ") + hipGetErrorString(e));
  }
  name_last_batch(h, batch);  // (the handle names the whole batch again, whatever the last window left)
  if (rc != APSS_OK) {
    h->n_res = -1;
    return rc;
  }
  for_summed_stats(h->st, sum, [](auto &s, const auto &v) { s = v; });
  h->tk = tk;
  adopt_list(h, h->win, n_out);
  return APSS_OK;
}

// The global cut of the call's final list (apss_top_pairs.hpp): its K best pairs in rank order are adopted.
int32_t cut_top_pairs(apss_handle *h, const QueryBatch &batch) {
  h->tpi.pairs_in = h->n_res;
  if (h->n_res <= 0) return APSS_OK;
  if (h->n_res > 0xffffffffLL) {
    h->n_res = -1;
    return fail(h, APSS_E_UNSUPPORTED, "global top-K: a final list of 2^32 pairs or more");
  }
  APSS_TRY(run_stage(h, "global top-K", h->tp.mem, [&](const char **bad) {
    return tp_run(h->tp, h->stream, h->out_q, h->out_c, h->out_s, h->n_res, batch.ext, batch.nq, h->ext.p, h->n_rows, h->top_pairs,
                  h->dbgcfg.tp_grid > 0 ? h->dbgcfg.tp_grid : kTpGridCap, h->scalars->top_pairs, &h->tpi, bad);
  }));
  adopt_list(h, h->tp.out_q.p, h->tp.out_c.p, h->tp.out_s.p, h->tpi.kept);
  return APSS_OK;
}

// the whole store as a query batch (apss_self_join; its last rows: apss_insert_and_query)
QueryBatch store_batch(const apss_handle *h) {
  return QueryBatch{{h->n_rows, h->rowptr.p, h->idx.p, h->val.p, h->ext.p}, 0, h->store_max_nnz, h->store_max_norm2, h->nnz};
}

// A query-type call: its list (probe_lists), then, with apss_set_top_pairs, ONE global cut of that list.  *n_results is written
// here, from what the last stage adopted
int32_t probe(apss_handle *h, const QueryBatch &batch, int64_t *n_results) {
  h->tpi = apss_top_pairs_info{};
  h->tpi.k_pairs = h->top_pairs;
  if (h->cc_on) {  // (finish_list absorbs the list, or every window's, when the batch is rows of the store)
    h->cci.declined = batch.slot_first < 0 && !batch.slots && batch.nq > 0 ? APSS_CC_OUTSIDE : APSS_CC_RAN;
    h->cci.pairs_absorbed = 0;
    h->cci.hook_launches = 0;
    h->cci.hook_ms = 0;
    h->cc.hook_open = false;
  }
  APSS_TRY(probe_lists(h, batch, n_results));
  if (h->top_pairs > 0 && !h->sharded && !batch.absorb_only) APSS_TRY(cut_top_pairs(h, batch));
  if (n_results) *n_results = h->n_res;
  return APSS_OK;
}

int32_t validate_host_csr(apss_handle *h, int64_t n, const int64_t *rowptr, const int32_t *indices,
                          const double *values, const int64_t *ext_ids) {
  if (n < 0) return fail(h, APSS_E_INVALID, "negative row count");
  if (n == 0) return APSS_OK;
  if (!rowptr || !ext_ids) return fail(h, APSS_E_INVALID, "null rowptr / ext_ids");
  if (rowptr[0] != 0) return fail(h, APSS_E_INVALID, "rowptr[0] must be 0");
  for (int64_t i = 0; i < n; ++i)
    if (rowptr[i + 1] < rowptr[i]) return fail(h, APSS_E_INVALID, "rowptr must be non-decreasing");
  if (rowptr[n] > 0 && (!indices || !values)) return fail(h, APSS_E_INVALID, "null indices / values");
  return APSS_OK;
}

// host CSR (double values, as SparkSparseVector.values) -> device input staging (float values).  The doubles are
// copied as they are and narrowed on the device: a host-side conversion loop cost more than the extra PCIe bytes.
__global__ void k_narrow_f64(const double *in, float *out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = (float)in[i];
}

int32_t upload(apss_handle *h, int64_t n, const int64_t *rowptr, const int32_t *indices, const double *values,
               const int64_t *ext_ids) {
  const int64_t nnz = n ? rowptr[n] : 0;
  APSS_TRY(ensure(h, h->in_val, (size_t)std::max<int64_t>(nnz, 1)));
  const size_t off_ext = (size_t)(n + 1) * sizeof(int64_t), off_val = off_ext + (size_t)n * sizeof(int64_t);
  const size_t off_idx = off_val + (size_t)nnz * sizeof(double), bytes = off_idx + (size_t)nnz * sizeof(int32_t);
  if (n > 0 && h->pin.p && bytes <= kPinBytes) {
    // a small message: packed into pinned memory [rowptr | ext ids | values | indices] -> ONE truly asynchronous copy, no
    // synchronisation here (the staging is the handle's own: the caller's arrays are consumed by the memcpy below, and every
    // entry point synchronises before it returns)
    APSS_TRY(ensure(h, h->pack, kPinBytes));
    std::memcpy(h->pin.p, rowptr, off_ext);
    std::memcpy(h->pin.p + off_ext, ext_ids, (size_t)n * sizeof(int64_t));
    if (nnz) {
      std::memcpy(h->pin.p + off_val, values, (size_t)nnz * sizeof(double));
      std::memcpy(h->pin.p + off_idx, indices, (size_t)nnz * sizeof(int32_t));
    }
    HIPCHK(h, hipMemcpyAsync(h->pack.p, h->pin.p, bytes, hipMemcpyHostToDevice, h->stream));
    h->up_rowptr = reinterpret_cast<const int64_t *>(h->pack.p);
    h->up_ext = reinterpret_cast<const int64_t *>(h->pack.p + off_ext);
    h->up_idx = reinterpret_cast<const int32_t *>(h->pack.p + off_idx);
    if (nnz) {
      hipLaunchKernelGGL(k_narrow_f64, dim3((unsigned)std::min<int64_t>(2048, ceil_div(nnz, 256))), dim3(256), 0, h->stream,
                         reinterpret_cast<const double *>(h->pack.p + off_val), h->in_val.p, nnz);
      HIPCHK(h, hipGetLastError());
    }
    return APSS_OK;
  }
  APSS_TRY(ensure(h, h->in_rowptr, (size_t)n + 1));
  APSS_TRY(ensure(h, h->in_ext, (size_t)std::max<int64_t>(n, 1)));
  APSS_TRY(ensure(h, h->in_idx, (size_t)std::max<int64_t>(nnz, 1)));
  APSS_TRY(ensure(h, h->in_val64, (size_t)std::max<int64_t>(nnz, 1)));
  h->up_rowptr = h->in_rowptr.p;
  h->up_ext = h->in_ext.p;
  h->up_idx = h->in_idx.p;
  if (n) {
    HIPCHK(h, hipMemcpyAsync(h->in_rowptr.p, rowptr, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->in_ext.p, ext_ids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  }
  if (nnz) {
    HIPCHK(h, hipMemcpyAsync(h->in_idx.p, indices, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->in_val64.p, values, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_narrow_f64, dim3(2048), dim3(256), 0, h->stream, (const double *)h->in_val64.p, h->in_val.p, nnz);
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));  // the caller's buffers may be reused on return
  return APSS_OK;
}

int32_t insert_dev_impl(apss_handle *h, int64_t n, int64_t nnz, const int64_t *d_rowptr, const int32_t *d_idx,
                        const float *d_val, const int64_t *d_ext, int64_t *first_new_row) {
  *first_new_row = h->n_rows;
  if (n == 0) return APSS_OK;
  forget_last_call(h);  // (the results and the query batch of the last call may point into store arrays that this insert reallocates)
  if (h->n_rows + n > 0x7fffffffLL) return fail(h, APSS_E_INVALID, "more than 2^31 - 1 vectors in one handle");
  int64_t kept_rows = 0, kept_nnz = 0;
  const bool was_nonneg = h->nonneg;
  APSS_TRY(ingest(h, n, nnz, d_rowptr, d_idx, d_val, d_ext, true, &kept_rows, &kept_nnz));
  if (h->sharded && h->head_k && !h->nonneg) {  // refused before anything is committed: the index stays as it was
    h->nonneg = was_nonneg;
    return fail(h, APSS_E_UNSUPPORTED, "a term shard with a dense-head block needs non-negative weights (apss_set_head_terms)");
  }
  const int64_t row0 = h->n_rows;
  h->n_rows += kept_rows;
  h->nnz += kept_nnz;
  if (h->cc_on && kept_rows > 0) h->cci.complete = 0;  // (new slots, singletons once the structure is next used; their edges were never seen)
  // a small batch onto an existing index waits in the TAIL (k_tail_score scores it directly) until the tail is worth a
  // rebuild of the last tile: a single-vector message then costs no pass over the dim-wide segment table
  const bool tail_ok = h->use_coarse && !h->sharded && h->idx_rows > 0 && !h->dbgcfg.no_tail;
  if (tail_ok && kept_rows <= kTailMaxBatch && h->n_rows - h->idx_rows <= kTailMaxRows) {
    h->st.build_ms = 0;
    return APSS_OK;
  }
  APSS_TRY(build_index(h, row0));
  return APSS_OK;
}

// rows of the dense-head block and tail ratios of a query batch given as CSR with absolute row offsets
int32_t pack_query_head(apss_handle *h, const int64_t *rowptr, const int32_t *idx, const float *val, int64_t nq) {
  const int64_t q_pad = ceil_div(nq, kHeadCTile) * kHeadCTile;
  APSS_TRY(ensure(h, h->q_W, (size_t)(q_pad * h->head_k)));
  APSS_TRY(ensure(h, h->q_sub, (size_t)nq));
  // (a query batch with larger norms than the store's shrinks the block's scale: the store's rows are re-quantised)
  APSS_TRY(head_fit_scale(h, std::max((double)h->store_max_norm2, (double)h->q_max_norm2), reinterpret_cast<unsigned char *>(h->W.p),
                          ceil_div(h->idx_rows, kHeadCTile) * kHeadCTile * (int64_t)h->head_k));
  HeadPackArgs a{};
  head_pack_rendering(h, a);
  a.rowptr = rowptr;
  a.idx = idx;
  a.val = val;
  a.row0 = 0;
  a.row1 = nq;
  a.head_pos = h->head_pos.p;
  a.kh = h->head_k;
  a.W = h->q_W.p;
  a.w_row0 = 0;
  a.w_pad = q_pad;
  a.ratio_t = h->q_sub.p;
  a.head_nonempty = nullptr;
  a.row_inv = nullptr;
  a.prune_above = -INFINITY;
  a.fold_from = h->head_exact;
  hipLaunchKernelGGL(k_head_pack, dim3((unsigned)ceil_div(q_pad, 8)), dim3(512), 0, h->stream, a);
  HIPCHK(h, hipGetLastError());
  return APSS_OK;
}

int32_t query_dev_impl(apss_handle *h, int64_t n, int64_t nnz, const int64_t *d_rowptr, const int32_t *d_idx,
                       const float *d_val, const int64_t *d_ext, int64_t *n_results) {
  // the results and the query batch of the last call live until the next query-type call: this one restages q_* (a plain
  // batch is written there before its flags are known, and the buffers may be reallocated), so they are gone from here on --
  // also when this batch is rejected (the result calls then answer APSS_E_STATE, as after an insert)
  forget_last_call(h);
  int64_t kept_rows = 0, kept_nnz = 0;
  APSS_TRY(ingest(h, n, nnz, d_rowptr, d_idx, d_val, d_ext, false, &kept_rows, &kept_nnz));
  // the batch's rows of the dense-head block and its tail ratios (the store's were packed when it was indexed)
  if (h->head_k && !h->sharded && kept_rows > 0) APSS_TRY(pack_query_head(h, h->q_rowptr.p, h->q_idx.p, h->q_val.p, kept_rows));
  return probe(h, QueryBatch{{kept_rows, h->q_rowptr.p, h->q_idx.p, h->q_val.p, h->q_ext.p}, -1, h->q_max_nnz, h->q_max_norm2, kept_nnz}, n_results);
}

// apss_clear: the index, the store and the marks go, the reservations and the settings stay
int32_t clear_impl(apss_handle *h) {
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->n_rows = 0;
  h->idx_rows = 0;
  h->nnz = 0;
  h->n_tiles = 0;
  for (apss_handle::IndexSet *s : {&h->ex, &h->cx}) { s->n_tiles = 0; s->post_used = 0; s->h_base.clear(); s->built_rows = 0; }
  h->ex_built_rows = 0;
  forget_last_call(h);
  h->nonneg = true;
  h->q_nonneg = true;
  h->no_acc8 = h->dbgcfg.filter.no_acc8;
  h->merge_off = false;
  h->downgrades = 0;
  h->store_max_nnz = 0;
  h->store_max_norm2 = 0.f;
  h->store_nonempty = 0;
  if (!h->head_fixed) {  // (terms set through apss_set_head_terms are configuration: they outlive the data)
    h->head_k = 0;
    h->head_terms.clear();
  }
  h->head_eval_rows = 0;
  h->head_blocked = false;
  h->head_nonempty = 0;
  h->cut_lo = h->cut_hi = 0;
  h->df_rows = -1;
  h->rm_marked = 0;  // (the marks belong to slots, and the slots are gone)
  h->dead_rows = 0;
  if (h->cc_on) reset_components(h, false);  // (the setting stays, the structure is empty: complete)
  return APSS_OK;
}

int32_t refuse_shard_removal(apss_handle *h, const char *what) {
  return fail(h, APSS_E_UNSUPPORTED, std::string(what) + ": not on a term shard (it holds slices of rows; a compaction needs whole ones)");
}

// An id list of a call, d_ids[0, n) (device, n > 0), ascending in h->rm_sorted (rocprim radix sort through h->rm_tmp).  What the
// sort needs is reserved first; the sort itself opens the call's timed stretch (e0)
int32_t sort_ids(apss_handle *h, const int64_t *d_ids, int64_t n, DevEvent &e0) {
  APSS_TRY(ensure(h, h->rm_sorted, (size_t)n));
  size_t tmp_bytes = 0;
  HIPCHK(h, rocprim::radix_sort_keys(nullptr, tmp_bytes, d_ids, h->rm_sorted.p, (size_t)n, 0, 64, h->stream));
  APSS_TRY(ensure(h, h->rm_tmp, tmp_bytes + 256));
  HIPCHK(h, begin_timed(h->stream, e0));
  HIPCHK(h, rocprim::radix_sort_keys((void *)h->rm_tmp.p, tmp_bytes, d_ids, h->rm_sorted.p, (size_t)n, 0, 64, h->stream));
  return APSS_OK;
}

// ---- components across a removal (apss_components_repair.hpp) ----
// what apss_components_repair_info says of a call, before the call knows that it marked a row
void begin_repair_call(apss_handle *h) {
  apss_components_repair_info &ri = h->ccri;
  ri.declined = h->ccr_max <= 0 ? APSS_CCR_OFF : !h->cc_on ? APSS_CCR_NO_COMPONENTS : APSS_CCR_NOTHING;
  ri.rows_marked = ri.components_touched = ri.rows_rejoined = ri.pairs_rejoined = 0;
  ri.detach_ms = ri.rejoin_ms = 0;
  ri.launches = 0;
}

int32_t repair_components(apss_handle *h, int64_t marked);

// marks the stored rows whose external id is in d_ids[0, n) (device); *newly = rows that were live before
int32_t remove_impl(apss_handle *h, int64_t n, const int64_t *d_ids, int64_t *newly) {
  *newly = 0;
  if (n == 0 || h->n_rows == 0) return APSS_OK;
  if (n > 0x7fffffffLL) return fail(h, APSS_E_INVALID, "apss_remove: more than 2^31 - 1 ids in one call");
  APSS_TRY(rm_extend(h));
  APSS_TRY(ensure(h, h->rm_ctr, 1));
  HIPCHK(h, hipMemsetAsync(h->rm_ctr.p, 0, sizeof(unsigned long long), h->stream));
  APSS_TRY(sort_ids(h, d_ids, n, h->rm_ev0));
  // (two rows per thread; the workgroups loop: one global add each)
  const int64_t blocks = ceil_div(ceil_div(h->n_rows, 2), kRmThreads);
  hipLaunchKernelGGL(k_rm_mark, dim3((unsigned)std::min<int64_t>(blocks, rm_grid_cap(h, 4096))), dim3(kRmThreads), 0, h->stream, (const int64_t *)h->ext.p, h->n_rows,
                     (const int64_t *)h->rm_sorted.p, n, h->dead.p, h->rm_ctr.p);
  HIPCHK(h, hipGetLastError());
  unsigned long long marked = 0;
  float ms = 0.f;
  HIPCHK(h, end_timed_read(h->stream, h->rm_ev0, h->rm_ev1, {{&marked, h->rm_ctr.p, sizeof(marked)}}, &ms));
  h->ri.mark_ms = ms;
  h->rm_marked += (int64_t)marked;
  h->ri.removed_total += (int64_t)marked;
  *newly = (int64_t)marked;
  h->ccri.rows_marked = (int64_t)marked;
  if (h->cc_on && marked > 0) {  // (a removed row can split a component)
    if (h->ccr_max <= 0) {
      reset_components(h, true);
    } else {  // ... so the components that held one are taken apart and re-joined
      const int32_t rc = repair_components(h, (int64_t)marked);
      if (rc != APSS_OK) reset_components(h, true);  // (the marks stay: the removal happened)
      return rc;
    }
  }
  return APSS_OK;
}

// The live rows, gathered on the device into the input staging (k_rm_rows -> the handle's scan -> k_rm_gather), then what
// apss_clear + apss_insert_stored_dev of them does.  A failure behind the clear leaves an empty handle and the error.
int32_t compact_impl(apss_handle *h) {
  if (h->rm_marked <= 0) return APSS_OK;
  const int64_t n = h->n_rows, marked = h->rm_marked;
  APSS_TRY(rm_extend(h));
  for (DevBuf<int64_t> *b : {&h->s_keep, &h->s_cnt, &h->s_rowdst, &h->s_nnzdst}) APSS_TRY(ensure(h, *b, (size_t)n + 1));
  HIPCHK(h, begin_timed(h->stream, h->rm_ev0));
  hipLaunchKernelGGL(k_rm_rows, dim3((unsigned)std::min<int64_t>(ceil_div(n, kRmThreads), rm_grid_cap(h, 4096))), dim3(kRmThreads), 0, h->stream,
                     (const uint8_t *)h->dead.p, (const int64_t *)h->rowptr.p, n, h->s_keep.p, h->s_cnt.p);
  HIPCHK(h, hipGetLastError());
  APSS_TRY(scan_i64(h, (const int64_t *)h->s_keep.p, h->s_rowdst.p, n));
  APSS_TRY(scan_i64(h, (const int64_t *)h->s_cnt.p, h->s_nnzdst.p, n));
  // with apss_set_components_repair the forest moves with the rows: renumbered by the ranks just scanned and written aside, since
  // the rebuild below resets the structure on its way (apss_components_repair.hpp)
  const bool carry = h->cc_on && h->ccr_max > 0;
  const int32_t cc_complete = h->cci.complete;
  const int64_t cc_resets = h->cci.resets;
  if (carry) {
    int32_t launches = 0;
    HIPCHK(h, begin_timed(h->stream, h->cr_ev0));
    APSS_TRY(components_stage(h, [&] { return cr_remap(h->cc, h->stream, n, h->dead.p, h->s_rowdst.p, &launches); }));
    HIPCHK(h, h->cr_ev1.record(h->stream));
  }
  int64_t live_rows = 0, live_nnz = 0;
  HIPCHK(h, hipMemcpyAsync(&live_rows, h->s_rowdst.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(&live_nnz, h->s_nnzdst.p + n, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (live_rows != n - marked || live_nnz < 0 || live_nnz > h->nnz) return fail(h, APSS_E_STATE, "apss_compact: the marks and their count disagree");
  APSS_TRY(ensure(h, h->in_rowptr, (size_t)live_rows + 1));
  APSS_TRY(ensure(h, h->in_ext, (size_t)std::max<int64_t>(live_rows, 1)));
  APSS_TRY(ensure(h, h->in_idx, (size_t)std::max<int64_t>(live_nnz, 1)));
  APSS_TRY(ensure(h, h->in_val, (size_t)std::max<int64_t>(live_nnz, 1)));
  RmGatherArgs g{};
  g.dead = h->dead.p;
  g.rowptr = h->rowptr.p;
  g.ext = h->ext.p;
  g.idx = h->idx.p;
  g.val = h->val.p;
  g.rows = n;
  g.row_dst = h->s_rowdst.p;
  g.nnz_dst = h->s_nnzdst.p;
  g.o_rowptr = h->in_rowptr.p;
  g.o_ext = h->in_ext.p;
  g.o_idx = h->in_idx.p;
  g.o_val = h->in_val.p;
  hipLaunchKernelGGL(k_rm_gather, dim3((unsigned)ceil_div(n * kRmWave, kRmThreads)), dim3(kRmThreads), 0, h->stream, g);
  HIPCHK(h, hipGetLastError());
  APSS_TRY(clear_impl(h));
  int64_t first = 0;
  h->stored_rows = true;
  const int32_t rc = insert_dev_impl(h, live_rows, live_nnz, h->in_rowptr.p, h->in_idx.p, h->in_val.p, h->in_ext.p, &first);
  h->stored_rows = false;
  APSS_TRY(rc);
  float ms = 0.f;
  HIPCHK(h, end_timed_read(h->stream, h->rm_ev0, h->rm_ev1, {}, &ms));
  h->ri.compact_ms = ms;
  h->ri.compacted_rows = marked;
  ++h->ri.compactions;
  if (h->cc_on && !carry) reset_components(h, true);  // (the slots shifted: clear_impl emptied the structure, the insert made it incomplete)
  if (carry) {  // the renumbered forest and its unions word become the structure of the rebuilt store: as complete as it was
    APSS_TRY(components_stage(h, [&] { return cr_install(h->cc, h->stream, live_rows); }));
    h->cci.complete = cc_complete || live_rows == 0;
    h->cci.resets = cc_resets;
    float remap_ms = 0.f;
    if (hipEventElapsedTime(&remap_ms, h->cr_ev0, h->cr_ev1) == hipSuccess) h->ccri.remap_ms = remap_ms;  // (the stream has been waited for)
    ++h->ccri.remaps;
  }
  return APSS_OK;
}

// apss_set_auto_compact: at the start of an insert-type call, BEFORE its batch is staged (the compaction gathers into the staging)
int32_t auto_compact(apss_handle *h) {
  if (!(h->auto_compact > 0.0) || h->rm_marked <= 0 || !((double)h->rm_marked > h->auto_compact * (double)h->n_rows)) return APSS_OK;
  return compact_impl(h);
}

// apss_query_stored, step 1: the live stored rows that d_ids[0, n) (device, n > 0) name -- the sorted list looked up per slot, the
// keep flags and entry counts scanned into destinations, the id counters (apss_query_stored.hpp).  Ends in the ONE readback
// between selection and gather: the two scan totals and the id counts
int32_t select_stored_rows(apss_handle *h, int64_t n, const int64_t *d_ids, int64_t *sel_rows, int64_t *sel_nnz) {
  const int64_t rows = h->n_rows;
  if (h->rm_marked > 0) APSS_TRY(rm_extend(h));
  APSS_TRY(ensure(h, h->qs_found, (size_t)n));
  APSS_TRY(ensure(h, h->qs_ctr, 2));
  if (rows > 0)
    for (DevBuf<int64_t> *b : {&h->s_keep, &h->s_cnt, &h->s_rowdst, &h->s_nnzdst}) APSS_TRY(ensure(h, *b, (size_t)rows + 1));
  APSS_TRY(sort_ids(h, d_ids, n, h->qs_ev[0]));
  HIPCHK(h, hipMemsetAsync(h->qs_found.p, 0, (size_t)n, h->stream));
  HIPCHK(h, hipMemsetAsync(h->qs_ctr.p, 0, 2 * sizeof(unsigned long long), h->stream));
  if (rows > 0) {
    QsSelectArgs s{};
    s.ext = h->ext.p;
    s.rowptr = h->rowptr.p;
    s.rows = rows;
    s.dead = h->rm_marked > 0 ? h->dead.p : nullptr;  // (nothing marked: nothing of the map is read)
    s.ids = h->rm_sorted.p;
    s.n_ids = n;
    s.found = h->qs_found.p;
    s.keep = h->s_keep.p;
    s.cnt = h->s_cnt.p;
    const int64_t blocks = ceil_div(ceil_div(rows, 2), kQsThreads);
    hipLaunchKernelGGL(k_qs_select, dim3((unsigned)std::min<int64_t>(blocks, rm_grid_cap(h, 4096))), dim3(kQsThreads), 0, h->stream, s);
    HIPCHK(h, hipGetLastError());
    ++h->qsi.launches;
    APSS_TRY(scan_i64(h, (const int64_t *)h->s_keep.p, h->s_rowdst.p, rows));
    APSS_TRY(scan_i64(h, (const int64_t *)h->s_cnt.p, h->s_nnzdst.p, rows));
  }
  hipLaunchKernelGGL(k_qs_ids, dim3((unsigned)std::min<int64_t>(ceil_div(n, kQsThreads), rm_grid_cap(h, 4096))), dim3(kQsThreads), 0, h->stream,
                     (const int64_t *)h->rm_sorted.p, n, (const uint8_t *)h->qs_found.p, h->qs_ctr.p);
  HIPCHK(h, hipGetLastError());
  ++h->qsi.launches;
  int64_t *back = h->scalars->stored_back;
  back[0] = back[1] = 0;
  const size_t total = rows > 0 ? sizeof(int64_t) : 0;
  float ms = 0.f;  // (the wait: the caller's id array may be reused from here on)
  HIPCHK(h, end_timed_read(h->stream, h->qs_ev[0], h->qs_ev[1], {{&back[0], h->s_rowdst.p + rows, total}, {&back[1], h->s_nnzdst.p + rows, total},
                                                       {&back[2], h->qs_ctr.p, 2 * sizeof(unsigned long long)}}, &ms));
  *sel_rows = back[0];
  *sel_nnz = back[1];
  h->qsi.ids_distinct = back[2];
  h->qsi.ids_missing = back[3];
  h->qsi.select_ms = ms;
  if (*sel_rows < 0 || *sel_rows > rows || *sel_nnz < 0 || *sel_nnz > h->nnz) return fail(h, APSS_E_STATE, "apss_query_stored: the selection and the store disagree");
  return APSS_OK;
}

// ... step 2: the selected rows, gathered into the query staging exactly as they are stored, with the batch summaries the probe
// plans with (k_qs_slots, k_qs_gather) and, on a handle with a dense-head block, their rows of the block
int32_t gather_stored_rows(apss_handle *h, int64_t sel_rows, int64_t sel_nnz) {
  const int64_t rows = h->n_rows;
  APSS_TRY(ensure(h, h->qs_slots, (size_t)sel_rows));
  APSS_TRY(ensure(h, h->q_rowptr, (size_t)sel_rows + 1));
  APSS_TRY(ensure(h, h->q_ext, (size_t)sel_rows));
  APSS_TRY(ensure(h, h->q_idx, (size_t)std::max<int64_t>(sel_nnz, 1)));
  APSS_TRY(ensure(h, h->q_val, (size_t)std::max<int64_t>(sel_nnz, 1)));
  APSS_TRY(ensure(h, h->flagword, 4));
  HIPCHK(h, begin_timed(h->stream, h->qs_ev[2]));
  HIPCHK(h, hipMemsetAsync(h->flagword.p, 0, 4 * sizeof(unsigned int), h->stream));
  hipLaunchKernelGGL(k_qs_slots, dim3((unsigned)std::min<int64_t>(ceil_div(rows, kQsThreads), rm_grid_cap(h, 4096))), dim3(kQsThreads), 0, h->stream,
                     (const int64_t *)h->s_keep.p, (const int64_t *)h->s_rowdst.p, rows, h->qs_slots.p);
  HIPCHK(h, hipGetLastError());
  QsGatherArgs g{};
  g.slots = h->qs_slots.p;
  g.n_sel = sel_rows;
  g.rowptr = h->rowptr.p;
  g.ext = h->ext.p;
  g.idx = h->idx.p;
  g.val = h->val.p;
  g.nnz_dst = h->s_nnzdst.p;
  g.o_rowptr = h->q_rowptr.p;
  g.o_ext = h->q_ext.p;
  g.o_idx = h->q_idx.p;
  g.o_val = h->q_val.p;
  g.flags_out = h->flagword.p;
  // (one wave per SELECTED row: the grid does not know how many rows are stored)
  hipLaunchKernelGGL(k_qs_gather, dim3((unsigned)ceil_div(sel_rows * kQsWave, kQsThreads)), dim3(kQsThreads), 0, h->stream, g);
  HIPCHK(h, hipGetLastError());
  h->qsi.launches += 2;
  // the batch summaries: the probe plans on the host with them, before its first launch
  unsigned int *flags_host = h->scalars->ingest_flags;
  float ms = 0.f;
  HIPCHK(h, end_timed_read(h->stream, h->qs_ev[2], h->qs_ev[3], {{flags_host, h->flagword.p, 4 * sizeof(unsigned int)}}, &ms));
  h->qsi.gather_ms = ms;
  APSS_TRY(take_ingest_flags(h, flags_host, false));
  // the batch's rows of the dense-head block and its tail ratios, as query_dev_impl packs them
  if (h->head_k && !h->sharded) APSS_TRY(pack_query_head(h, h->q_rowptr.p, h->q_idx.p, h->q_val.p, sel_rows));
  return APSS_OK;
}

// ... step 3: the rows the handle's scan arrays select -- whoever wrote them: k_qs_select for an id list, k_cr_detach for the
// components a removal touched -- become the staged query batch and are probed with their slot list
int32_t probe_selected_rows(apss_handle *h, int64_t sel_rows, int64_t sel_nnz, bool absorb_only, int64_t *n_results) {
  h->q_nonneg = true;
  h->q_max_nnz = 0;
  h->q_max_norm2 = 0.f;
  if (sel_rows > 0) APSS_TRY(gather_stored_rows(h, sel_rows, sel_nnz));
  // (qs_slots: the slot of every selected row -- what the components stage maps the batch's rows with)
  return probe(h, QueryBatch{{sel_rows, h->q_rowptr.p, h->q_idx.p, h->q_val.p, h->q_ext.p}, -1, h->q_max_nnz, h->q_max_norm2, sel_nnz,
                             sel_rows > 0 ? h->qs_slots.p : nullptr, absorb_only}, n_results);
}

// apss_query_stored: the live stored rows named by d_ids[0, n) (device) become the staged query batch -- selected, scanned and
// gathered on the device (apss_query_stored.hpp), never through ingest: they were normalised, pruned and admitted when they came
// in -- and the batch is probed as the outside batch apss_query_dev would stage from the same rows.
int32_t query_stored_impl(apss_handle *h, int64_t n, const int64_t *d_ids, int64_t *n_rows, int64_t *n_results) {
  // a query-type call: the last results and query batch are gone from here on (the staging is rewritten), also when it fails
  forget_last_call(h);
  h->qsi = apss_stored_query_info{};
  h->qsi.ids_given = n;
  int64_t sel_rows = 0, sel_nnz = 0;
  if (n > 0) APSS_TRY(select_stored_rows(h, n, d_ids, &sel_rows, &sel_nnz));
  h->qsi.rows_selected = sel_rows;
  h->qsi.nnz_selected = sel_nnz;
  if (n_rows) *n_rows = sel_rows;
  return probe_selected_rows(h, sel_rows, sel_nnz, false, n_results);
}

// The components a removal touched, taken apart and re-joined (apss_components_repair.hpp; include/apss.h: "with the repair on").
// Runs behind k_rm_mark with `marked` > 0 rows newly marked, the repair and the components on.  A failure leaves the caller to
// reset the structure.
int32_t repair_components(apss_handle *h, int64_t marked) {
  apss_components_repair_info &ri = h->ccri;
  const int64_t rows = h->n_rows;
  ri.declined = APSS_CCR_RAN;
  for (DevBuf<int64_t> *b : {&h->s_keep, &h->s_cnt, &h->s_rowdst, &h->s_nnzdst}) APSS_TRY(ensure(h, *b, (size_t)rows + 1));
  APSS_TRY(ensure(h, h->qs_ctr, 2));
  HIPCHK(h, hipMemsetAsync(h->qs_ctr.p, 0, 2 * sizeof(unsigned long long), h->stream));
  HIPCHK(h, begin_timed(h->stream, h->cr_ev0));
  APSS_TRY(run_stage(h, "components repair", h->cc.mem, [&](const char **) {
    return cr_detach_select(h->cc, h->stream, rows, h->dead.p, h->rowptr.p, h->s_keep.p, h->s_cnt.p, h->qs_ctr.p, &ri.launches);
  }));
  APSS_TRY(scan_i64(h, (const int64_t *)h->s_keep.p, h->s_rowdst.p, rows, &ri.launches));
  APSS_TRY(scan_i64(h, (const int64_t *)h->s_cnt.p, h->s_nnzdst.p, rows, &ri.launches));
  // the ONE readback between detach and gather: the two scan totals (the rows to re-join, their entries) and the flagged roots
  int64_t *back = h->scalars->stored_back;
  float ms = 0.f;
  HIPCHK(h, end_timed_read(h->stream, h->cr_ev0, h->cr_ev1, {{&back[0], h->s_rowdst.p + rows, sizeof(int64_t)}, {&back[1], h->s_nnzdst.p + rows, sizeof(int64_t)},
                                                       {&back[2], h->qs_ctr.p, sizeof(unsigned long long)}}, &ms));
  ri.detach_ms = ms;
  const int64_t sel_rows = back[0], sel_nnz = back[1];
  // (every row marked by an earlier call is a singleton that flagged itself: the others are the components this call touched)
  ri.components_touched = back[2] - (h->rm_marked - marked);
  if (sel_rows < 0 || sel_rows > rows - h->rm_marked || sel_nnz < 0 || sel_nnz > h->nnz || ri.components_touched < 0)
    return fail(h, APSS_E_STATE, "components repair: the selection and the store disagree");
  if (sel_rows > h->ccr_max) {  // today's rule: a remove never costs more than the caller allowed
    ri.declined = APSS_CCR_BUDGET;
    ++ri.budget_resets;
    reset_components(h, true);
    return APSS_OK;
  }
  ++ri.repairs;
  if (sel_rows == 0) return APSS_OK;  // (the marked rows were singletons: the last call's results stay)
  ri.rows_rejoined = sel_rows;
  // the re-join is a probe of the selected rows: the last results and query batch are gone from here on, also when it fails
  forget_last_call(h);
  h->qsi = apss_stored_query_info{};
  h->qsi.rows_selected = sel_rows;
  h->qsi.nnz_selected = sel_nnz;
  HIPCHK(h, begin_timed(h->stream, h->cr_ev0));
  const int32_t rc = probe_selected_rows(h, sel_rows, sel_nnz, true, nullptr);  // (no per-query or global cut: the forest alone wants the list)
  forget_last_call(h);  // (its list went into the forest; nobody asked for it)
  APSS_TRY(rc);
  HIPCHK(h, end_timed_read(h->stream, h->cr_ev0, h->cr_ev1, {}, &ms));
  ri.rejoin_ms = ms;
  ri.launches += h->qsi.launches;
  ri.pairs_rejoined = h->cci.pairs_absorbed;
  if (h->cci.declined != APSS_CC_RAN) return fail(h, APSS_E_STATE, "components repair: the re-join's list was not absorbed");
  return APSS_OK;
}

int32_t check_stored_query(apss_handle *h, const char *what, int64_t n, const int64_t *ids, int64_t *n_rows, int64_t *n_results) {
  if (n_rows) *n_rows = 0;
  if (n_results) *n_results = 0;
  if (h->sharded) return fail(h, APSS_E_UNSUPPORTED, std::string(what) + ": not on a term shard (it holds slices of rows; a query batch needs whole ones)");
  if (n < 0 || (n > 0 && !ids)) return fail(h, APSS_E_INVALID, std::string(what) + ": n >= 0 ids");
  if (n > 0x7fffffffLL) return fail(h, APSS_E_INVALID, std::string(what) + ": more than 2^31 - 1 ids in one call");
  return APSS_OK;
}

}  // namespace

// =====================================================================================================
extern "C" {

int32_t apss_create(const apss_config *cfg, apss_handle **out) {
  if (!cfg || !out) {
    g_create_error = "null argument";
    return APSS_E_INVALID;
  }
  *out = nullptr;
  if (cfg->struct_size != (int32_t)sizeof(apss_config)) {
    g_create_error = "apss_config.struct_size mismatch";
    return APSS_E_INVALID;
  }
  if (cfg->dim <= 0 || !std::isfinite(cfg->theta)) {
    g_create_error = "dim must be > 0 and theta finite";
    return APSS_E_INVALID;
  }
  apss_handle *h = new (std::nothrow) apss_handle();
  if (!h) return APSS_E_NOMEM;
  h->cfg = *cfg;
  h->dbgcfg = parse_debug_env();
  if (h->cfg.term_hi == 0 && h->cfg.term_lo == 0) h->cfg.term_hi = cfg->dim;
  if (h->cfg.term_lo < 0 || h->cfg.term_hi > cfg->dim || h->cfg.term_lo >= h->cfg.term_hi) {
    g_create_error = "bad term range";
    delete h;
    return APSS_E_INVALID;
  }
  h->sharded = !(h->cfg.term_lo == 0 && h->cfg.term_hi == cfg->dim);
  // term-range shards use the coarse filter too (measured T=2: 130 ms vs 195 ms per shard with the single-pass kernel);
  // their survivors are the shard's candidates, scored exactly in phase 2.  APSS_SHARD_EXACT=1: single-pass kernel.
  h->use_coarse = !(cfg->flags & (APSS_FLAG_EXACT_ACCUM | APSS_FLAG_FORCE_GENERAL | APSS_FLAG_FORCE_SCAN)) &&
                  (!h->sharded || !h->dbgcfg.shard_exact);
  h->cb = cfg->tile_rows ? cfg->tile_rows : (cfg->theta > 0.0 ? 16384 : 8192);  // (theta <= 0: gen_block, two workgroups per CU)
  h->ex.cb = h->cb;
  h->ex.align = kSegAlign;
  h->cx.cb = std::min(2 * h->cb, 32768);
  if (h->dbgcfg.cx_tile) h->cx.cb = h->dbgcfg.cx_tile;  // experiment hook (multiple of 64, <= 65536)
  h->no_acc8 = h->dbgcfg.filter.no_acc8;
  if (h->dbgcfg.fold_w == 128 || h->dbgcfg.fold_w == 256) {  // experiment: two blocks
    h->head_exact = 256;
    h->head_fold_w = h->dbgcfg.fold_w;
  } else if (h->dbgcfg.mix >= 32 && h->dbgcfg.mix <= 224 && h->dbgcfg.mix % 32 == 0) {  // experiment: another split of the one block
    h->head_exact = h->dbgcfg.mix;
    h->head_fold_w = 256 - h->dbgcfg.mix;
  }
  h->cx.align = h->dbgcfg.seg_align == 16 ? 16 : kSegAlignC;
  h->cx.coarse = true;
  if (h->cb < 64 || h->cb > 32768 || (h->cb % 64)) {
    g_create_error = "tile_rows must be a multiple of 64 in [64, 32768]";
    delete h;
    return APSS_E_INVALID;
  }
  if (h->sharded && !(cfg->theta > 0.0)) {
    g_create_error = "term-range shards need theta > 0 (candidate test p_g >= theta*|q_g|*|c_g|)";
    delete h;
    return APSS_E_UNSUPPORTED;
  }
  h->dev = cfg->device_id;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0 || h->dev < 0 || h->dev >= ndev) {
    g_create_error = std::string("no usable HIP device (there is no CPU fallback): ") +
                     (e != hipSuccess ? hipGetErrorString(e) : "device ordinal out of range");
    delete h;
    return APSS_E_DEVICE;
  }
  if ((e = hipSetDevice(h->dev)) != hipSuccess || (e = h->own_stream.make()) != hipSuccess) {
    g_create_error = std::string("HIP init failed: ") + hipGetErrorString(e);
    delete h;
    return APSS_E_DEVICE;
  }
  h->stream = h->own_stream;
  (void)h->pin.grow(kGrowStage, kPinBytes + kPinScalars, 0, nullptr, nullptr);  // (without it: the unpacked copies)
  if (h->pin.p) h->scalars = new (h->pin.p + kPinBytes) PinScalars{};
  if (cfg->capacity_rows > 0) {
    if (ensure(h, h->rowptr, (size_t)cfg->capacity_rows + 1, 0, true) != APSS_OK ||
        ensure(h, h->ext, (size_t)cfg->capacity_rows, 0, true) != APSS_OK) {
      g_create_error = h->err;
      apss_destroy(h);
      return APSS_E_NOMEM;
    }
  }
  if (cfg->capacity_nnz > 0) {
    if (ensure(h, h->idx, (size_t)cfg->capacity_nnz, 0, true) != APSS_OK ||
        ensure(h, h->erow, (size_t)cfg->capacity_nnz, 0, true) != APSS_OK ||
        ensure(h, h->val, (size_t)cfg->capacity_nnz, 0, true) != APSS_OK ||
        (h->use_coarse ? ensure(h, h->cx.post_c, (size_t)cfg->capacity_nnz * 2 + 64, 0, true)
                       : ensure(h, h->ex.post, (size_t)cfg->capacity_nnz + (size_t)cfg->capacity_nnz / 2 + 64, 0, true)) != APSS_OK) {
      g_create_error = h->err;
      apss_destroy(h);
      return APSS_E_NOMEM;
    }
  }
  *out = h;
  return APSS_OK;
}

void apss_destroy(apss_handle *h) {
  if (!h) return;
  (void)hipSetDevice(h->dev);
  if (h->own_stream.made()) (void)hipStreamSynchronize(h->own_stream);
  delete h;
}

const char *apss_last_error(const apss_handle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int32_t apss_set_stream(apss_handle *h, void *hip_stream, int32_t use_own) {
  APSS_TRY(enter(h));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->stream = use_own ? h->own_stream : (hipStream_t)hip_stream;  // NULL is the device's default stream
  return APSS_OK;
}

int32_t apss_insert(apss_handle *h, int64_t n, const int64_t *rowptr, const int32_t *indices, const double *values,
                    const int64_t *ext_ids) {
  APSS_TRY(enter(h));
  APSS_TRY(validate_host_csr(h, n, rowptr, indices, values, ext_ids));
  APSS_TRY(auto_compact(h));
  if (n == 0) return APSS_OK;
  APSS_TRY(upload(h, n, rowptr, indices, values, ext_ids));
  int64_t first = 0;
  return insert_dev_impl(h, n, rowptr[n], h->up_rowptr, h->up_idx, h->in_val.p, h->up_ext, &first);
}

int32_t apss_query(apss_handle *h, int64_t n, const int64_t *rowptr, const int32_t *indices, const double *values,
                   const int64_t *ext_ids, int64_t *n_results) {
  APSS_TRY(enter(h));
  APSS_TRY(validate_host_csr(h, n, rowptr, indices, values, ext_ids));
  APSS_TRY(upload(h, n, rowptr, indices, values, ext_ids));
  return query_dev_impl(h, n, n ? rowptr[n] : 0, h->up_rowptr, h->up_idx, h->in_val.p, h->up_ext, n_results);
}

int32_t apss_insert_and_query(apss_handle *h, int64_t n, const int64_t *rowptr, const int32_t *indices,
                              const double *values, const int64_t *ext_ids, int64_t *n_results) {
  APSS_TRY(enter(h));
  APSS_TRY(validate_host_csr(h, n, rowptr, indices, values, ext_ids));
  APSS_TRY(auto_compact(h));  // (before the batch is staged; the _dev entry below then finds nothing over the fraction)
  APSS_TRY(upload(h, n, rowptr, indices, values, ext_ids));
  return apss_insert_and_query_dev(h, n, n ? rowptr[n] : 0, h->up_rowptr, h->up_idx, h->in_val.p, h->up_ext, n_results);
}

int32_t apss_self_join(apss_handle *h, int64_t *n_results) {
  APSS_TRY(enter(h));
  if (h->idx_rows < h->n_rows) APSS_TRY(build_index(h, h->idx_rows));  // a self-join runs over the index: fold the tail in
  if (!h->cc_on) return probe(h, store_batch(h), n_results);
  // the components of the join: the call's list is every edge there is, so the structure starts over and ends complete -- unless
  // the probe cut its rounds (APSS_CC_TILE_CUT), which leaves singletons
  reset_components(h, false);
  const int32_t rc = probe(h, store_batch(h), n_results);
  if (rc == APSS_OK && h->cci.declined == APSS_CC_RAN) h->cci.complete = 1;
  else if (rc == APSS_OK) reset_components(h, false);
  return rc;
}

int32_t apss_result_count(const apss_handle *h, int64_t *n_results) {
  if (!h || !n_results) return APSS_E_INVALID;
  if (h->n_res < 0) return APSS_E_STATE;
  *n_results = h->n_res;
  return APSS_OK;
}

__global__ void k_gather_ids(const int32_t *res_q, const int32_t *res_c, const int64_t *q_ext, const int64_t *c_ext,
                             int64_t n, int64_t *out_q, int64_t *out_c) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    out_q[i] = q_ext[res_q[i]];
    out_c[i] = c_ext[res_c[i]];
  }
}

int32_t apss_fetch_results(apss_handle *h, int64_t offset, int64_t count, int64_t *out_q, int64_t *out_c,
                           float *out_score) {
  APSS_TRY(enter(h));
  if (h->n_res < 0) return fail(h, APSS_E_STATE, "no query has run on this handle");
  if (offset < 0 || count < 0 || offset + count > h->n_res) return fail(h, APSS_E_INVALID, "fetch range out of bounds");
  if (count == 0) return APSS_OK;
  if (!out_q || !out_c || !out_score) return fail(h, APSS_E_INVALID, "null output buffer");
  // map (query row, candidate slot) to external ids on the device, then copy out
  if (h->pin.p && (size_t)count * 20 <= kPinBytes) {  // a small answer: one packed copy into pinned memory
    APSS_TRY(ensure(h, h->pack, kPinBytes));
    int64_t *pq = reinterpret_cast<int64_t *>(h->pack.p), *pc = pq + count;
    float *ps = reinterpret_cast<float *>(pc + count);
    hipLaunchKernelGGL(k_gather_ids, dim3((unsigned)ceil_div(count, 256)), dim3(256), 0, h->stream, h->out_q + offset, h->out_c + offset,
                       h->res_q_ext, (const int64_t *)h->ext.p, count, pq, pc);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(ps, h->out_s + offset, (size_t)count * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->pin.p, h->pack.p, (size_t)count * 20, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::memcpy(out_q, h->pin.p, (size_t)count * sizeof(int64_t));
    std::memcpy(out_c, h->pin.p + (size_t)count * sizeof(int64_t), (size_t)count * sizeof(int64_t));
    std::memcpy(out_score, h->pin.p + (size_t)count * 2 * sizeof(int64_t), (size_t)count * sizeof(float));
    return APSS_OK;
  }
  APSS_TRY(ensure(h, h->s_rowdst, (size_t)count));
  APSS_TRY(ensure(h, h->s_nnzdst, (size_t)count));
  hipLaunchKernelGGL(k_gather_ids, dim3((unsigned)ceil_div(count, 256)), dim3(256), 0, h->stream,
                     h->out_q + offset, h->out_c + offset, h->res_q_ext,
                     (const int64_t *)h->ext.p, count, h->s_rowdst.p, h->s_nnzdst.p);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipMemcpyAsync(out_q, h->s_rowdst.p, (size_t)count * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(out_c, h->s_nnzdst.p, (size_t)count * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(out_score, h->out_s + offset, (size_t)count * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return APSS_OK;
}

int32_t apss_size(const apss_handle *h, int64_t *rows, int64_t *nnz) {
  if (!h) return APSS_E_INVALID;
  if (rows) *rows = h->n_rows;
  if (nnz) *nnz = h->nnz;
  return APSS_OK;
}

int32_t apss_stats_get(apss_handle *h, apss_stats *out) {
  if (!h || !out) return APSS_E_INVALID;
  h->st.rows = h->n_rows;
  h->st.nnz = h->nnz;
  h->st.tiles = h->use_coarse && h->ex_built_rows < h->idx_rows ? h->cx.n_tiles : ceil_div(h->idx_rows, h->ex.cb);
  h->st.hbm_bytes = (int64_t)h->bytes_reserved;
  h->st.downgrades = h->downgrades;
  h->st.head_terms = h->head_k ? (int64_t)h->head_terms.size() : 0;  // (as they are now: a policy handle is asked after its insert)
  h->st.head_columns = (uint32_t)h->head_k;
  // the caller says how large ITS apss_stats is: an older caller's shorter struct gets the fields it knows, nothing beyond
  const int32_t caller = out->struct_size;
  if (caller < (int32_t)(2 * sizeof(int32_t)) || caller > (1 << 16))
    return fail(h, APSS_E_INVALID, "apss_stats.struct_size must be set to sizeof(apss_stats) before the call");
  const int32_t n = std::min<int32_t>(caller, (int32_t)sizeof(apss_stats));
  h->st.struct_size = n;
  std::memcpy(out, &h->st, (size_t)n);
  return APSS_OK;
}

int32_t apss_insert_dev(apss_handle *h, int64_t n, int64_t nnz, const int64_t *d_rowptr, const int32_t *d_indices,
                        const float *d_values, const int64_t *d_ext_ids) {
  APSS_TRY(enter(h));
  if (n < 0 || nnz < 0) return fail(h, APSS_E_INVALID, "negative size");
  if (n > 0 && (!d_rowptr || !d_ext_ids || (nnz > 0 && (!d_indices || !d_values))))
    return fail(h, APSS_E_INVALID, "null device pointer");
  APSS_TRY(auto_compact(h));
  int64_t first = 0;
  return insert_dev_impl(h, n, nnz, d_rowptr, d_indices, d_values, d_ext_ids, &first);
}

int32_t apss_insert_stored_dev(apss_handle *h, int64_t n, int64_t nnz, const int64_t *d_rowptr, const int32_t *d_indices,
                               const float *d_values, const int64_t *d_ext_ids) {
  APSS_TRY(enter(h));
  if (n < 0 || nnz < 0) return fail(h, APSS_E_INVALID, "negative size");
  if (n > 0 && (!d_rowptr || !d_ext_ids || (nnz > 0 && (!d_indices || !d_values))))
    return fail(h, APSS_E_INVALID, "null device pointer");
  APSS_TRY(auto_compact(h));
  int64_t first = 0;
  h->stored_rows = true;
  const int32_t rc = insert_dev_impl(h, n, nnz, d_rowptr, d_indices, d_values, d_ext_ids, &first);
  h->stored_rows = false;
  return rc;
}

int32_t apss_get_store_dev(apss_handle *h, const int64_t **d_rowptr, const int32_t **d_indices, const float **d_values, int64_t *rows,
                       int64_t *nnz) {
  if (!h) return APSS_E_INVALID;
  const bool any = h->n_rows > 0;
  if (d_rowptr) *d_rowptr = any ? h->rowptr.p : nullptr;
  if (d_indices) *d_indices = any ? h->idx.p : nullptr;
  if (d_values) *d_values = any ? h->val.p : nullptr;
  if (rows) *rows = h->n_rows;
  if (nnz) *nnz = h->nnz;
  return APSS_OK;
}

// what the handle knows of one rendering, copied out: nothing is built, launched or reserved (include/apss.h)
int32_t apss_index_view_get(apss_handle *h, int32_t rendering, apss_index_view *out) {
  if (!h || !out || (rendering != 0 && rendering != 1)) return APSS_E_INVALID;
  const int32_t caller = out->struct_size;
  if (caller < (int32_t)(2 * sizeof(int32_t)) || caller > (1 << 16))
    return fail(h, APSS_E_INVALID, "apss_index_view.struct_size must be set to sizeof(apss_index_view) before the call");
  const apss_handle::IndexSet &ix = rendering ? h->cx : h->ex;
  // (the exact rendering of a handle that filters with the coarse one goes stale at an insert: ex_built_rows says how far it holds)
  const bool built = ix.n_tiles > 0 && ix.built_rows > 0 && (int64_t)ix.h_base.size() == ix.n_tiles + 1 &&
                     (rendering ? h->use_coarse : h->ex_built_rows == ix.built_rows);
  const bool scales = h->sharded || h->head_k > 0;
  apss_index_view v{};
  v.rendering = rendering;
  v.tile_rows = ix.cb;
  v.seg_align = ix.align;
  v.posting_bytes = ix.coarse ? (int32_t)sizeof(uint32_t) : (int32_t)sizeof(Posting);
  v.slot_form = !ix.coarse ? APSS_SLOT_PLAIN : (ix.cb <= 32768 ? APSS_SLOT_TIMES2 : (ix.cb > 65536 ? APSS_SLOT_WIDE : APSS_SLOT_PLAIN));
  v.weights_scaled = scales && ix.coarse ? 1 : 0;
  v.dim = h->cfg.dim;
  if (built) {
    v.n_tiles = ix.n_tiles;
    v.built_rows = ix.built_rows;
    v.post_used = ix.post_used;
    v.d_seg = ix.seg.p;
    v.d_base = ix.base.p;
    v.d_post = ix.coarse ? (const void *)ix.post_c.p : (const void *)ix.post.p;
    v.d_sub = scales ? h->sub.p : nullptr;
    v.d_tile_min = scales ? (ix.coarse ? h->tile_min_c.p : h->tile_min.p) : nullptr;
    v.max_seg = ix.max_seg;
    v.long_segs = ix.long_segs;
    v.chunk_weight = ix.round_chunks;
  }
  const int32_t n = std::min<int32_t>(caller, (int32_t)sizeof(apss_index_view));
  v.struct_size = n;
  std::memcpy(out, &v, (size_t)n);
  return APSS_OK;
}

int32_t apss_query_dev(apss_handle *h, int64_t n, int64_t nnz, const int64_t *d_rowptr, const int32_t *d_indices,
                       const float *d_values, const int64_t *d_ext_ids, int64_t *n_results) {
  APSS_TRY(enter(h));
  if (n < 0 || nnz < 0) return fail(h, APSS_E_INVALID, "negative size");
  if (n > 0 && (!d_rowptr || !d_ext_ids || (nnz > 0 && (!d_indices || !d_values))))
    return fail(h, APSS_E_INVALID, "null device pointer");
  return query_dev_impl(h, n, nnz, d_rowptr, d_indices, d_values, d_ext_ids, n_results);
}

int32_t apss_insert_and_query_dev(apss_handle *h, int64_t n, int64_t nnz, const int64_t *d_rowptr,
                                  const int32_t *d_indices, const float *d_values, const int64_t *d_ext_ids,
                                  int64_t *n_results) {
  APSS_TRY(enter(h));
  if (n < 0 || nnz < 0) return fail(h, APSS_E_INVALID, "negative size");
  if (n > 0 && (!d_rowptr || !d_ext_ids || (nnz > 0 && (!d_indices || !d_values))))
    return fail(h, APSS_E_INVALID, "null device pointer");
  APSS_TRY(auto_compact(h));
  int64_t first = 0;
  const int32_t cc_complete = h->cci.complete;
  APSS_TRY(insert_dev_impl(h, n, nnz, d_rowptr, d_indices, d_values, d_ext_ids, &first));
  // the batch is now rows [first, n_rows) of the store: query it in place (rowptr offsets are absolute)
  const int32_t rc = probe(h, store_batch(h).rows(first, h->n_rows), n_results);
  // (the call reported every pair between its rows and everything stored: the components are as complete as they were)
  if (h->cc_on && rc == APSS_OK && h->cci.declined == APSS_CC_RAN) h->cci.complete = cc_complete;
  return rc;
}

int32_t apss_clear(apss_handle *h) {
  APSS_TRY(enter(h));
  return clear_impl(h);
}

int32_t apss_set_head_terms(apss_handle *h, int32_t n_terms, const int32_t *terms, int32_t part, int32_t n_parts) {
  APSS_TRY(enter(h));
  if (h->n_rows != 0) return fail(h, APSS_E_STATE, "apss_set_head_terms: the handle holds vectors (set the block before the first insert or after apss_clear)");
  if (n_terms < 0 || n_terms > kHeadMaxTerms || (n_terms > 0 && !terms)) return fail(h, APSS_E_INVALID, "apss_set_head_terms: 0 .. 32768 terms");
  if (n_parts < 1 || part < 0 || part >= n_parts) return fail(h, APSS_E_INVALID, "apss_set_head_terms: part must be in [0, n_parts)");
  if (n_parts > 1 && !h->sharded)
    return fail(h, APSS_E_INVALID, "apss_set_head_terms: only a term shard multiplies a share of the block (n_parts > 1)");
  if (n_terms == 0) {
    h->head_fixed = false;
    h->head_k = 0;
    h->head_terms.clear();
    h->head_part = 0;
    h->head_parts = 1;
    return APSS_OK;
  }
  if (!h->use_coarse || !(h->cfg.theta > 0.0))
    return fail(h, APSS_E_UNSUPPORTED, "a dense-head block needs the two-pass join (theta > 0, no EXACT_ACCUM / FORCE_* flag)");
  if (h->sharded && (h->cfg.flags & APSS_FLAG_ADMISSION))
    return fail(h, APSS_E_UNSUPPORTED, "a term shard packs the block's rows from the batch row by row: not with APSS_FLAG_ADMISSION");
  if (!(h->dbgcfg.fold_w == 128 || h->dbgcfg.fold_w == 256) && !h->dbgcfg.mix) {  // (the experiments' geometry stays)
    h->head_fold_w = h->head_fold_user ? h->head_fold_user : 128;
    h->head_exact = 256 - h->head_fold_w;
  }
  std::vector<int32_t> pos((size_t)h->cfg.dim, -1);
  for (int32_t i = 0; i < n_terms; ++i) {
    if (terms[i] < 0 || terms[i] >= h->cfg.dim || pos[(size_t)terms[i]] >= 0)
      return fail(h, APSS_E_INVALID, "apss_set_head_terms: terms must be distinct and in [0, dim)");
    pos[(size_t)terms[i]] = head_column(i, h->head_fold_w, h->head_exact);
  }
  APSS_TRY(ensure(h, h->head_pos, (size_t)h->cfg.dim));
  HIPCHK(h, hipMemcpyAsync(h->head_pos.p, pos.data(), (size_t)h->cfg.dim * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->head_terms.assign(terms, terms + n_terms);
  h->head_k = head_width(n_terms, h->head_fold_w, h->head_exact, head_wants_i8(h));
  h->head_fixed = true;
  h->head_blocked = false;
  h->head_part = part;
  h->head_parts = n_parts;
  h->cx.n_tiles = 0;
  h->ex_built_rows = 0;
  return APSS_OK;
}

int32_t apss_set_head_fold(apss_handle *h, int32_t columns) {
  APSS_TRY(enter(h));
  if (columns != 0 && columns != 64 && columns != 128 && columns != 192) return fail(h, APSS_E_INVALID, "apss_set_head_fold: 0 (default: 128), 64, 128 or 192 columns");
  if (h->n_rows != 0) return fail(h, APSS_E_STATE, "apss_set_head_fold: on an empty handle (it takes effect at the next apss_set_head_terms)");
  h->head_fold_user = columns;
  return APSS_OK;
}

int32_t apss_get_head_terms(apss_handle *h, int32_t capacity, int32_t *out_terms, int32_t *n_terms) {
  if (!h || !n_terms) return APSS_E_INVALID;
  const int32_t n = h->head_k ? (int32_t)h->head_terms.size() : 0;
  *n_terms = n;
  if (out_terms)
    for (int32_t i = 0; i < std::min(n, capacity); ++i) out_terms[i] = h->head_terms[(size_t)i];
  return APSS_OK;
}

int32_t apss_set_top_k(apss_handle *h, int32_t k) {
  APSS_TRY(enter(h));
  // (a refusal is also left where apss_last_error(NULL) finds it: a wrapper that applies k right after apss_create and destroys
  // the handle when it is refused reports it as a failed create)
  if (k < 0 || k > APSS_TOP_K_MAX) return fail(h, APSS_E_INVALID, g_create_error = "apss_set_top_k: k must be in [0, 1024] (0: off)");
  if (k > 0 && h->sharded)
    return fail(h, APSS_E_UNSUPPORTED, g_create_error = "apss_set_top_k: a term shard reports candidates with partial scores; the group cuts behind its exchange");
  h->top_k = k;
  return APSS_OK;
}

int32_t apss_set_top_pairs(apss_handle *h, int64_t k_pairs) {
  if (!h) return APSS_E_INVALID;
  // (a refusal is left for apss_last_error(NULL) too, as apss_set_top_k's)
  if (k_pairs < 0 || k_pairs > APSS_TOP_PAIRS_MAX)
    return fail(h, APSS_E_INVALID, g_create_error = "apss_set_top_pairs: k_pairs must be in [0, 2^20] (0: off)");
  if (k_pairs > 0 && h->sharded)
    return fail(h, APSS_E_UNSUPPORTED, g_create_error = "apss_set_top_pairs: a term shard reports candidates with partial scores; it has no final list to cut");
  h->top_pairs = k_pairs;
  return APSS_OK;
}

int32_t apss_top_pairs_get(apss_handle *h, apss_top_pairs_info *out) {
  if (!h || !out) return APSS_E_INVALID;
  const int32_t caller = out->struct_size;
  if (caller < (int32_t)(2 * sizeof(int32_t)) || caller > (1 << 16))
    return fail(h, APSS_E_INVALID, "apss_top_pairs_info.struct_size must be set to sizeof(apss_top_pairs_info) before the call");
  const int32_t n = std::min<int32_t>(caller, (int32_t)sizeof(apss_top_pairs_info));
  h->tpi.struct_size = n;
  std::memcpy(out, &h->tpi, (size_t)n);
  return APSS_OK;
}

int32_t apss_set_components(apss_handle *h, int32_t on) {
  if (!h) return APSS_E_INVALID;
  // (a refusal is left for apss_last_error(NULL) too, as apss_set_top_k's)
  if (on != 0 && on != 1) return fail(h, APSS_E_INVALID, g_create_error = "apss_set_components: on must be 0 or 1");
  if (on && h->sharded)
    return fail(h, APSS_E_UNSUPPORTED, g_create_error = "apss_set_components: a term shard reports candidates with partial scores; it has no final list whose pairs are edges");
  if (!on) {
    if (h->cc_on) {
      APSS_TRY(enter(h));
      HIPCHK(h, hipStreamSynchronize(h->stream));  // (a hook may still be running on the arrays)
      h->cc = CcWork{};  // (its arrays take their bytes off the reservation as they go)
    }
    h->cc_on = false;
    const int64_t resets = h->cci.resets;
    h->cci = apss_components_info{};
    h->cci.resets = resets;
    return APSS_OK;
  }
  h->cc_on = true;
  h->cci.on = 1;
  h->cci.declined = APSS_CC_RAN;
  reset_components(h, false);
  return APSS_OK;
}

int32_t apss_components_get(apss_handle *h, apss_components_info *out) {
  if (!h || !out) return APSS_E_INVALID;
  const int32_t caller = out->struct_size;
  if (caller < (int32_t)(2 * sizeof(int32_t)) || caller > (1 << 16))
    return fail(h, APSS_E_INVALID, "apss_components_info.struct_size must be set to sizeof(apss_components_info) before the call");
  if (h->cc_on) {
    APSS_TRY(enter(h));
    APSS_TRY(label_components(h));
  } else {
    h->cci.declined = APSS_CC_OFF;
  }
  const int32_t n = std::min<int32_t>(caller, (int32_t)sizeof(apss_components_info));
  h->cci.struct_size = n;
  std::memcpy(out, &h->cci, (size_t)n);
  return APSS_OK;
}

int32_t apss_components_dev(apss_handle *h, const int32_t **d_label, int64_t *rows) {
  APSS_TRY(enter(h));
  if (!h->cc_on) return fail(h, APSS_E_STATE, "apss_components_dev: the setting is off (apss_set_components)");
  APSS_TRY(label_components(h));
  if (d_label) *d_label = h->n_rows > 0 ? h->cc.label.p : nullptr;
  if (rows) *rows = h->n_rows;
  return APSS_OK;
}

int32_t apss_components_fetch(apss_handle *h, int64_t offset, int64_t count, int32_t *out_label, int64_t *out_rep_ext) {
  APSS_TRY(enter(h));
  if (!h->cc_on) return fail(h, APSS_E_STATE, "apss_components_fetch: the setting is off (apss_set_components)");
  if (offset < 0 || count < 0 || offset > h->n_rows || count > h->n_rows - offset) return fail(h, APSS_E_INVALID, "apss_components_fetch: a range outside [0, rows]");
  APSS_TRY(label_components(h));
  if (count == 0 || (!out_label && !out_rep_ext)) return APSS_OK;
  if (out_rep_ext) {  // the ids are gathered through the handle's small staging buffer, a piece at a time (stream order keeps the pieces apart)
    APSS_TRY(ensure(h, h->pack, kPinBytes));
    const int64_t piece = (int64_t)(kPinBytes / sizeof(int64_t));
    for (int64_t at = 0; at < count; at += piece) {
      const int64_t n = std::min(piece, count - at);
      hipLaunchKernelGGL(k_cc_rep, dim3(cc_grid(n, kCcGridCap)), dim3(kCcThreads), 0, h->stream, (const int32_t *)h->cc.label.p, (const int64_t *)h->ext.p,
                         offset + at, n, h->n_rows, reinterpret_cast<int64_t *>(h->pack.p));
      HIPCHK(h, hipGetLastError());
      HIPCHK(h, hipMemcpyAsync(out_rep_ext + at, h->pack.p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    }
  }
  if (out_label) HIPCHK(h, hipMemcpyAsync(out_label, h->cc.label.p + offset, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return APSS_OK;
}

int32_t apss_set_components_repair(apss_handle *h, int64_t max_rows) {
  if (!h) return APSS_E_INVALID;
  // (a refusal is left for apss_last_error(NULL) too, as apss_set_top_k's)
  if (h->sharded)
    return fail(h, APSS_E_UNSUPPORTED, g_create_error = "apss_set_components_repair: a term shard keeps no components (apss_set_components) to repair");
  if (max_rows < 0 || max_rows > 0x7fffffffLL)
    return fail(h, APSS_E_INVALID, g_create_error = "apss_set_components_repair: max_rows must be in [0, 2^31 - 1] (0: off)");
  h->ccr_max = max_rows;
  return APSS_OK;
}

int32_t apss_components_repair_get(apss_handle *h, apss_components_repair_info *out) {
  if (!h || !out) return APSS_E_INVALID;
  const int32_t caller = out->struct_size;
  if (caller < (int32_t)(2 * sizeof(int32_t)) || caller > (1 << 16))
    return fail(h, APSS_E_INVALID, "apss_components_repair_info.struct_size must be set to sizeof(apss_components_repair_info) before the call");
  const int32_t n = std::min<int32_t>(caller, (int32_t)sizeof(apss_components_repair_info));
  apss_components_repair_info ri = h->ccri;  // (what the last remove left is the handle's; the answer is a copy)
  ri.struct_size = n;
  ri.max_rows = h->ccr_max;
  // no remove has marked a row yet, or the last one marked none: `declined` says why a remove would not repair NOW (include/apss.h)
  if (ri.rows_marked == 0) ri.declined = h->ccr_max <= 0 ? APSS_CCR_OFF : !h->cc_on ? APSS_CCR_NO_COMPONENTS : APSS_CCR_NOTHING;
  std::memcpy(out, &ri, (size_t)n);
  return APSS_OK;
}

int32_t apss_set_top_k_window(apss_handle *h, int64_t max_pairs) {
  if (!h) return APSS_E_INVALID;
  // (a refusal is left for apss_last_error(NULL) too, as apss_set_top_k's)
  if (max_pairs < 0) return fail(h, APSS_E_INVALID, g_create_error = "apss_set_top_k_window: max_pairs must be >= 0 (0: off)");
  if (max_pairs > 0 && h->sharded)
    return fail(h, APSS_E_UNSUPPORTED, g_create_error = "apss_set_top_k_window: a term shard reports candidates with partial scores; it has no per-query top-k to window");
  h->top_k_window = max_pairs;
  return APSS_OK;
}

int32_t apss_set_top_k_tile_cut(apss_handle *h, int32_t on) {
  if (!h) return APSS_E_INVALID;
  // (a refusal is left for apss_last_error(NULL) too, as apss_set_top_k's)
  if (on != 0 && on != 1) return fail(h, APSS_E_INVALID, g_create_error = "apss_set_top_k_tile_cut: 0 (off) or 1");
  if (on && h->sharded)
    return fail(h, APSS_E_UNSUPPORTED, g_create_error = "apss_set_top_k_tile_cut: a term shard reports candidates with partial scores; it has no per-query top-k to cut for");
  h->tile_cut = on != 0;
  return APSS_OK;
}

int32_t apss_topk_tile_cut_get(apss_handle *h, apss_topk_tile_cut_info *out) {
  if (!h || !out) return APSS_E_INVALID;
  const int32_t caller = out->struct_size;
  if (caller < (int32_t)(2 * sizeof(int32_t)) || caller > (1 << 16))
    return fail(h, APSS_E_INVALID, "apss_topk_tile_cut_info.struct_size must be set to sizeof(apss_topk_tile_cut_info) before the call");
  const int32_t n = std::min<int32_t>(caller, (int32_t)sizeof(apss_topk_tile_cut_info));
  h->tci.struct_size = n;
  std::memcpy(out, &h->tci, (size_t)n);
  return APSS_OK;
}

int32_t apss_remove(apss_handle *h, int64_t n, const int64_t *ext_ids, int64_t *n_rows_removed) {
  APSS_TRY(enter(h));
  if (n_rows_removed) *n_rows_removed = 0;
  if (h->sharded) return refuse_shard_removal(h, "apss_remove");
  if (n < 0 || (n > 0 && !ext_ids)) return fail(h, APSS_E_INVALID, "apss_remove: n >= 0 ids");
  begin_repair_call(h);
  if (n == 0 || h->n_rows == 0) return APSS_OK;
  APSS_TRY(ensure(h, h->rm_ids, (size_t)n));
  HIPCHK(h, hipMemcpyAsync(h->rm_ids.p, ext_ids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  int64_t newly = 0;
  APSS_TRY(remove_impl(h, n, h->rm_ids.p, &newly));  // (synchronises: the caller's array may be reused on return)
  if (n_rows_removed) *n_rows_removed = newly;
  return APSS_OK;
}

int32_t apss_remove_dev(apss_handle *h, int64_t n, const int64_t *d_ext_ids, int64_t *n_rows_removed) {
  APSS_TRY(enter(h));
  if (n_rows_removed) *n_rows_removed = 0;
  if (h->sharded) return refuse_shard_removal(h, "apss_remove_dev");
  if (n < 0 || (n > 0 && !d_ext_ids)) return fail(h, APSS_E_INVALID, "apss_remove_dev: n >= 0 ids");
  begin_repair_call(h);
  int64_t newly = 0;
  APSS_TRY(remove_impl(h, n, d_ext_ids, &newly));
  if (n_rows_removed) *n_rows_removed = newly;
  return APSS_OK;
}

int32_t apss_compact(apss_handle *h) {
  APSS_TRY(enter(h));
  if (h->sharded) return refuse_shard_removal(h, "apss_compact");
  return compact_impl(h);
}

int32_t apss_set_auto_compact(apss_handle *h, double fraction) {
  if (!h) return APSS_E_INVALID;
  if (h->sharded) return refuse_shard_removal(h, "apss_set_auto_compact");
  if (!(fraction >= 0.0 && fraction < 1.0)) return fail(h, APSS_E_INVALID, "apss_set_auto_compact: the fraction must be in [0, 1) (0: off)");
  h->auto_compact = fraction;
  return APSS_OK;
}

int32_t apss_removal_get(apss_handle *h, apss_removal_info *out) {
  if (!h || !out) return APSS_E_INVALID;
  if (h->sharded) return refuse_shard_removal(h, "apss_removal_get");
  const int32_t caller = out->struct_size;
  if (caller < (int32_t)(2 * sizeof(int32_t)) || caller > (1 << 16))
    return fail(h, APSS_E_INVALID, "apss_removal_info.struct_size must be set to sizeof(apss_removal_info) before the call");
  const int32_t n = std::min<int32_t>(caller, (int32_t)sizeof(apss_removal_info));
  h->ri.struct_size = n;
  h->ri.rows_removed = h->rm_marked;
  h->ri.rows_live = h->n_rows - h->rm_marked;
  h->ri.auto_compact = h->auto_compact;
  std::memcpy(out, &h->ri, (size_t)n);
  return APSS_OK;
}

int32_t apss_query_stored(apss_handle *h, int64_t n, const int64_t *ext_ids, int64_t *n_rows, int64_t *n_results) {
  APSS_TRY(enter(h));
  APSS_TRY(check_stored_query(h, "apss_query_stored", n, ext_ids, n_rows, n_results));
  if (n > 0) {
    APSS_TRY(ensure(h, h->rm_ids, (size_t)n));
    HIPCHK(h, hipMemcpyAsync(h->rm_ids.p, ext_ids, (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  }
  return query_stored_impl(h, n, h->rm_ids.p, n_rows, n_results);  // (synchronises when n > 0: the caller's array may be reused on return)
}

int32_t apss_query_stored_dev(apss_handle *h, int64_t n, const int64_t *d_ext_ids, int64_t *n_rows, int64_t *n_results) {
  APSS_TRY(enter(h));
  APSS_TRY(check_stored_query(h, "apss_query_stored_dev", n, d_ext_ids, n_rows, n_results));
  return query_stored_impl(h, n, d_ext_ids, n_rows, n_results);
}

int32_t apss_stored_query_get(apss_handle *h, apss_stored_query_info *out) {
  if (!h || !out) return APSS_E_INVALID;
  const int32_t caller = out->struct_size;
  if (caller < (int32_t)(2 * sizeof(int32_t)) || caller > (1 << 16))
    return fail(h, APSS_E_INVALID, "apss_stored_query_info.struct_size must be set to sizeof(apss_stored_query_info) before the call");
  const int32_t n = std::min<int32_t>(caller, (int32_t)sizeof(apss_stored_query_info));
  h->qsi.struct_size = n;
  std::memcpy(out, &h->qsi, (size_t)n);
  return APSS_OK;
}

int32_t apss_topk_window_get(apss_handle *h, apss_topk_window_info *out) {
  if (!h || !out) return APSS_E_INVALID;
  const int32_t caller = out->struct_size;
  if (caller < (int32_t)(2 * sizeof(int32_t)) || caller > (1 << 16))
    return fail(h, APSS_E_INVALID, "apss_topk_window_info.struct_size must be set to sizeof(apss_topk_window_info) before the call");
  const int32_t n = std::min<int32_t>(caller, (int32_t)sizeof(apss_topk_window_info));
  h->tw.struct_size = n;
  std::memcpy(out, &h->tw, (size_t)n);
  return APSS_OK;
}

int32_t apss_topk_window_cuts(apss_handle *h, int64_t capacity, int64_t *out_cuts, int64_t *n_cuts) {
  if (!h || !n_cuts) return APSS_E_INVALID;
  if (capacity < 0 || (capacity > 0 && !out_cuts)) return fail(h, APSS_E_INVALID, "apss_topk_window_cuts: capacity without an array");
  *n_cuts = (int64_t)h->win_cuts.size();
  const int64_t n = std::min<int64_t>(capacity, *n_cuts);
  if (n > 0) std::memcpy(out_cuts, h->win_cuts.data(), (size_t)n * sizeof(int64_t));
  return APSS_OK;
}

int32_t apss_topk_get(apss_handle *h, apss_topk_info *out) {
  if (!h || !out) return APSS_E_INVALID;
  const int32_t caller = out->struct_size;
  if (caller < (int32_t)(2 * sizeof(int32_t)) || caller > (1 << 16))
    return fail(h, APSS_E_INVALID, "apss_topk_info.struct_size must be set to sizeof(apss_topk_info) before the call");
  const int32_t n = std::min<int32_t>(caller, (int32_t)sizeof(apss_topk_info));
  h->tk.struct_size = n;
  std::memcpy(out, &h->tk, (size_t)n);
  return APSS_OK;
}

int32_t apss_ext_ids_dev(apss_handle *h, const int64_t **d_store_ext, const int64_t **d_query_ext) {
  if (!h) return APSS_E_INVALID;
  if (d_store_ext) *d_store_ext = h->n_rows > 0 ? h->ext.p : nullptr;
  if (d_query_ext) *d_query_ext = h->res_q_ext;
  return APSS_OK;
}

int32_t apss_results_dev(apss_handle *h, const int32_t **d_q_row, const int32_t **d_c_slot, const float **d_score,
                         int64_t *n_results) {
  if (!h) return APSS_E_INVALID;
  if (h->n_res < 0) return fail(h, APSS_E_STATE, "no query has run on this handle");
  if (d_q_row) *d_q_row = h->out_q;
  if (d_c_slot) *d_c_slot = h->out_c;
  if (d_score) *d_score = h->out_s;
  if (n_results) *n_results = h->n_res;
  return APSS_OK;
}

int32_t apss_results_copy_dev(apss_handle *h, int64_t offset, int64_t count, int32_t *d_q_row, int32_t *d_c_slot,
                              float *d_score) {
  APSS_TRY(enter(h));
  if (h->n_res < 0) return fail(h, APSS_E_STATE, "no query has run on this handle since the last insert");
  if (offset < 0 || count < 0 || offset + count > h->n_res) return fail(h, APSS_E_INVALID, "copy range out of bounds");
  if (count == 0) return APSS_OK;
  if (d_q_row) HIPCHK(h, hipMemcpyAsync(d_q_row, h->out_q + offset, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
  if (d_c_slot) HIPCHK(h, hipMemcpyAsync(d_c_slot, h->out_c + offset, (size_t)count * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
  if (d_score) HIPCHK(h, hipMemcpyAsync(d_score, h->out_s + offset, (size_t)count * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  return APSS_OK;
}

int32_t apss_partial_scores_dev(apss_handle *h, int64_t n_pairs, const int32_t *d_q_row, const int32_t *d_c_slot,
                                float *d_out_partial) {
  APSS_TRY(enter(h));
  if (n_pairs < 0) return fail(h, APSS_E_INVALID, "negative pair count");
  if (n_pairs == 0) return APSS_OK;
  if (!h->last_q_rowptr) return fail(h, APSS_E_STATE, "no query batch on this handle since the last insert");
  if (!d_q_row || !d_c_slot || !d_out_partial) return fail(h, APSS_E_INVALID, "null device pointer");
  PartialArgs a{};
  a.n_pairs = n_pairs;
  a.q_row = d_q_row;
  a.c_slot = d_c_slot;
  a.q_rowptr = h->last_q_rowptr;
  a.q_idx = h->last_q_idx;
  a.q_val = h->last_q_val;
  a.c_rowptr = h->rowptr.p;
  a.c_idx = h->idx.p;
  a.c_val = h->val.p;
  a.out = d_out_partial;
  a.nq = h->last_nq;
  a.n_rows = h->n_rows;
  for (int64_t p0 = 0; p0 < n_pairs; p0 += (1LL << 27)) {  // (a launch may not have 2^32 threads or more)
    PartialArgs aa = a;
    aa.n_pairs = std::min<int64_t>(1LL << 27, n_pairs - p0);
    aa.q_row = d_q_row + p0;
    aa.c_slot = d_c_slot + p0;
    aa.out = d_out_partial + p0;
    hipLaunchKernelGGL(k_partial_scores, dim3((unsigned)ceil_div(aa.n_pairs * kGroup, 256)), dim3(256), 0, h->stream, aa);
    HIPCHK(h, hipGetLastError());
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return APSS_OK;
}

}  // extern "C"
