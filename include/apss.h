/*
 * apss.h -- C ABI of the MI355X-native all-pairs-similarity hot path (libapss_hip.so).
 *
 * Drop-in boundary.  The reference (mcgill-cpslab/all-pairs-similarity, Scala/Akka) has no FFI of its own;
 * the seam this library replaces is the `case IndexData(vectors)` handler of one IndexingWorkerActor
 *     core/src/main/scala/cpslab/deploy/server/IndexingWorkerActor.scala:123-137
 * i.e. buildInvertedIndex (IWA:61-71) + querySimilarItems (IWA:74-111) + CommonUtils.calculateSimilarity
 * (core/src/main/scala/cpslab/deploy/CommonUtils.scala:98-117), with SparkSparseVector (size, indices:
 * Array[Int], values: Array[Double]) in and the SimilarityOutput map (message/Message.scala:20-21) out.
 * A JNI shim (all-pairs-similarity_amd/jvm/) forwards 1:1 to these entry points; see INTEGRATION.md.
 *
 * Conventions: plain pointers and sizes only; every function returns an int32 status (0 = ok, < 0 = error,
 * text via apss_last_error); nothing throws or calls back across the boundary; inputs are caller-owned and
 * consumed before return; results stay in the handle until the next query-type call, insert or clear (after an
 * insert or clear the result calls answer APSS_E_STATE) and are copied out with apss_fetch_results (two-call
 * pattern: ask for the count, then fetch).
 * Threading mirrors the actor model: at most one thread inside a given handle at a time, different handles
 * may be used concurrently; the library sets the device on every entry and owns one HIP stream per handle.
 *
 * Semantics: "intended" semantics of the reference -- exact threshold join
 * sim(q, c) = sum_i q_i * c_i >= theta (inclusive, IWA:93) over every candidate c sharing >= 1 indexed term
 * with q, self-exclusion by EXTERNAL id (IWA:91), each (q, c) reported once (the reference's duplicate
 * reports across term workers, IWA:105 "TODO: need to deduplicate", are collapsed).  The reference's
 * first-dim skip quirk (IWA:89 vs 106) is NOT reproduced on the device; it is restated only in oracle/.
 * Scores are accumulated in fp32 on the device (reference: double): |score - double| <= 1e-5 and set
 * membership may differ only for |score - theta| <= 1e-5.
 */
#ifndef APSS_H
#define APSS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define APSS_OK 0
#define APSS_E_INVALID (-1)     /* bad argument / malformed vector: the IllegalArgumentException of `require`
                                   (CommonUtils.scala:99, vector/SparseVector.scala:75,202) */
#define APSS_E_NOMEM (-2)       /* host or device allocation failed */
#define APSS_E_DEVICE (-3)      /* HIP runtime error (no GPU, launch failure, ...) */
#define APSS_E_STATE (-4)       /* call not valid in this state (e.g. fetch before any query) */
#define APSS_E_UNSUPPORTED (-5) /* option not supported by this build */

/* apss_config.flags */
#define APSS_FLAG_VALUE_PRUNE 1u /* drop entries with value <= index_threshold before indexing, no
                                    re-normalisation (WriteWorkerActor.scala:188-194) */
#define APSS_FLAG_ADMISSION 2u   /* admit a vector only if sum_i v_i >= theta (EntryProxyActor.scala:81-93,
                                    max-weight == 1.0 per EntryProxyActor.scala:51-57) */
#define APSS_FLAG_NORMALIZE 4u   /* L2-normalise rows on ingest (benchmark/LoadGenerator.scala:34-37) */
#define APSS_FLAG_FORCE_SCAN 8u  /* always use the general accumulator-scan kernel (the theta <= 0 path) */
#define APSS_FLAG_FORCE_GENERAL 16u /* never use the per-wave speed path of the probe (test hook) */
#define APSS_FLAG_EXACT_ACCUM 32u   /* single-pass join with exact accumulators only: no coarse filter + rescoring pass */
#define APSS_FLAG_NO_SYMMETRY 64u    /* a whole-store join (apss_self_join, insert-and-query into an empty handle) probes every
                                       pair in BOTH directions like the reference (IWA:123-134) instead of running the
                                       filter over half of the tile pairs and mirroring its survivors; same results */

typedef struct apss_handle apss_handle;

typedef struct apss_config {
  int32_t struct_size;     /* sizeof(apss_config), for ABI evolution */
  int32_t dim;             /* cpslab.allpair.vectorDim: every vector's `size` (CU:99) */
  double theta;            /* cpslab.allpair.similarityThreshold (IWA:23) */
  double index_threshold;  /* cpslab.allpair.indexThreshold (WWA:35), used with APSS_FLAG_VALUE_PRUNE */
  uint32_t flags;          /* APSS_FLAG_* */
  int32_t device_id;       /* HIP device ordinal */
  int32_t term_lo;         /* term-range shard [term_lo, term_hi): only these dims are indexed and scored */
  int32_t term_hi;         /*   (0, 0) or (0, dim) = the whole term space (single GPU) */
  int32_t tile_rows;       /* candidate tile of the EXACT rendering of the index (8-B postings, u32 / fp32 accumulators in one
                              workgroup's LDS: k_probe_wave, k_probe): 0 = default (16384 rows: two workgroups share a CU's
                              160 KB of LDS), else a multiple of 64, <= 32768.  The coarse rendering the two-pass join filters
                              with has tiles of min(2 * tile_rows, 32768) rows (16-bit accumulators); with tile_rows == 0 the
                              library may pick 65536 (sparse regime, term shards with 8-bit accumulators) or 131072 rows
                              (sparser still) from the data: apss_stats.tiles says what it took */
  int32_t head_terms;      /* dense-head block: 0 = the library decides from the term distribution, -1 = never,
                              N <= 32768 = always the N most frequent terms.  Up to 256 terms: a column each.  More: ONE block of
                              256 columns, the 128 most frequent terms with a column each, the others FOLDED into the other 128
                              (a shared column holds the L2 norm of its terms: by Cauchy-Schwarz an upper bound of their partial
                              score that keeps the row's norm).  Terms in the block are scored by an MFMA contraction instead of their posting lists --
                              over INT8 rows rounded UP (a sound filter: integer products, int32 sums) or bf16 rows
                              (apss_stats.head_int8); survivors are re-scored exactly: results are the same set */
  int64_t capacity_rows;   /* hints for the initial HBM reservation (0 = grow on demand) */
  int64_t capacity_nnz;
} apss_config;

typedef struct apss_stats {
  int32_t struct_size;      /* IN: sizeof(apss_stats) as the caller compiled it -- apss_stats_get writes no more than that many
                               bytes (the struct grows at its end from release to release); OUT: the bytes written */
  uint32_t symmetric;       /* 1: the last call ran as a symmetric whole-store join (see APSS_FLAG_NO_SYMMETRY) */
  int64_t rows;             /* vectors in the store */
  int64_t nnz;              /* postings in the index */
  int64_t tiles;            /* candidate tiles */
  int64_t posting_visits;   /* (query, term, posting) FMAs of the last query-type call */
  int64_t candidate_pairs;  /* distinct (q, c != q) pairs scored by the last query-type call.  With a dense-head block:
                               max(pairs sharing a tail term, pairs sharing a head term), a LOWER bound of the distinct
                               count (a pair sharing both kinds is scored by both filters, counted once here) */
  int64_t result_pairs;     /* pairs >= theta of the last query-type call */
  double probe_ms;          /* device time of the last call's probe kernel(s), HIP events */
  double build_ms;          /* device time of the last insert's index build, HIP events */
  int64_t probe_launches;   /* probe kernel launches of the last call (re-runs after a result-buffer growth count) */
  int64_t hbm_bytes;        /* device bytes currently reserved by the handle */
  int64_t filter_survivors; /* two-pass join: pairs the coarse filter passed on to exact rescoring (0: single pass) */
  double rescore_ms;        /* two-pass join: device time of the exact rescoring kernel */
  int64_t head_terms;       /* terms held in the dense-head block at the last call (0: none) */
  int64_t head_pairs;       /* (q, c != q) pairs sharing a head term, scored by the dense contraction of the last call */
  int64_t head_survivors;   /* pairs the dense filter passed on to exact rescoring */
  double head_ms;           /* device time of the dense-head kernel, HIP events */
  double head_flops;        /* 2 * KH * (query slots x candidate rows actually multiplied) of the last call */
  int64_t thin_launches;    /* probe launches of the last call that took the thin-round filter kernel (k_probe_even: a term
                               shard's or a sparse batch's rounds of a few hundred postings) */
  uint32_t downgrades;      /* APSS_DOWNGRADE_*: permanent fallbacks (until apss_clear) this handle took because of a call it could
                               not serve on its fast layout; each costs one full index rebuild when it happens */
  uint32_t head_columns;    /* width of a row of the dense-head block at the last call: 64 | 128 | 256 (0: none) */
  char probe_kernel[96];    /* the probe kernel instantiation the last query-type call launched, as rocprofv3 prints its name up
                               to the template arguments' spelling, e.g. "k_probe_even<512, 6, 128, false, false, false>" (threads, window steps,
                               long-segment list, shard rule, signed, 8-bit accumulators) or "k_probe_even_merged<4, true>" (a term shard's rounds
                               with two query rows each: window steps, 8-bit accumulators; queries_per_round); "" before any probe.
                               One name is not rocprofv3's: "k_probe_even<512, 6, 128, false, false, true, planes>" is the plain
                               512-thread instantiation with two planes of 8-bit sums and one barrier per round, the kernel
                               k_probe_planes<6> */
  int64_t device_posting_visits; /* posting visits the kernels of the last call actually made: equal to posting_visits except
                                    on a symmetric whole-store join, where posting_visits / candidate_pairs keep counting what
                                    the reference's two-directional probe visits and the device visits about half of it */
  uint32_t symmetric_declined; /* APSS_SYM_*: why the last query-type call did NOT run as a symmetric join (0 when it did) */
  int32_t query_chunk;      /* query rows per workgroup of the last probe launch (the symmetric join needs a power of two that
                               divides filter_tile_rows) */
  int32_t filter_tile_rows; /* candidate rows per tile of the index rendering the last probe ran over */
  int32_t head_int8;        /* 1: the dense-head block's rows are the INT8 rendering (rounded up; v_mfma_i32_32x32x32_i8: head_flops are
                               integer operations then, against twice the bf16 peak), 0: bf16 */
  int32_t queries_per_round; /* thin-round filter of a term shard: query rows that SHARED a round of the last probe launch (1 | 2 | 4).
                                M neighbouring rows are staged as one row and a candidate's accumulator holds the sum of their M
                                filter sums -- an upper bound of each (non-negative weights), so the filter stays sound; a crossing
                                becomes M pairs, each tested against the shard rule on its exact partial score before it is
                                reported (filter_survivors: no more than without merging).  candidate_pairs then counts a
                                candidate touched by several rows of one round once: a lower bound */
  int32_t reserved0;
} apss_stats;

/* apss_stats.symmetric_declined */
#define APSS_SYM_RAN 0u          /* the call ran symmetrically */
#define APSS_SYM_FLAG 1u         /* APSS_FLAG_NO_SYMMETRY (or the debug token) */
#define APSS_SYM_NOT_WHOLE 2u    /* the query batch is not the whole indexed store (a batch onto an older store, an outside
                                    batch, rows waiting outside the tile index) */
#define APSS_SYM_PATH 3u         /* the call did not take the two-pass filter (theta <= 0, exact-accumulate, signed fallback) */
#define APSS_SYM_LONG_ROWS 4u    /* a query row of more than 512 terms is cut into parts (virtual rows) */
#define APSS_SYM_ONE_TILE 5u     /* the index has a single tile: nothing to halve */
#define APSS_SYM_CHUNK 6u        /* the query chunk does not divide a tile (query_chunk, filter_tile_rows) */

#define APSS_DOWNGRADE_ACC8 1u /* 8-bit accumulators over 65536 / 131072-row tiles given up (a long row, a large norm, an
                                  unselective byte filter): 16-bit accumulators over smaller tiles.  Also set when the two-plane
                                  byte sums of a plain handle over <= 32768-row tiles proved unselective: back to 16-bit sums
                                  over the same tiles, the one downgrade that rebuilds nothing */
#define APSS_DOWNGRADE_HEAD 2u /* the dense-head block was given up (signed weights, norms out of range): its terms are back
                                  in the inverted index */

/* ---- lifetime (actor construction / stop, IWA:21-39) ---- */
int32_t apss_create(const apss_config *cfg, apss_handle **out);
void apss_destroy(apss_handle *h);
/* message of the last failing call on this handle ("" if none); h == NULL: last apss_create failure */
const char *apss_last_error(const apss_handle *h);
/* Run the handle's work on a caller-owned HIP stream (hipStream_t as void*; NULL = the device's default stream),
 * or, with use_own != 0, go back to the handle's own stream.  The handle's own stream is a blocking stream: it
 * orders itself after work already queued on the default stream (where PyTorch runs unless told otherwise). */
int32_t apss_set_stream(apss_handle *h, void *hip_stream, int32_t use_own);

/* ---- host-pointer entry points (what the JNI shim binds) ----
 * CSR batch: n rows; row i = indices[rowptr[i] .. rowptr[i+1]) strictly increasing in [0, dim), values alike
 * (doubles, as SparkSparseVector.values), ext_ids[i] = the caller's integer handle for the String id. */

/* buildInvertedIndex(batch), IWA:61-71 */
int32_t apss_insert(apss_handle *h, int64_t n, const int64_t *rowptr, const int32_t *indices,
                    const double *values, const int64_t *ext_ids);
/* querySimilarItems(batch) on a frozen index (stopUpdateIndex, IWA:125-127); unseen dims are empty lists */
int32_t apss_query(apss_handle *h, int64_t n, const int64_t *rowptr, const int32_t *indices,
                   const double *values, const int64_t *ext_ids, int64_t *n_results);
/* the IndexData handler: build, then query; the batch sees itself and everything before it (IWA:125-133) */
int32_t apss_insert_and_query(apss_handle *h, int64_t n, const int64_t *rowptr, const int32_t *indices,
                              const double *values, const int64_t *ext_ids, int64_t *n_results);
/* query every stored vector against the whole index (single-batch self-join, the benchmark driver) */
int32_t apss_self_join(apss_handle *h, int64_t *n_results);

/* results of the last query-type call: (query ext id, candidate ext id, score); order unspecified (apss_set_top_k specifies one) */
int32_t apss_result_count(const apss_handle *h, int64_t *n_results);
int32_t apss_fetch_results(apss_handle *h, int64_t offset, int64_t count, int64_t *out_q, int64_t *out_c,
                           float *out_score);

int32_t apss_size(const apss_handle *h, int64_t *rows, int64_t *nnz);
int32_t apss_stats_get(apss_handle *h, apss_stats *out);

/* ---- device-pointer entry points (inputs already resident in HBM: bench.py, multi-GPU host code) ----
 * d_rowptr int64[n+1] (relative to the batch: d_rowptr[0] == 0), d_indices int32[nnz], d_values float[nnz],
 * d_ext_ids int64[n]; all on the handle's device.  Work is enqueued on the handle's stream; the calls that
 * return counts synchronise that stream. */
int32_t apss_insert_dev(apss_handle *h, int64_t n, int64_t nnz, const int64_t *d_rowptr,
                        const int32_t *d_indices, const float *d_values, const int64_t *d_ext_ids);
int32_t apss_query_dev(apss_handle *h, int64_t n, int64_t nnz, const int64_t *d_rowptr,
                       const int32_t *d_indices, const float *d_values, const int64_t *d_ext_ids,
                       int64_t *n_results);
int32_t apss_insert_and_query_dev(apss_handle *h, int64_t n, int64_t nnz, const int64_t *d_rowptr,
                                  const int32_t *d_indices, const float *d_values, const int64_t *d_ext_ids,
                                  int64_t *n_results);
/* drop the index and the store, keep the reservation (lets a benchmark step re-run build + join) */
int32_t apss_clear(apss_handle *h);
/* device views of the last results: int32 query row (within the last query batch), int32 candidate slot,
 * float score; valid until the next query-type call */
int32_t apss_results_dev(apss_handle *h, const int32_t **d_q_row, const int32_t **d_c_slot,
                         const float **d_score, int64_t *n_results);
/* the same, copied device-to-device into caller-owned HBM buffers (any of the three may be NULL) on the handle's
 * stream: how multi-GPU host code keeps the candidate lists on the device between the phases of a sharded join */
int32_t apss_results_copy_dev(apss_handle *h, int64_t offset, int64_t count, int32_t *d_q_row, int32_t *d_c_slot,
                              float *d_score);

/* ---- term-range shards (multi-GPU; one handle per GPU owning dims [term_lo, term_hi)) ----
 * Phase 1, local: a query-type call on a shard handle reports CANDIDATES, pairs whose local partial score
 * p_g satisfies p_g >= theta * |q_g||c_g| / (|q||c|)  (|x_g| = L2 norm of x restricted to the shard's dims, |x| =
 * norm of the whole row as the caller handed it in, after the value prune).  Every pair with total score >= theta
 * passes this test on at least one shard, whatever the row norms and whatever the signs of the weights:
 * p_g <= |q_g||c_g| and sum_g |q_g||c_g| <= |q||c| (Cauchy-Schwarz twice), so if every shard failed the test the
 * total would be below theta.  The caller must hand every shard the WHOLE row (the library restricts it).
 * Phase 2: the host unions the candidate lists of all shards, every shard fills its exact partial score for
 * each pair with apss_partial_scores_dev, the partials are summed across GPUs (RCCL all-reduce) and
 * thresholded.  Pairs are (query row of the last query batch, candidate slot). */
int32_t apss_partial_scores_dev(apss_handle *h, int64_t n_pairs, const int32_t *d_q_row,
                                const int32_t *d_c_slot, float *d_out_partial);


/* ---- dense-head block set by the caller ----
 * The `n_terms` (<= 32768; more than 256: the first 128 with a column each, the others folded, in the order given) most frequent terms are scored by an MFMA contraction (INT8 rows rounded up, or bf16: apss_stats.head_int8) over W = [rows x n_terms] instead of
 * their posting lists (CommonUtils.scala:110-115 restricted to those dims; a FILTER: survivors are re-scored exactly).
 * On a plain handle this replaces the library's own choice (apss_config.head_terms).  On a TERM SHARD it is the only way
 * to get a block: every shard of a join must be given the SAME terms -- they are a part of their own, {H, T_1 .. T_T}, in
 * the partition the candidate rule above is proved for, so a head term lies in no shard's inverted index (it stays in the
 * store of the shard whose range holds it, for the exact partial scores of phase 2) -- and shard `part` of `n_parts`
 * multiplies the 64-row candidate tiles t with t % n_parts == part of the contraction against the whole query batch
 * (the block is cut over the GPUs by candidate row, not by term).  A query-type call on such a shard reports the union of
 * both filters' candidates (duplicates possible).  Valid on an empty handle only (before the first insert / after
 * apss_clear); the setting survives apss_clear; n_terms == 0 removes it.  Shards: non-negative weights, no
 * APSS_FLAG_ADMISSION (APSS_E_UNSUPPORTED otherwise). */
int32_t apss_set_head_terms(apss_handle *h, int32_t n_terms, const int32_t *terms, int32_t part, int32_t n_parts);
/* How many of the 256 columns of a head of more than 256 terms are FOLDED columns (64 | 128 | 192; 0 = the default, 128):
 * the 256 - columns most frequent terms keep a column each, the others share the folded ones (L2 norm per column).  Takes effect at the next
 * apss_set_head_terms; on an empty handle. */
int32_t apss_set_head_fold(apss_handle *h, int32_t columns);
/* the block's terms in block order (chosen by the library or set by the caller); *n_terms = how many there are */
int32_t apss_get_head_terms(apss_handle *h, int32_t capacity, int32_t *out_terms, int32_t *n_terms);
/* device views of the external ids: int64[rows] of the store, int64[query rows] of the last query batch (NULL before
 * any query-type call / after an insert); valid until the next insert, query-type call or clear */
int32_t apss_ext_ids_dev(apss_handle *h, const int64_t **d_store_ext, const int64_t **d_query_ext);
/* device views of the stored CSR: int64[rows + 1] row offsets (from 0), int32[nnz] terms, float[nnz] weights -- the rows as they
 * are scored (after normalisation, value prune and admission; a term shard holds only its range of every row).  NULL views
 * when the store is empty; valid until the next insert or clear */
int32_t apss_get_store_dev(apss_handle *h, const int64_t **d_rowptr, const int32_t **d_indices, const float **d_values,
                       int64_t *rows, int64_t *nnz);
/* ---- read-only view of a built rendering of the inverted index ("What the tests hold the index to") ----
 * rendering 0: the exact rendering (8-B postings {uint32 slot, float w}); 1: the coarse rendering (4-B posting words).
 * The call builds nothing, launches nothing and reserves nothing: it copies out what the handle already knows.  Layout:
 *   d_seg  uint32[n_tiles][dim][2]: {first posting, length} of term t in tile T, relative to the tile's base; every start is a
 *          multiple of seg_align, and a segment owns the aligned extent [start, start + ceil(length / seg_align) * seg_align)
 *   d_base int64[n_tiles + 1]: first posting of every tile in d_post; d_base[n_tiles] == post_used
 *   d_post postings: slot = store row - tile * tile_rows.  Coarse words by slot_form:
 *          APSS_SLOT_TIMES2  (slot * 2) | fp16 bits << 16       (tiles of at most 32768 rows)
 *          APSS_SLOT_PLAIN    slot      | fp16 bits << 16       (65536-row tiles)
 *          APSS_SLOT_WIDE     slot << 15 | fp16 bits & 0x7fff   (131072-row tiles; weights are non-negative there)
 *          the fp16 is the weight rounded to nearest even, raised to bits 1 where it would be 0: no posting word is zero, and
 *          every word of an aligned extent behind its segment's length IS zero.  The exact rendering always says APSS_SLOT_PLAIN.
 *   d_sub  float[rows]: with weights_scaled the coarse weights are stored divided by d_sub[row] where that is positive (the
 *          shard rule: |x_g| / |x|; a handle with a dense-head block: its tail's share); NULL otherwise
 *   d_tile_min float[n_tiles]: the smallest positive d_sub over each tile's rows (0: none), for either rendering of a handle that
 *          scales; NULL otherwise
 * The rendering covers the store rows [0, built_rows): rows behind them wait outside the index until a later insert folds them in.
 * A rendering that has not been built (or whose tiles are stale: the exact rendering of a handle that filters with the coarse one
 * is rebuilt only by a call that needs it) answers n_tiles = 0 and NULL views.  The views are valid until the next insert, clear,
 * compaction or query-type call (which may rebuild a rendering). */
#define APSS_SLOT_PLAIN 0
#define APSS_SLOT_TIMES2 1
#define APSS_SLOT_WIDE 2
typedef struct apss_index_view {
  int32_t struct_size;     /* IN: caller's sizeof; OUT: bytes written (as apss_stats) */
  int32_t rendering;       /* as asked */
  int32_t tile_rows;       /* rows per tile */
  int32_t seg_align;       /* postings per aligned unit (one 128-B line) */
  int32_t posting_bytes;   /* 8 or 4 */
  int32_t slot_form;       /* APSS_SLOT_* */
  int32_t weights_scaled;  /* 1: weights are stored divided by d_sub[row] */
  int32_t dim;             /* terms per tile of d_seg (its stride) */
  int64_t n_tiles;
  int64_t built_rows;
  int64_t post_used;       /* postings of d_post in use, padding included */
  const void *d_seg;
  const int64_t *d_base;
  const void *d_post;
  const float *d_sub;
  const float *d_tile_min;
  int64_t max_seg;         /* longest (tile, term) segment, as the probe was told */
  int64_t long_segs;       /* segments of more than 256 postings, as the probe was told (exact for a rendering built whole
                              from tile 0; an append to the last tile does not recount that tile) */
  double chunk_weight;     /* 16-posting chunks an average stored row deals out per tile (measured by a build from tile 0) */
} apss_index_view;
int32_t apss_index_view_get(apss_handle *h, int32_t rendering, apss_index_view *out);

/* as apss_insert_dev, for rows that ALREADY passed this configuration's ingest filters (rows of some handle's store, e.g.
 * reassembled from term shards): no normalisation, value prune or admission is applied again (a pruned row re-normalised
 * would change, an admission test on its pruned sum could drop it).  A term shard still keeps its range of every row and
 * takes its sub-norms and dense-head rows from the whole rows it is handed */
int32_t apss_insert_stored_dev(apss_handle *h, int64_t n, int64_t nnz, const int64_t *d_rowptr, const int32_t *d_indices,
                               const float *d_values, const int64_t *d_ext_ids);

/* ---- per-query top-k ----
 * k = 0 (the default): off -- every query-type call returns every pair with score >= theta, in no specified order.
 * k in 1 .. APSS_TOP_K_MAX: the final list of every query-type call made afterwards (apss_query[_dev], apss_insert_and_query[_dev],
 * apss_self_join) holds, for each query row of the batch, at most k of that row's pairs >= theta -- the first k in the order
 *   1. fp32 score descending, as the device reports it (-0.0f counts as +0.0f and is reported as +0.0f);
 *   2. candidate external id ascending;
 *   3. candidate slot ascending (two stored rows may carry the same external id)
 * -- and its order is specified: grouped by query row ascending, in rank order inside a row.  Everything that reads the
 * results of the last call (n_results, apss_result_count, apss_fetch_results, apss_results_dev, apss_results_copy_dev,
 * apss_stats.result_pairs) sees the selected list; apss_topk_get reports the count before the cut.  The setting may be changed
 * at any time (it takes effect at the next query-type call, leaves the last call's results alone and survives apss_clear).
 * The cut is one device pass over the call's final list on the handle's stream (k_topk_*: count, scan, scatter, select).
 * APSS_E_INVALID: k < 0 or k > APSS_TOP_K_MAX.  APSS_E_UNSUPPORTED: k > 0 on a term shard (its candidates carry partial scores;
 * apss_group_set_top_k cuts behind the group's exchange). */
#define APSS_TOP_K_MAX 1024
typedef struct apss_topk_info {
  int32_t struct_size;       /* IN: caller's sizeof; OUT: bytes written (as apss_stats) */
  int32_t k;                 /* the setting the last query-type call ran with (0: off) */
  int64_t pairs_over_theta;  /* pairs >= theta of the last call before the cut (== result_pairs when k == 0) */
  int64_t kept;              /* pairs in the final list */
  int64_t queries_cut;       /* query rows that had more than k pairs (0 when k == 0) */
  int64_t longest_segment;   /* most pairs >= theta any one query row had (0 when k == 0: nothing counts them) */
  double select_ms;          /* device time of the k_topk_* kernels, HIP events (0 when k == 0) */
  int32_t select_launches;   /* k_topk_* launches of the last call (0 when k == 0) */
  int32_t reserved0;
} apss_topk_info;
int32_t apss_set_top_k(apss_handle *h, int32_t k);
int32_t apss_topk_get(apss_handle *h, apss_topk_info *out);

/* ---- per-query top-k in bounded memory: windows of query rows ("Windows") ----
 * Without a window budget the cut runs once, over the call's whole list of pairs >= theta -- which must fit the device first (at
 * theta <= 0: every pair that shares a term).  With max_pairs > 0 and k > 0 a query-type call whose batch could report more than
 * max_pairs pairs (query rows x stored rows > max_pairs) is run as WINDOWS of consecutive query rows, each joined and cut on its
 * own and appended to the call's list, so that the handle never holds more than about max_pairs uncut pairs:
 *   b(q) = min(sum of df_t over the terms t of query row q, stored rows), df_t = stored rows holding t (rows waiting outside the
 *   tile index included), bounds the pairs of row q: every reported pair shares a term.  A window is the longest run of rows
 *   from its start whose sum of b is <= max_pairs; a row with b > max_pairs is a window of one (single_row_over counts them).
 * The answer is the list of the unwindowed call, element by element: same order, same score bits; apss_topk_info and apss_stats
 * are summed over the windows (longest_segment: the maximum).  The symmetric whole-store join does not run in windows
 * (apss_stats.symmetric_declined = APSS_SYM_NOT_WHOLE).  k_win_df / k_win_bound plan the windows (df is recomputed from the
 * store at every windowed call), k_win_append concatenates.
 * max_pairs = 0 (the default): off, everything as without the setting.  No effect while k = 0.  The setting may be changed at any
 * time (it takes effect at the next query-type call, leaves the last call's results alone and survives apss_clear).
 * APSS_E_INVALID: max_pairs < 0.  APSS_E_UNSUPPORTED: max_pairs > 0 on a term shard (as apss_set_top_k). */
typedef struct apss_topk_window_info {
  int32_t struct_size;       /* IN: caller's sizeof; OUT: bytes written (as apss_stats) */
  int32_t windows;           /* windows of the last query-type call (0: it was not windowed) */
  int64_t max_pairs;         /* the setting the call ran with */
  int64_t bound_total;       /* sum of b(q) over the batch */
  int64_t bound_window_max;  /* the largest sum of b over one window */
  int64_t pairs_window_max;  /* the most pairs >= theta any one window's uncut final list held (with apss_set_top_k_tile_cut
                              applied: the most pairs any one window's probe EMITTED -- what the handle really held) */
  int64_t rows_window_min;   /* rows of the shortest / longest window */
  int64_t rows_window_max;
  int64_t single_row_over;   /* windows of one row whose bound exceeds max_pairs */
  int32_t overflow_reruns;   /* windows whose probe ran again because a list overflowed */
  int32_t plan_launches;     /* k_win_df + k_win_bound launches (k_win_append runs once per non-empty window and is not counted) */
  double plan_ms;            /* device time of the planning kernels, HIP events */
} apss_topk_window_info;
int32_t apss_set_top_k_window(apss_handle *h, int64_t max_pairs);
int32_t apss_topk_window_get(apss_handle *h, apss_topk_window_info *out);
/* the windows of the last query-type call as windows + 1 ascending row offsets of its batch (cuts[0] = 0, cuts[windows] = rows of
 * the batch); *n_cuts = how many there are (0: the call was not windowed); the first min(capacity, *n_cuts) are written */
int32_t apss_topk_window_cuts(apss_handle *h, int64_t capacity, int64_t *out_cuts, int64_t *n_cuts);

/* ---- per-query top-k: each round cut inside the theta <= 0 probe kernel ("Cut inside the probe") ----
 * At theta <= 0 the probe writes every touched candidate of every (query row, candidate tile) round, and the pass above then
 * reads that list three more times to keep k pairs per row.  With on = 1 and k > 0, a call that runs the theta <= 0 kernel
 * (k_probe<2, ...>) on a plain handle cuts each ROUND before it is written: a round with more than k pairs >= theta emits only
 * those whose score key (the order-preserving 32-bit image of the fp32 score) is >= P << 16, P = the top 16 bits of the round's
 * k-th largest key.  Every pair among a row's first k is among the first k of its own round, so the pass sees a superset of
 * every row's winners with unchanged score bits: the final list is the list of the call without the setting, element by element.
 * apss_topk_info keeps reporting what the call FOUND (pairs_over_theta, queries_cut, longest_segment: from per-row counts the
 * kernel takes before the cut); apss_topk_tile_cut_info says what the probe emitted.  In a windowed call every window's probe
 * takes the cut; the info is summed over the windows, and apss_topk_window_info.pairs_window_max then reports the EMITTED list
 * of a window, which is what the handle really held (ties can make a round emit everything: b(q) stays the reservation).
 * Every other path ignores the setting and says why in `declined`: theta > 0 (the two-pass join, k_probe_wave, k_probe<0 | 1>,
 * with or without APSS_FLAG_EXACT_ACCUM), k = 0, a call that launched nothing.  Groups do not take the setting.
 * on = 0 (the default): off, everything exactly as without the setting.  The setting may be changed at any time (it takes effect
 * at the next query-type call, leaves the last call's results alone and survives apss_clear).
 * APSS_E_INVALID: on outside {0, 1}, NULL.  APSS_E_UNSUPPORTED: on = 1 on a term shard (as apss_set_top_k). */
#define APSS_TILE_CUT_RAN 0
#define APSS_TILE_CUT_OFF 1     /* setting off */
#define APSS_TILE_CUT_NO_K 2    /* k == 0 */
#define APSS_TILE_CUT_PATH 3    /* the call did not run the theta <= 0 kernel (or the handle is a term shard) */
typedef struct apss_topk_tile_cut_info {
  int32_t struct_size;     /* IN: caller's sizeof; OUT: bytes written */
  int32_t applied;         /* 1: the last query-type call's probe cut its rounds */
  int32_t declined;        /* APSS_TILE_CUT_* */
  int32_t prefix_bits;     /* 16 */
  int64_t pairs_emitted;   /* pairs the probe left for the pass (== pairs_over_theta when not applied) */
  int64_t rounds_cut;      /* (query row, tile) rounds that had more than k pairs >= theta */
} apss_topk_tile_cut_info;  /* 32 bytes */
int32_t apss_set_top_k_tile_cut(apss_handle *h, int32_t on);
int32_t apss_topk_tile_cut_get(apss_handle *h, apss_topk_tile_cut_info *out);

/* ---- removal of stored vectors: mark, drop from the results, compact the store ----
 * The reference's store only grows; it stops indexing after cpslab.allpair.benchmark.expDuration instead
 * (IndexingWorkerActor.scala:33-39, 143-144).  Plain handles only.
 *
 * apss_remove[_dev](n, ext_ids) MARKS every stored row whose external id is in the list (two rows may carry one id: both are
 * marked; self-exclusion is by external id too).  Ids that are not stored, ids whose rows are marked already and ids repeated in
 * the list are ignored; *n_rows_removed (may be NULL) = the rows newly marked.  The mark belongs to the SLOT, not to the id: a
 * vector inserted later under a removed id is live.  The results of the last call are left alone (as apss_set_top_k leaves
 * them).  One pass over the store's external ids per call (k_rm_mark), whatever n is.  _dev: d_ext_ids int64[n] on the handle's
 * device, read on the handle's stream; the call synchronises that stream.
 *
 * From then on every query-type call answers as if the marked rows were not stored: no pair with a marked candidate is reported,
 * and when the query batch IS stored rows (apss_self_join) no pair with a marked query row either -- on every path (two-pass
 * join, APSS_FLAG_EXACT_ACCUM, APSS_FLAG_FORCE_SCAN, theta <= 0, rows waiting outside the tile index, the dense head, virtual rows,
 * the mirrored half of a symmetric join): the call's final list is filtered once (k_rm_drop) BEFORE the top-k cut, so with k > 0 a
 * row's k best are its k best LIVE pairs, and in a windowed call every window's list is filtered before that window's cut.
 * n_results, apss_stats.result_pairs, apss_topk_info.pairs_over_theta / queries_cut / longest_segment speak of live pairs.
 * apss_stats.candidate_pairs, posting_visits and the windows' b(q) keep counting marked rows until a compaction (the probe still
 * visits them): they stay upper bounds.  apss_topk_window_info.pairs_window_max is taken before the filter (what the handle held).
 * While any row is marked apss_set_top_k_tile_cut is declined (APSS_TILE_CUT_REMOVED): a round's k-th score could belong to a
 * marked candidate, so the cut inside the probe is not safe; the final list stays right.
 * With nothing marked a query-type call launches nothing new and reads nothing new.
 *
 * apss_compact: the store becomes the live rows in their stored order and the index is rebuilt -- exactly what apss_clear
 * followed by apss_insert_stored_dev of the live rows gives (no normalisation, prune or admission is applied again; settings
 * survive as they do across apss_clear), without the rows leaving the device.  Slots shift: the results of the last call are gone
 * afterwards (APSS_E_STATE, as after an insert), and so are the views of apss_get_store_dev / apss_ext_ids_dev.  With nothing
 * marked it is a no-op that keeps the last results.  While it runs apss_stats.hbm_bytes may grow by one copy of the live store
 * (the gathered rows wait in the handle's input staging, which is kept like every reservation).
 *
 * apss_set_auto_compact(f): f = 0 (the default) = off; f in (0, 1): at the start of every insert-type call (apss_insert,
 * apss_insert_and_query, their _dev forms, apss_insert_stored_dev) the handle compacts first if rows_removed > f * rows.  The
 * setting survives apss_clear.  APSS_E_INVALID: f outside [0, 1) or not a number.
 *
 * apss_clear drops the marks.  apss_size and apss_stats.rows keep reporting physical rows, marked ones included.
 * APSS_E_INVALID: NULL handle, n < 0, NULL ids with n > 0.  APSS_E_UNSUPPORTED ("term shard"): any of the five on a term shard --
 * it holds slices of rows and a compaction needs whole ones.  apss_group has no removal. */
#define APSS_TILE_CUT_REMOVED 4 /* apss_topk_tile_cut_info.declined: rows are marked removed (apss_remove) */
typedef struct apss_removal_info {
  int32_t struct_size;        /* IN: caller's sizeof; OUT: bytes written (as apss_stats) */
  int32_t compactions;        /* since create */
  int64_t rows_removed;       /* stored rows currently marked (0 after a compaction or apss_clear) */
  int64_t rows_live;          /* apss_size rows - rows_removed */
  int64_t removed_total;      /* rows ever marked, since create */
  int64_t pairs_dropped;      /* pairs the last query-type call dropped because an end was removed */
  int64_t compacted_rows;     /* rows the last compaction discarded */
  double auto_compact;        /* the setting */
  double mark_ms, drop_ms, compact_ms; /* device time, HIP events: last apss_remove*, last call's drop, last compaction */
  int32_t drop_launches;      /* k_rm_drop launches of the last query-type call (0 when nothing is marked) */
  int32_t reserved0;
} apss_removal_info;          /* 88 bytes */
int32_t apss_remove(apss_handle *h, int64_t n, const int64_t *ext_ids, int64_t *n_rows_removed);
int32_t apss_remove_dev(apss_handle *h, int64_t n, const int64_t *d_ext_ids, int64_t *n_rows_removed);
int32_t apss_compact(apss_handle *h);
int32_t apss_set_auto_compact(apss_handle *h, double fraction);
int32_t apss_removal_get(apss_handle *h, apss_removal_info *out);

/* ---- query stored vectors by external id, gathered on the device ----
 * "What is similar to these items that you already hold?"  The reference never asks: its actor answers a vector only at the
 * moment it arrives (IndexingWorkerActor.scala:123-137) and keeps nothing but a String -> Long id map on the JVM side.  Plain
 * handles only.
 *
 * The batch.
 *  - It holds every live stored row whose external id is in the list, in stored (slot) order.
 *  - A row that is marked removed is not selected.
 *  - An id carried by two live rows selects both.
 *  - An id that is repeated in the list, not stored, or stored only as marked rows selects nothing more.
 *  - *n_rows (may be NULL) is the number of rows in the batch.
 * The answer.
 *  - It is what apss_query_dev gives for those rows exactly as apss_get_store_dev shows them.
 *  - Normalisation, value prune and admission are not applied again.
 *  - Self-exclusion is by external id, so a selected row never pairs with its twin under the same id.
 *  - Pairs with marked candidates are dropped by the existing k_rm_drop, before the top-k cut.
 *  - apss_set_top_k, apss_set_top_k_window and apss_set_top_k_tile_cut apply as to any outside batch.
 *  - The call takes no symmetric join even when every stored id is named: apss_stats.symmetric = 0,
 *    symmetric_declined = APSS_SYM_NOT_WHOLE.
 *  - It builds nothing.  Rows waiting outside the tile index are met the way apss_query meets them.
 *  - It is not an insert-type call, so auto-compaction does not run.
 * Results.
 *  - It is a query-type call.
 *  - It invalidates the last results on entry, as apss_query_dev does, including when it fails afterwards.
 *  - apss_results_dev gives the query row within the batch.
 *  - apss_ext_ids_dev's d_query_ext gives the batch's ids.
 * Edge cases.
 *  - n == 0, an empty store, or nothing selected: APSS_OK, *n_rows = 0, *n_results = 0, apss_result_count answers 0.
 * Errors.
 *  - APSS_E_INVALID: NULL handle, n < 0, NULL ids with n > 0, n > 2^31 - 1.
 *  - APSS_E_UNSUPPORTED ("term shard"): a term shard.  It holds slices of rows.
 *  - apss_group has no such call: its members hold slices of rows (term ranges) or of the store (row ranges).
 *
 * The rows are selected and copied on the device and cross no ingest: the id list is sorted (rocprim radix sort), ONE pass over
 * the store's external ids selects (k_qs_select; it reads the marks only while rows are marked), one pass over the sorted list
 * counts (k_qs_ids), and a gather whose grid is sized by the rows SELECTED (k_qs_slots, k_qs_gather) writes them into the query
 * staging together with the batch summaries the probe plans with.  The call then takes the path apss_query_dev of the same rows
 * takes.  _dev: d_ext_ids int64[n] on the handle's device, read on the handle's stream.  Both forms synchronise that stream. */
typedef struct apss_stored_query_info {
  int32_t struct_size;     /* IN: caller's sizeof; OUT: bytes written (as apss_stats) */
  int32_t launches;        /* k_qs_* launches of the last apss_query_stored[_dev] (the id sort is not counted) */
  int64_t ids_given;       /* n */
  int64_t ids_distinct;    /* distinct ids in the list */
  int64_t ids_missing;     /* distinct ids with no LIVE stored row */
  int64_t rows_selected;   /* rows of the query batch */
  int64_t nnz_selected;    /* their entries */
  double select_ms, gather_ms; /* device time, HIP events */
} apss_stored_query_info;    /* 64 bytes */
int32_t apss_query_stored(apss_handle *h, int64_t n, const int64_t *ext_ids, int64_t *n_rows, int64_t *n_results);
int32_t apss_query_stored_dev(apss_handle *h, int64_t n, const int64_t *d_ext_ids, int64_t *n_rows, int64_t *n_results);
int32_t apss_stored_query_get(apss_handle *h, apss_stored_query_info *out);

/* ---- global top-K: a call's K best pairs, selected on the device ----
 * BASELINE.md's parity rule calls "top-k" the first k of the result set sorted by (-score, qId, cId): a cut over the WHOLE call,
 * where apss_set_top_k cuts every query row's own list.  Plain handles only.
 *
 * The setting.
 *  - k_pairs = 0 (the default): off.  A call launches nothing new, reads nothing new and allocates nothing.
 *  - k_pairs in 1 .. APSS_TOP_PAIRS_MAX: every query-type call made afterwards ends with the cut: apss_query[_dev],
 *    apss_insert_and_query[_dev], apss_self_join and apss_query_stored[_dev].
 *  - It may change at any time, takes effect at the next query-type call, leaves the last call's results alone and survives
 *    apss_clear, exactly like apss_set_top_k.
 * The order is total.  Ascending rank means:
 *  1. fp32 score descending, as the device reports it.  -0.0f counts as +0.0f and is reported as +0.0f (topk_key).
 *  2. Query external id ascending (signed int64).
 *  3. Candidate external id ascending.
 *  4. Query row within the batch ascending (two batch rows may carry one id).
 *  5. Candidate slot ascending.
 * The answer.
 *  - The final list is the first min(K, n) pairs of the call's final list (n pairs) in that order, stored in rank order.
 *  - Everything that reads the results sees it: n_results, apss_result_count, apss_fetch_results, apss_results_dev,
 *    apss_results_copy_dev, apss_stats.result_pairs.
 *  - With n <= K nothing is dropped, but the list is still put into rank order.
 *  - Score bits are unchanged.
 * Where the cut runs.  It is the last stage of the call:
 *  - after the join;
 *  - after k_rm_drop: a row marked removed never takes a place among the K;
 *  - after the per-query cut if k > 0: the K best are chosen among the kept per-query lists, and the global rank order
 *    replaces "grouped by query";
 *  - in a windowed call (apss_set_top_k_window) once, after the windows' lists are concatenated.
 *  - apss_topk_info, apss_topk_window_info, apss_topk_tile_cut_info and apss_removal_info keep reporting their own stages;
 *    apss_top_pairs_info.pairs_in is what they handed over.
 *  - The symmetric whole-store join is untouched: both directions of a pair are two pairs of the list.
 * Errors.
 *  - APSS_E_INVALID: NULL handle, k_pairs < 0 or > APSS_TOP_PAIRS_MAX.
 *  - APSS_E_UNSUPPORTED ("term shard"): k_pairs > 0 on a term shard.  Its candidates carry partial scores.
 *  - APSS_E_UNSUPPORTED from the query-type call: a final list of 2^32 pairs or more (the stage names a pair by 32 bits).
 *  - A failure inside the stage leaves the results invalid (APSS_E_STATE from the result calls).
 *  - apss_group has no such call: a group's final list lies behind its exchange, and this stage runs on one handle's stream.
 *
 * The stage reads the list where it lies (csrc/apss_top_pairs.hpp): a radix select over the 32-bit score key (k_tp_hist,
 * k_tp_pick; no host read between its passes), one collecting pass (k_tp_collect), a radix select down the ids for the pairs that
 * tie the K-th score -- one 32-bit index per tied pair is all it keeps of them, and a store of duplicates ties them all --
 * (k_tp_tie_hist, k_tp_tie_collect), then stable rocprim sorts over the min(K, n) kept pairs (k_tp_keys, k_tp_write).  It waits
 * for the handle's stream twice. */
#define APSS_TOP_PAIRS_MAX (1 << 20)
typedef struct apss_top_pairs_info {
  int32_t struct_size;   /* IN: caller's sizeof; OUT: bytes written (as apss_stats) */
  int32_t launches;      /* k_tp_* launches of the last query-type call (rocprim sorts not counted; 0: nothing ran) */
  int64_t k_pairs;       /* the setting the last call ran with (0: off) */
  int64_t pairs_in;      /* length of the call's final list before this cut */
  int64_t kept;          /* min(k_pairs, pairs_in) */
  int64_t above;         /* pairs whose score key is strictly above the K-th pair's (0 when nothing was cut) */
  int64_t tied;          /* pairs of the list that share the K-th pair's score key (0 when nothing was cut) */
  int64_t tied_kept;     /* kept - above (0 when nothing was cut) */
  double kth_score;      /* the K-th pair's fp32 score (0 when nothing was cut) */
  double select_ms;      /* device time of the whole stage, HIP events */
} apss_top_pairs_info;   /* 72 bytes */
int32_t apss_set_top_pairs(apss_handle *h, int64_t k_pairs);
int32_t apss_top_pairs_get(apss_handle *h, apss_top_pairs_info *out);

/* ---- near-duplicate groups: the connected components of the join, kept on the device ----
 * What a caller of near-duplicate detection wants is groups of items, not a list of pairs.  The maintained structure is the
 * connected components of the graph "stored row - stored row, edge = a pair of a call's final list".  It lives on the device, is
 * kept up to date across calls, and is read as one label per stored slot.  Plain handles only.  Default off: with the setting
 * off a call launches nothing new, reads nothing new and allocates nothing.
 *
 * Labels.
 *  - label[slot] is the smallest slot of the slot's component.  This is canonical: it does not depend on launch order, so a CPU
 *    union-find gives the same array.
 *  - A row marked removed has label -1.
 *  - apss_components_fetch writes, for slots [offset, offset + count), the label and the external id of the labelled slot.  For
 *    a removed row it writes -1 and the row's own id.  Either output pointer may be NULL.
 *  - apss_components_dev gives the device view int32[rows].  The view is valid until the next insert, query-type call, remove,
 *    compact, clear or apss_set_components.
 * State rules.
 *  - apss_set_components(h, 1) turns the structure on (given while it is on: starts it over).
 *    - Every stored slot becomes a singleton.
 *    - complete = 1 only on an empty store.
 *    - The setting survives apss_clear, which empties the structure and sets complete = 1.
 *  - apss_set_components(h, 0) frees the stage's buffers.
 *    - apss_components_dev and apss_components_fetch then answer APSS_E_STATE.
 *    - apss_components_get answers with on = 0, declined = APSS_CC_OFF.
 *  - Where the stage runs.
 *    - It runs behind k_rm_drop and before the per-query cut.
 *    - The graph is therefore every live pair at or above theta, whatever apss_set_top_k and apss_set_top_pairs keep of the list
 *      afterwards.
 *    - In a windowed call every window's list is absorbed before that window's cut.
 *    - The result list of the call is untouched, element by element.
 *  - Query row to slot.
 *    - slot_first + row when the batch is stored rows (apss_self_join, apss_insert_and_query[_dev]).
 *    - The selected slots for apss_query_stored[_dev].
 *    - Otherwise the call is declined with APSS_CC_OUTSIDE and changes nothing.
 *    - With APSS_FLAG_ADMISSION the batch rows that were not admitted have no slot: the mapping is taken from what the handle
 *      itself names as the batch (the rows it stored), not from the caller's row numbers.
 *  - apss_self_join resets to singletons, absorbs, and leaves complete = 1.
 *  - apss_insert_and_query[_dev] sets new slots to singletons, absorbs, and keeps complete as it was.
 *  - apss_query_stored[_dev] absorbs and keeps complete.  Its pairs are true edges.
 *  - apss_insert[_dev] and apss_insert_stored_dev set new slots to singletons and set complete = 0.  Their rows' edges were never
 *    seen.
 *  - A call declined with APSS_CC_TILE_CUT:
 *    - absorbs nothing (of a windowed call: nothing from its first window that cut on; what earlier windows gave are true edges);
 *    - sets complete = 0 if it stored rows;
 *    - resets to singletons with complete = 0 on a non-empty store if it is an apss_self_join.
 *  - apss_remove[_dev] that marks at least one row, and every compaction that discards rows (auto-compaction included): reset to
 *    singletons, complete = 0 unless the store is empty, resets + 1.  A removed row can split a component, and a compaction
 *    shifts slots.  (resets counts these and the resets a failed stage forces; a self-join's own fresh start is none.)
 *    The structure is never wrong about an edge: at every moment it is the components of a subset of the true live edges, and
 *    complete says whether it is all of them.
 *  - Errors.
 *    - APSS_E_INVALID: NULL handle, on outside {0, 1}, bad struct_size, a range outside [0, rows].
 *    - APSS_E_UNSUPPORTED ("term shard"): on = 1 on a term shard.
 *    - A HIP error inside the stage fails the call (APSS_E_DEVICE / APSS_E_NOMEM) and leaves the structure reset with
 *      complete = 0.
 *    - apss_group has no such call.
 * Cost.
 *  - The absorbing launches (k_cc_init over the new slots, k_cc_hook over the list) run on the handle's stream and read nothing
 *    back.  A query-type call gains no synchronisation.  (Growing the structure's arrays waits once, as growing the store does.)
 *  - Labels, counts and unions_total are produced lazily: at the first apss_components_get, _dev or _fetch after a change
 *    (k_cc_label, k_cc_count, ONE synchronisation).  A second read without a change launches nothing (label_launches says so).
 *  - Memory: two 32-bit words per slot of capacity, grown by half: at most 12 B per stored slot.  It is counted in
 *    apss_stats.hbm_bytes and freed by apss_set_components(h, 0). */
#define APSS_CC_RAN 0
#define APSS_CC_OFF 1        /* setting off */
#define APSS_CC_OUTSIDE 2    /* the batch was not rows of the store (apss_query[_dev]): nothing absorbed, nothing changed */
#define APSS_CC_TILE_CUT 3   /* the probe cut its rounds (apss_set_top_k_tile_cut applied): the list is not every pair */
typedef struct apss_components_info {
  int32_t struct_size;     /* IN: caller's sizeof; OUT: bytes written (as apss_stats) */
  int32_t on;
  int32_t complete;        /* 1: the structure has absorbed every pair >= theta among the live stored rows */
  int32_t declined;        /* APSS_CC_* of the last query-type call */
  int64_t rows;            /* slots labelled (apss_size rows) */
  int64_t rows_live;
  int64_t components;      /* among live rows, singletons included */
  int64_t singletons;
  int64_t largest;         /* rows of the largest component */
  int64_t pairs_absorbed;  /* pairs of the last query-type call handed to the stage */
  int64_t unions_total;    /* hooks that joined two components since the last reset: components == rows_live - unions_total */
  int64_t resets;          /* since create */
  double hook_ms;          /* device time of the last call's k_cc_hook launches, HIP events (known once the labels are next read) */
  double label_ms;         /* device time of the last labelling (k_cc_label, k_cc_count) */
  int32_t hook_launches;   /* of the last query-type call */
  int32_t label_launches;  /* of the last labelling (0: this read found the labels up to date) */
  int64_t reserved;        /* 0 */
} apss_components_info;    /* 112 bytes */
int32_t apss_set_components(apss_handle *h, int32_t on);
int32_t apss_components_get(apss_handle *h, apss_components_info *out);
int32_t apss_components_dev(apss_handle *h, const int32_t **d_label, int64_t *rows);
int32_t apss_components_fetch(apss_handle *h, int64_t offset, int64_t count, int32_t *out_label, int64_t *out_rep_ext);

/* ---- near-duplicate groups across a removal and a compaction: the repair ----
 * The rules above make apss_remove and apss_compact forget the groups: every slot becomes a singleton and only a whole-store
 * apss_self_join brings them back.  With the repair on, a removal re-joins the components it touched and nothing else, and a
 * compaction renumbers the forest instead of forgetting it.  Plain handles only.  Default off: with the setting off every call
 * launches, reads and allocates exactly what it does without this section.
 *
 * The setting.
 *  - apss_set_components_repair(h, max_rows): 0 is off.  1 .. 2^31 - 1 is the budget: the most live rows one apss_remove[_dev]
 *    may re-join.
 *  - It may change at any time and survives apss_clear.  It has no effect while apss_set_components is off.
 * What changes with the repair on (and apss_set_components on).
 *  - apss_remove[_dev] that newly marks at least one row, on the handle's stream behind the marking:
 *    - The forest is flattened, every marked slot flags its root, and every slot under a flagged root becomes a singleton again.
 *      The live ones among them, A rows, are the rows to re-join.  A is read back: one wait.
 *    - A = 0 (the marked rows were singletons): nothing is re-joined.  The last call's results stay fetchable, complete and resets
 *      are unchanged, declined = APSS_CCR_RAN.
 *    - 0 < A <= max_rows: the A rows are gathered and probed as the batch apss_query_stored of them would be, and their list goes
 *      behind k_rm_drop into the forest.  complete and resets stay as they were.  The re-join is a probe: the last call's results
 *      and query batch are gone afterwards (APSS_E_STATE, as after an insert), and apss_stats, apss_removal_info.pairs_dropped
 *      and apss_components_info.pairs_absorbed speak of the re-join.  Its list is wanted by the forest alone: neither
 *      apss_set_top_k nor apss_set_top_pairs cuts it, nothing of it is kept (apss_stats.result_pairs = 0), and
 *      apss_set_top_k_window bounds its memory as it bounds a call's.
 *    - A > max_rows: the rule without the repair -- reset to singletons, complete = 0 unless the store is empty, resets + 1 --
 *      and declined = APSS_CCR_BUDGET, budget_resets + 1.  A remove never costs more than the caller allowed.
 *    - A failure inside the stage fails the call and leaves the structure reset with complete = 0.  The marks stay: the removal
 *      happened.
 *  - Why complete may stay 1: a marked row is always a singleton once apss_remove returns.  A live edge with no end in a touched
 *    component is still in the forest; one with an end in a touched component has both ends there, both are re-joined, and the
 *    edge is in the re-join's list.  The labels are those of a fresh apss_self_join over the live rows.  A structure that was
 *    incomplete stays incomplete and stays never wrong about an edge.
 *  - apss_compact and auto-compaction renumber the forest: label and parent move with the rows to their new slots.  complete and
 *    resets stay, remaps + 1.  The insert that an auto-compaction precedes then follows its own rule above.
 *  - Errors.
 *    - APSS_E_INVALID: NULL handle, max_rows < 0 or > 2^31 - 1, bad struct_size.
 *    - APSS_E_UNSUPPORTED ("term shard"): the setter on a term shard.
 *    - apss_group has no such call. */
#define APSS_CCR_RAN 0
#define APSS_CCR_OFF 1            /* this setting off */
#define APSS_CCR_NO_COMPONENTS 2  /* apss_set_components off */
#define APSS_CCR_BUDGET 3         /* more rows to re-join than max_rows: reset to singletons */
#define APSS_CCR_NOTHING 4        /* nothing newly marked: nothing launched */
typedef struct apss_components_repair_info {
  int32_t struct_size;         /* IN: caller's sizeof; OUT: bytes written (as apss_stats) */
  int32_t declined;            /* APSS_CCR_* of the last apss_remove[_dev].  While that call (or no call yet) marked no row, the getter
                                  answers from the settings as they are now: OFF, NO_COMPONENTS or NOTHING */
  int64_t max_rows;            /* the setting (0: off) */
  int64_t rows_marked;         /* rows newly marked by that call */
  int64_t components_touched;  /* components that held a newly marked row */
  int64_t rows_rejoined;       /* live rows taken apart and re-joined */
  int64_t pairs_rejoined;      /* length of the list the re-join absorbed */
  int64_t repairs;             /* since create: removes that ran the stage */
  int64_t budget_resets;       /* since create: removes declined with APSS_CCR_BUDGET */
  int64_t remaps;              /* since create: compactions that renumbered the forest */
  double detach_ms;            /* device time of flatten, touch, detach and the scans of that call, HIP events */
  double rejoin_ms;            /* device time of its gather and probe */
  double remap_ms;             /* device time of the last compaction's flatten and renumbering */
  int32_t launches;            /* kernel launches of that call's repair stage, its scans and gather included, the re-join's probe not
                                  (apss_stats has it) */
  int32_t reserved0;           /* 0 */
} apss_components_repair_info; /* 104 bytes */
int32_t apss_set_components_repair(apss_handle *h, int64_t max_rows);
int32_t apss_components_repair_get(apss_handle *h, apss_components_repair_info *out);


/* =====================================================================================================================
 * apss_group: the sharded index of one node -- T term ranges x D row ranges of member shards, one per GPU -- behind ONE
 * object (apss_group_create: T x 1, every member holds its slice of every row; apss_group_create_grid: T x D, below).
 *
 * The reference shards its inverted index by term inside the server: WriteWorkerActor buckets every vector by
 * dim % maxShardNum and flushes one DataPacket per shard (WriteWorkerActor.scala:164-183), EntryProxyActor fans a packet out
 * to maxIndexEntryActorNum IndexingWorkerActors by dim % maxIndexEntryActorNum (EntryProxyActor.scala:37-49), and every
 * worker handles IndexData on its own (IndexingWorkerActor.scala:122-137), re-scoring the full vectors it was sent.  A group
 * is that fan-out and its workers on the GPUs of one node: member g owns a contiguous term RANGE (cut on the first batch,
 * balanced by sum df^2; re-cut as the store grows with APSS_GROUP_ADAPT_LAYOUT), stores only that slice of every vector
 * and runs the member-local phase of the join; the group
 * combines the members' answers with the exchange the reference does not need because it replicates whole vectors:
 *
 *   1. every member, concurrently (one host thread per member): apss_insert_and_query_dev / apss_query_dev on its shard
 *      handle -> CANDIDATE pairs (the shard rule above apss_partial_scores_dev);
 *   2. all-gather of the members' candidate lists (8-B keys), sorted union on every member;
 *   3. every member: exact partial score of every pair of the union (apss_partial_scores_dev);
 *   4. all-reduce(SUM) of the partial scores, `>= theta` (IWA:93), compaction on member 0.
 *
 * Exchange (steps 2 and 4): RCCL over xGMI (ncclBroadcast-grouped all-gather, ncclAllReduce on the members' streams; librccl
 * is loaded on first use) when every member has a GPU of its own; members that SHARE a device (tests on a one-GPU box) are
 * combined by device-to-device copies and a summing kernel -- same lists, same order, same results.
 * On skewed data the members share one dense-head block (apss_set_head_terms): member 0's device runs the library's policy
 * on a sample of the first batch and every member is given the same terms; apss_config.head_terms = -1 disables it.
 *
 * One thread at a time inside a group (it is one actor's state); results stay in the group until the next query-type
 * call, insert or clear.  apss_config: dim, theta, index_threshold, flags, tile_rows, head_terms and the capacity hints
 * apply to every member; device_id, term_lo, term_hi are ignored (the group sets them).  APSS_FLAG_ADMISSION is not
 * supported with more than one member and a dense-head block (as on a single shard handle).
 *
 * GRIDS (apss_group_create_grid): the reference shards on two levels (WriteWorkerActor.scala:164-183 by dim % maxShardNum,
 * EntryProxyActor.scala:37-49 by dim % maxIndexEntryActorNum); the second level here is D ROW ranges.  Member (j, i) = row
 * range j, term range i holds term range i of the rows of row range j; the T members of a row range are a term-sharded
 * group of their own (steps 1-4 above run inside a row range, the row ranges never wait for each other), the term cuts and
 * the dense head are shared by all row ranges.  The answer of every call is the list a single plain handle gives.
 *   rows: a batch of n rows is cut into D contiguous spans, span k = [ceil(n k / D), ceil(n (k + 1) / D)); span k goes to row
 *     range (first + k) mod D, first = the row range holding the fewest rows when the call starts (lowest index on ties) --
 *     single vectors fill the ranges round-robin, equal batches divisible by D keep them exactly equal.
 *   insert: row range j inserts its span.  query (frozen index): every row range is asked the whole batch; the lists are
 *     disjoint by candidate and are concatenated.
 *   insert-and-query, row range j: OWN phase = insert_and_query of its span (pairs of the span with the range's store and
 *     itself), then OUTSIDE phase = ONE query of the other spans' whole rows, concatenated in span order, against the range's
 *     store + span.  When every row range was empty at the start of the call (a whole-store join) the symmetry is used ACROSS
 *     the row ranges: range j meets only the (D - 1) / 2 ranges before it (cyclically; for even D also the opposite range
 *     when j is the lower of the two) and every pair it finds is reported in both directions -- unless
 *     APSS_GROUP_NO_SYMMETRIC_RANGES or APSS_FLAG_NO_SYMMETRY is set.  On a non-empty store every cell meets all other spans
 *     and nothing is mirrored.
 *   results: (query ext id, candidate ext id, score) triples are gathered on each row range's first device after each phase;
 *     the group's list is their concatenation over the row ranges.
 *   exchange: RCCL (one communicator per row range) when in every row range the T members have a device each, copies
 *     otherwise; T = 1: none, a row range's answer is final.
 *   not supported with D > 1 (APSS_E_UNSUPPORTED): APSS_GROUP_ADAPT_LAYOUT and apss_group_relayout.
 * ===================================================================================================================== */
typedef struct apss_group apss_group;

#define APSS_GROUP_FORCE_EXCHANGE 1u /* run the exchange (steps 2-4) even for a group of ONE member, whose handle holds the whole
                                        term space and whose answer is already final (test hook: the RCCL path on one GPU) */
#define APSS_GROUP_NO_RCCL 2u        /* never load RCCL: combine the members with device-to-device copies (peer access or staging
                                        through the host) even when every member has its own GPU */
#define APSS_GROUP_ADAPT_LAYOUT 4u   /* re-decide the layout as the store grows: before an insert-type call that brings the store to
                                        max(1024, 2 x layout_rows) rows, cuts and head are decided again on the store plus the
                                        batch and the store is rebuilt in the new layout (apss_group_relayout) */

#define APSS_GROUP_NO_SYMMETRIC_RANGES 8u /* grids: every cell meets every other row range (no mirroring) */

#define APSS_EXCHANGE_NONE 0   /* one member, its answer is final */
#define APSS_EXCHANGE_COPIES 1 /* device-to-device copies + summing kernel (members share a device, or APSS_GROUP_NO_RCCL) */
#define APSS_EXCHANGE_RCCL 2   /* RCCL collectives on the members' streams */

#define APSS_GROUP_MAX_MEMBERS 64

typedef struct apss_group_stats {
  int32_t struct_size;        /* IN: sizeof(apss_group_stats) of the caller; OUT: bytes written (as apss_stats) */
  int32_t n_members;
  int32_t exchange;           /* APSS_EXCHANGE_* the last query-type call used */
  int32_t head_terms;         /* terms in the members' shared dense-head block (0: none) */
  int64_t rows;               /* vectors in the store (every member holds its slice of each) */
  int64_t nnz;                /* postings over all members */
  int64_t posting_visits;     /* sum over the members, last query-type call (reference-equivalent: see apss_stats) */
  int64_t device_posting_visits;
  int64_t member_touched_pairs; /* sum over the members of apss_stats.candidate_pairs (a pair sharing terms in k ranges counts k times) */
  int64_t candidates_sum;     /* sum over the members of the candidate lists' lengths (step 1) */
  int64_t candidates_max;     /* ... the longest list */
  int64_t union_pairs;        /* distinct candidates (step 2) */
  int64_t result_pairs;       /* pairs >= theta */
  int64_t all_gather_bytes;   /* bytes every member RECEIVES in step 2: 8 x (candidates_sum - its own) at most */
  int64_t all_reduce_bytes;   /* 4 x union_pairs: the vector of step 4 */
  double member_ms_max;       /* wall time of step 1, slowest member (ingest + build + filter kernels + their syncs) */
  double probe_ms_max;        /* apss_stats.probe_ms, slowest member */
  double build_ms_max;
  double head_ms_max;
  double exchange_ms;         /* wall time of steps 2-4 (gather, union, partial scores, reduce, threshold) */
  double partial_ms_max;      /* ... of which apss_partial_scores_dev, slowest member */
  double total_ms;            /* wall time of the call */
  int32_t term_cuts[APSS_GROUP_MAX_MEMBERS + 1]; /* member g owns terms [term_cuts[g], term_cuts[g + 1]) (head terms excepted) */
} apss_group_stats;

/* the group's layout and the history of its re-layouts (apss_group_layout_get; struct_size as apss_stats) */
typedef struct apss_group_layout {
  int32_t struct_size;        /* IN: sizeof(apss_group_layout) of the caller; OUT: bytes written */
  int32_t n_members;
  int64_t layout_rows;        /* store rows (plus the batch that triggered it) the current layout was decided on */
  int64_t next_eval_rows;     /* APSS_GROUP_ADAPT_LAYOUT: an insert-type call that brings the store to this many rows re-decides
                                 (0: the flag is off, or nothing about the layout can change) */
  int64_t evaluations;        /* layout decisions since create, the first batch's excepted (schedule checks and apss_group_relayout) */
  int64_t relayouts;          /* ... of those, the ones that rebuilt the store (the decision differed from the layout in place) */
  double last_relayout_ms;    /* wall time of the last evaluation (decision + rebuild) */
  double total_relayout_ms;   /* ... summed over every evaluation */
  int64_t relayout_bytes;     /* bytes copied between the members' devices to reassemble whole rows, in total */
  int32_t head_terms;         /* terms of the shared dense-head block (0: none) */
  int32_t term_cuts[APSS_GROUP_MAX_MEMBERS + 1];
  double dfsq[APSS_GROUP_MAX_MEMBERS]; /* per member: sum of df^2 over the stored rows' tail terms in its range (what the
                                          balanced cuts even out), computed on the device at this call */
} apss_group_layout;

/* what the row ranges of a grid did in the last call (apss_group_grid_get; struct_size as apss_stats).  On a grid
 * apss_group_stats.n_members is T x D, term_cuts has T + 1 entries, the sums run over all members and both phases (a member's
 * posting_visits as its handle reports them, the outside phase counted twice when its pairs were mirrored: what the
 * reference's two-directional probe visits), exchange_ms is the slowest row range's; apss_group_member_stats(g, j * T + i)
 * addresses member (j, i) */
typedef struct apss_group_grid {
  int32_t struct_size;        /* IN: sizeof(apss_group_grid) of the caller; OUT: bytes written */
  int32_t n_term_ranges;      /* T */
  int32_t n_row_ranges;       /* D */
  int32_t symmetric_ranges;   /* 1: the last query-type call met half of the other row ranges per cell and mirrored */
  int64_t rows_in_range[APSS_GROUP_MAX_MEMBERS]; /* rows held by row range j */
  int64_t outside_rows_max;   /* rows of the longest outside batch a cell met in the last call */
  int64_t mirrored_pairs;     /* results of the last call that are mirrors of a pair found in the other direction */
  double own_ms_max;          /* wall time of the own phase, slowest row range */
  double outside_ms_max;      /* ... of the outside phase */
} apss_group_grid;

/* n_members >= 1 shards on the HIP devices device_ids[0 .. n_members) (a device may appear more than once);
 * = apss_group_create_grid(cfg, n_members, 1, ...) */
int32_t apss_group_create(const apss_config *cfg, int32_t n_members, const int32_t *device_ids, uint32_t group_flags,
                          apss_group **out);
/* T = n_term_ranges term ranges x D = n_row_ranges row ranges; member (j, i) = row range j, term range i,
 * lives on device_ids[j * T + i]; T * D <= APSS_GROUP_MAX_MEMBERS */
int32_t apss_group_create_grid(const apss_config *cfg, int32_t n_term_ranges, int32_t n_row_ranges,
                               const int32_t *device_ids, uint32_t group_flags, apss_group **out);
int32_t apss_group_grid_get(apss_group *g, apss_group_grid *out);
void apss_group_destroy(apss_group *g);
/* message of the last failing call ("" if none); g == NULL: last apss_group_create failure */
const char *apss_group_last_error(const apss_group *g);
/* Name the term ranges instead of letting the first batch decide: cuts[0] = 0 < cuts[1] < .. < cuts[T] = dim (T = n_members
 * of apss_group_create, n_term_ranges of a grid).
 * Before the group's first insert only (the members' handles are created with their ranges then). */
int32_t apss_group_set_term_cuts(apss_group *g, const int32_t *cuts);

/* host-pointer entry points (what the JNI shim binds): the CSR batch of apss_insert / apss_query / apss_insert_and_query,
 * handed WHOLE to every member (each keeps its term range) */
int32_t apss_group_insert(apss_group *g, int64_t n, const int64_t *rowptr, const int32_t *indices, const double *values,
                          const int64_t *ext_ids);
int32_t apss_group_query(apss_group *g, int64_t n, const int64_t *rowptr, const int32_t *indices, const double *values,
                         const int64_t *ext_ids, int64_t *n_results);
int32_t apss_group_insert_and_query(apss_group *g, int64_t n, const int64_t *rowptr, const int32_t *indices,
                                    const double *values, const int64_t *ext_ids, int64_t *n_results);
/* device-pointer entry point: member m reads the batch from d_rowptr[m], d_indices[m], d_values[m], d_ext_ids[m], resident
 * on ITS device (members that share a device may be given the same pointers); layouts as apss_insert_and_query_dev.  On a
 * grid every member is handed the WHOLE batch (m = j * T + i) and cuts its row range's span and outside batch out of it on
 * its device */
int32_t apss_group_insert_and_query_dev(apss_group *g, int64_t n, int64_t nnz, const int64_t *const *d_rowptr,
                                        const int32_t *const *d_indices, const float *const *d_values,
                                        const int64_t *const *d_ext_ids, int64_t *n_results);
/* drop index and store of every member; the reservations and the LAYOUT stay -- term cuts and dense-head terms, whether named
 * by the caller or decided from the batches so far, and layout_rows (they are configuration, like apss_set_head_terms on a
 * handle: a benchmark step re-runs build + join on the same layout and does not re-layout).  A new layout comes from
 * apss_group_relayout, from APSS_GROUP_ADAPT_LAYOUT as the store grows, or from a new group */
int32_t apss_group_clear(apss_group *g);
/* Re-decide the layout now, from the stored rows.  cuts == NULL: term cuts balanced by sum df^2 over the store's tail terms
 * (equal widths below 1024 rows) unless they were named (apss_group_set_term_cuts), and the dense head from the library's
 * policy on a sample of up to 131072 whole rows; non-NULL: these cuts (the contract of apss_group_set_term_cuts) and only the
 * head is re-decided (the next schedule check or NULL call may cut again, unless cuts were named before the first insert).  A layout that differs from the one in place is BUILT, then
 * swapped: the members' slices are reassembled into whole rows on every device that holds a member, new member handles are
 * filled from them (apss_insert_stored_dev) and only when every member succeeded are the old ones destroyed -- so for a
 * moment each member's store exists twice.  A failure leaves the old layout and store untouched and returns the member's
 * error.  The results of the last query-type call are gone afterwards.  APSS_E_STATE on a group without rows;
 * APSS_E_UNSUPPORTED on a grid with more than one row range (the group is left as it is). */
int32_t apss_group_relayout(apss_group *g, const int32_t *cuts);
int32_t apss_group_layout_get(apss_group *g, apss_group_layout *out);

int32_t apss_group_result_count(const apss_group *g, int64_t *n_results);
/* (query ext id, candidate ext id, score) of the last query-type call, as apss_fetch_results */
int32_t apss_group_fetch_results(apss_group *g, int64_t offset, int64_t count, int64_t *out_q, int64_t *out_c,
                                 float *out_score);
int32_t apss_group_stats_get(apss_group *g, apss_group_stats *out);
/* the shard handle's own statistics (out->struct_size set by the caller, as apss_stats_get) */
int32_t apss_group_member_stats(apss_group *g, int32_t member, apss_stats *out);

/* Per-query top-k for the group's query-type calls (semantics: apss_set_top_k).  One member without an exchange: the member's
 * handle cuts its own final list.  T x 1 with an exchange: the cut runs on member 0's device behind the `>= theta` compaction
 * of step 4 (the members are term shards and never get a k).  GRIDS with D > 1 row ranges keep (ext, ext, score) triples per
 * row range on different devices: k > 0 answers APSS_E_UNSUPPORTED there and the group keeps working with k = 0.  May be called
 * before the first insert (the members' handles do not exist yet: the setting is applied when they are created). */
int32_t apss_group_set_top_k(apss_group *g, int32_t k);
int32_t apss_group_topk_get(apss_group *g, apss_topk_info *out);

#ifdef __cplusplus
}
#endif
#endif /* APSS_H */
