// apss_build.hpp -- the kernels of the index build (IWA:61-71): CSR rows of the store -> per-tile posting lists.  Four forms
// of count + scatter around one segment scan (k_tile_scan_part / k_tile_scan_place): global atomics (k_tile_hist, k_tile_scatter,
// and k_tile_shift for an append), streaming LDS (k_tile_*_lds), run-reading LDS (k_row_cuts, k_tile_runs, k_tile_place_sub) and
// the bucketed LDS build of large dims (k_bucket_pass).  Which one a build takes is apss_build_plan.hpp's decision; the host
// stages that launch them are build_tiles' (apss_hip.hip).  The probe kernels read what is packed here (pack_coarse*, kSegAlign*).
// A SECTION of apss_kernels.hpp, which includes it behind what it needs (kWave, kGroup, Posting, the block scan) and ahead of the
// probe kernels: include that header, never this one by itself.
#pragma once
#include "apss_build_plan.hpp"

namespace apss {

// ---------------------------------------------------------------------------------------------------------
// index build (IWA:61-71): for rows [row0, row1) of the store, fill the posting lists of their tiles.
// tile_seg[T][t] = {first posting, length} of term t in tile T, relative to the tile's posting base.  Every
// segment starts on a 128-B boundary (a multiple of kSegAlign postings): an L2 line then never straddles two
// segments, which cut the probe's memory-side traffic by a quarter (profiles/r01_summary.md).
// k_tile_hist counts lengths into .y; k_tile_scan turns them into aligned starts (.x) and clears .y;
// k_tile_scatter's cursor increments rebuild .y while placing the postings.
constexpr int kSegAlign = 16;   // exact index: 16 postings of 8 B = one 128-B line
constexpr int kSegAlignC = 32;  // coarse index: 32 postings of 4 B = one 128-B line

// coarse posting: u16 slot field | fp16 weight << 16 (4 B).  Read only by the coarse filter pass; every pair it
// lets through is re-scored from the fp32 store.  In tiles of <= 32768 rows the slot field holds slot * 2 = the LDS byte
// offset of the candidate's 16-bit accumulator (one AND gives the atomic's word address, one shift its half).
__device__ __forceinline__ uint32_t pack_coarse(uint32_t slot, float w) {
  // never the zero word: zero marks padding and idle lanes in the probe (a weight below fp16's range becomes its
  // smallest subnormal, which errs upward: safe for a filter)
  return (slot & 0xffffu) | (max((uint32_t)__half_as_ushort(__float2half_rn(w)), 1u) << 16);
}

// wide coarse posting (tiles of up to 131072 rows, 8-bit accumulators): slot << 15 | fp16 weight without its sign bit
// (weights are non-negative on this path); never the zero word either
__device__ __forceinline__ uint32_t pack_coarse_wide(uint32_t slot, float w) {
  return (slot << 15) | max((uint32_t)__half_as_ushort(__float2half_rn(w)) & 0x7fffu, 1u);
}

struct BuildArgs {
  const int64_t *rowptr;
  const int32_t *idx;             // term of every entry (a handle with a dense-head block builds from its tail view: apss_head.hpp)
  const float *val;
  int64_t row0, row1;
  int32_t cb;
  int32_t dim;
  uint2 *tile_seg;
  int64_t seg_stride;             // dim
  const int64_t *tile_post_base;  // [n_tiles + 1] first posting of each tile in `post`
  Posting *post;                  // exact format (8 B) ...
  uint32_t *post_c;               // ... or coarse format (4 B), when `coarse`
  int32_t coarse;
  int32_t coarse_shift;           // 1: the slot field holds slot * 2, the byte offset of the 16-bit accumulator (tiles <= 32768 rows)
  int32_t seg_align;              // postings per aligned unit (kSegAlign / kSegAlignC)
  int32_t coarse_wide;            // 1: pack_coarse_wide (17-bit slots)
  const uint32_t *erow;           // store row of every entry (LDS build)
  const float *row_scale;         // shard rule (coarse rendering): row r's weights are stored divided by row_scale[r] = |x_g| / |x|,
                                  //   so that the filter's threshold does not depend on the candidate (null: as they are)
  int32_t range_terms;            // terms per range of the LDS build's (tile, range) workgroups: 0 = kBuildRange; the bucketed build
                                  //   of large dims names its own (8192: measured)
  const int64_t *ent_base;        // LDS build over BUCKETED entries (dims of more than kBuildMaxRanges ranges): workgroup w = (tile, range)
                                  //   reads entries [ent_base[w], ent_base[w + 1]) of idx / erow / val, which then point at the
                                  //   bucketed copies (k_bucket_scatter); null: the tile's entries as they lie in the store
  const uint32_t *run_cut;        // run-reading LDS build (k_row_cuts): [row1 - row0][n_ranges + 1], see there
  int32_t term_lo, term_hi;       // the handle's term range: a (tile, range) workgroup outside it has nothing to read
  // ... in two passes (k_tile_runs<kRunPartition>): the entries of a (tile, range) are first partitioned into SUB-ranges of
  // 2^sub_shift terms -- bucket (tile - tile0) * n_sub + term >> sub_shift of o_ent, sizes from the histogram (sub_cnt),
  // starts from their scan (sub_base) -- and k_tile_place_sub then places them sub-range by sub-range
  int32_t sub_shift, n_sub;
  unsigned long long *sub_cnt;
  const int64_t *sub_base;
  uint2 *o_ent;                   // {term, finished posting word}: one 8-B store per entry (coarse renderings)
};

// one wave per row: coalesced reads of the row's entries
__global__ void k_tile_hist(BuildArgs a) {
  const int64_t row = a.row0 + ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int lane = threadIdx.x % kWave;
  if (row >= a.row1) return;
  uint2 *sg = a.tile_seg + (row / a.cb) * a.seg_stride;
  const int64_t b = a.rowptr[row], e = a.rowptr[row + 1];
  for (int64_t k = b + lane; k < e; k += kWave) {
    const int32_t t = a.idx[k];
    if ((uint32_t)t < (uint32_t)a.dim) atomicAdd(&sg[t].y, 1u);
  }
}

// Exclusive scan of a tile's aligned segment lengths -> segment starts; tile_total[tile] = postings incl. padding.  Two
// launches over (tile, block of kScanBlock terms) workgroups: k_tile_scan_part leaves every block's sum (and the build's
// statistics), k_tile_scan_place adds up the sums of the blocks before its own and writes the starts.  (One workgroup per
// tile walking its dim entries block after block took 85 us at dim = 100k whatever the number of tiles -- 25 dependent
// trips -- which a streamed batch paid on every append to the last tile; a block per workgroup is one trip.)
__global__ __launch_bounds__(1024) void k_tile_scan_part(const uint2 *tile_seg, int64_t seg_stride, int32_t dim, int64_t tile0,
                                                         int32_t n_blk, uint32_t align, uint32_t *part, uint32_t *max_len,
                                                         unsigned long long *chunk_w, uint32_t count_long) {
  __shared__ uint32_t wave_tot[17];
  const int64_t tile = tile0 + blockIdx.x / n_blk;
  const int32_t blk = (int32_t)(blockIdx.x % n_blk);
  const uint2 *sg = tile_seg + tile * seg_stride;
  const int tid = threadIdx.x;
  const int32_t i0 = blk * kScanBlock + tid * 4;
  uint32_t s = 0, longest = 0, n_long = 0;
  unsigned long long cw = 0;  // sum over the tile's short segments of length x 16-posting chunks
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t len = i0 + k < dim ? sg[i0 + k].y : 0u;
    s += (len + align - 1) / align * align;
    longest = max(longest, len);
    n_long += len > 256u ? 1u : 0u;  // (kLongLenW: what the probe kernels sweep as a long segment)
    cw += len <= 256u ? (unsigned long long)len * ((len + 15u) / 16u) : 0ull;
  }
  uint32_t total;
  (void)block_excl_scan_1024<uint32_t>(s, wave_tot, &total);
  if (tid == 0) part[blockIdx.x] = total;
  // the longest (tile, term) segment of the build: tells the probe whether its long-segment machinery is needed at all.
  // Combined per workgroup first (LDS), then ONE global atomic each per workgroup: same-address global atomics are serialised
  // at the memory side (a wave-level atomic per statistic made this kernel 215 us over 31 tiles x 25 blocks)
  __shared__ uint32_t sh_long[2];
  __shared__ unsigned long long sh_cw;
  if (tid == 0) {
    sh_long[0] = sh_long[1] = 0u;
    sh_cw = 0ull;
  }
  __syncthreads();
  for (int o = kWave / 2; o; o >>= 1) {
    longest = max(longest, (uint32_t)__shfl_xor((int)longest, o));
    n_long += (uint32_t)__shfl_xor((int)n_long, o);
  }
  // A row of the tile holds term t with probability len_t / rows, and a query holding t meets ceil(len_t / 16) chunks of this
  // tile: sum_t len_t * ceil(len_t / 16) / rows = the chunks an average round (a query distributed like the tile's rows) deals
  // out, whatever the term distribution -- what the probe sizes its register window from
  for (int o = kWave / 2; o; o >>= 1) cw += __shfl_xor(cw, o);
  if ((tid % kWave) == 0) {
    if (longest) atomicMax(&sh_long[0], longest);
    if (n_long) atomicAdd(&sh_long[1], n_long);
    if (cw) atomicAdd(&sh_cw, cw);
  }
  __syncthreads();
  if (tid == 0) {
    if (max_len && sh_long[0]) {
      atomicMax(max_len, sh_long[0]);
      if (sh_long[1] && count_long) atomicAdd(max_len + 1, sh_long[1]);  // [1]: long segments over all tiles of the build (an appended-to tile was counted before)
    }
    if (chunk_w && sh_cw) atomicAdd(chunk_w, sh_cw);
  }
}

__global__ __launch_bounds__(1024) void k_tile_scan_place(uint2 *tile_seg, int64_t seg_stride, int32_t dim, int64_t tile0, int32_t n_blk,
                                                          uint32_t align, uint32_t keep_len, const uint32_t *part, int64_t *tile_total) {
  __shared__ uint32_t wave_tot[17];
  __shared__ uint32_t before;
  const int64_t tile = tile0 + blockIdx.x / n_blk;
  const int32_t blk = (int32_t)(blockIdx.x % n_blk);
  uint2 *sg = tile_seg + tile * seg_stride;
  const int tid = threadIdx.x;
  // the sums of this tile's blocks before this one
  uint32_t mine = 0u;
  for (int32_t j = tid; j < blk; j += 1024) mine += part[(blockIdx.x / n_blk) * n_blk + j];
  uint32_t tot_before;
  (void)block_excl_scan_1024<uint32_t>(mine, wave_tot, &tot_before);
  if (tid == 0) before = tot_before;
  __syncthreads();  // (wave_tot is reused below)
  const uint32_t carry = before;
  const int32_t i0 = blk * kScanBlock + tid * 4;
  uint32_t len[4], s = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    len[k] = i0 + k < dim ? sg[i0 + k].y : 0u;
    s += (len[k] + align - 1) / align * align;
  }
  uint32_t total;
  uint32_t run = carry + block_excl_scan_1024<uint32_t>(s, wave_tot, &total);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    // (the atomic scatter rebuilds .y as its cursor, the LDS scatter never touches it)
    if (i0 + k < dim) sg[i0 + k] = make_uint2(run, keep_len ? len[k] : 0u);
    run += (len[k] + align - 1) / align * align;
  }
  if (blk == n_blk - 1 && tid == 0) tile_total[tile] = (int64_t)carry + (int64_t)total;
}

__global__ void k_tile_scatter(BuildArgs a) {
  const int64_t row = a.row0 + ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
  const int lane = threadIdx.x % kWave;
  if (row >= a.row1) return;
  const int64_t tile = row / a.cb;
  uint2 *sg = a.tile_seg + tile * a.seg_stride;
  const int64_t pbase = a.tile_post_base[tile];
  const uint32_t local = (uint32_t)(row - tile * a.cb);
  const int64_t b = a.rowptr[row], e = a.rowptr[row + 1];
  for (int64_t k = b + lane; k < e; k += kWave) {
    const int32_t t = a.idx[k];
    if ((uint32_t)t >= (uint32_t)a.dim) continue;
    // one 64-bit returning atomic on {start, cursor}: bumps the cursor (high word) and brings the start along
    const unsigned long long old = atomicAdd(reinterpret_cast<unsigned long long *>(&sg[t]), 1ull << 32);
    const uint32_t pos = (uint32_t)old + (uint32_t)(old >> 32);
    if (a.coarse) {
      const float sc = a.row_scale ? a.row_scale[row] : 1.0f;
      const float wv_ = sc > 0.f ? a.val[k] / sc : a.val[k];
      a.post_c[pbase + pos] = a.coarse_wide ? pack_coarse_wide(local, wv_) : pack_coarse(local << a.coarse_shift, wv_);
    } else {
      Posting p;
      p.slot = local;
      p.w = a.val[k];
      a.post[pbase + pos] = p;
    }
  }
}

// APPEND build (a streamed batch lands in the last, partly filled tile: IndexingWorkerActor.scala:61-71 appends to its posting
// lists): the new rows' terms are counted ON TOP of the tile's segment lengths (k_tile_hist over the new rows only), the scan
// gives every segment its new start -- a segment only ever grows, the ones behind it move right --, this kernel moves the
// tile's old postings from a scratch copy to their new places and leaves every cursor behind them, and k_tile_scatter places
// the new rows' postings after them.  Work: the new rows + one pass over the tile's postings, instead of recounting and
// re-scattering every row of the tile with two global atomics each.  16 lanes per term.
struct ShiftArgs {
  const uint2 *seg_old;   // [dim] {start, length} before the append (scratch copy)
  uint2 *seg_new;         // [dim] {new start, 0} from k_tile_scan; .y becomes the old length (the scatter's cursor)
  const uint32_t *old_c;  // the tile's old postings (scratch copy, offsets relative to the tile), coarse ...
  const Posting *old_x;   // ... or exact
  uint32_t *new_c;        // the tile's region in the posting array
  Posting *new_x;
  int32_t dim;
};
__global__ void k_tile_shift(ShiftArgs a) {
  const int64_t t = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup;
  const int gl = threadIdx.x % kGroup;
  if (t >= a.dim) return;
  const uint2 o = a.seg_old[t];
  const uint32_t n0 = a.seg_new[t].x;
  if (a.old_c) {
    for (uint32_t i = gl; i < o.y; i += kGroup) a.new_c[n0 + i] = a.old_c[o.x + i];
  } else {
    for (uint32_t i = gl; i < o.y; i += kGroup) a.new_x[n0 + i] = a.old_x[o.x + i];
  }
  if (gl == 0) a.seg_new[t].y = o.y;
}

// ---------------------------------------------------------------------------------------------------------
// LDS index build, for dims of at most kBuildMaxRanges ranges of kBuildRange terms: one workgroup per (tile, term range)
// streams the tile's entries and keeps the range's counters / cursors in LDS, so the 2 x 1e8 global atomics of
// k_tile_hist / k_tile_scatter (2.7e10/s on this part, whatever their scope) become LDS atomics.  Each range re-reads
// the tile's entries, which is why large dims (C5: 1M terms = 31 ranges) stay with the global-atomic kernels.
// These STREAMING kernels are what a build of ONE range takes (every entry is read once, coalesced), what the bucketed
// build of large dims runs over its buckets, and what APSS_DEBUG=build_stream keeps; with two ranges or more the
// run-reading kernels below read a tile's entries once instead of once per range.
__global__ __launch_bounds__(1024) void k_tile_hist_lds(BuildArgs a, int64_t tile0, int32_t n_ranges) {
  __shared__ uint32_t cnt[kBuildRange];
  const int tid = threadIdx.x;
  const int64_t tile = tile0 + blockIdx.x / n_ranges;
  const int32_t rt = a.range_terms ? a.range_terms : kBuildRange;
  const int32_t lo = (int32_t)(blockIdx.x % n_ranges) * rt;
  const uint32_t span = (uint32_t)(min(a.dim, lo + rt) - lo);
  for (int i = tid; i < rt; i += 1024) cnt[i] = 0u;
  __syncthreads();
  const int64_t rA = tile * a.cb, rB = min(a.row1, rA + (int64_t)a.cb);
  const int64_t eA = a.ent_base ? a.ent_base[blockIdx.x] : a.rowptr[rA], eB = a.ent_base ? a.ent_base[blockIdx.x + 1] : a.rowptr[rB];
  for (int64_t k = eA + tid; k < eB; k += 4096) {  // four loads in flight per thread
    int32_t t[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = k + 1024 * j < eB ? a.idx[k + 1024 * j] : -1;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if ((uint32_t)(t[j] - lo) < span) atomicAdd(&cnt[t[j] - lo], 1u);
  }
  __syncthreads();
  uint2 *sg = a.tile_seg + tile * a.seg_stride + lo;
  for (uint32_t i = tid; i < span; i += 1024) sg[i] = make_uint2(0u, cnt[i]);
}

__global__ __launch_bounds__(1024) void k_tile_scatter_lds(BuildArgs a, int64_t tile0, int32_t n_ranges) {
  __shared__ uint32_t cur[kBuildRange];
  const int tid = threadIdx.x;
  const int64_t tile = tile0 + blockIdx.x / n_ranges;
  const int32_t rt = a.range_terms ? a.range_terms : kBuildRange;
  const int32_t lo = (int32_t)(blockIdx.x % n_ranges) * rt;
  const uint32_t span = (uint32_t)(min(a.dim, lo + rt) - lo);
  const uint2 *sg = a.tile_seg + tile * a.seg_stride + lo;
  for (uint32_t i = tid; i < span; i += 1024) cur[i] = sg[i].x;  // cursor = segment start: the atomic returns the position
  __syncthreads();
  const int64_t pbase = a.tile_post_base[tile];
  const int64_t rA = tile * a.cb, rB = min(a.row1, rA + (int64_t)a.cb);
  const int64_t eA = a.ent_base ? a.ent_base[blockIdx.x] : a.rowptr[rA], eB = a.ent_base ? a.ent_base[blockIdx.x + 1] : a.rowptr[rB];
  // every entry's row and value are loaded with its term, matching or not: three times the read traffic of this pass
  // (it comes from the caches) instead of a second dependent memory round trip for the quarter that matches
  for (int64_t k = eA + tid; k < eB; k += 4096) {
    int32_t t[4];
    uint32_t er[4];
    float vv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t e = k + 1024 * j;
      const bool in = e < eB;
      t[j] = in ? a.idx[e] : -1;
      er[j] = in ? a.erow[e] : 0u;
      vv[j] = in ? a.val[e] : 0.f;
    }
    uint32_t pos[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if ((uint32_t)(t[j] - lo) < span) pos[j] = atomicAdd(&cur[t[j] - lo], 1u);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if ((uint32_t)(t[j] - lo) < span) {
        const uint32_t local = er[j] - (uint32_t)rA;
        if (a.coarse) {
          const float sc = a.row_scale ? a.row_scale[er[j]] : 1.0f;
          const float wv_ = sc > 0.f ? vv[j] / sc : vv[j];
          a.post_c[pbase + pos[j]] = a.coarse_wide ? pack_coarse_wide(local, wv_) : pack_coarse(local << a.coarse_shift, wv_);
        } else {
          Posting p;
          p.slot = local;
          p.w = vv[j];
          a.post[pbase + pos[j]] = p;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// RUN-READING LDS build.  The streaming kernels above read a tile's entries once per term range (C3: 7 ranges -- idx, erow
// and val of 1e8 entries seven times over, 11 GB to place 0.4 GB of postings).  But the rows of the store are sorted by term
// (k_ingest_count rejects a batch whose indices are not strictly increasing, k_ingest_write and the tail view compact in
// order), so the entries of row r that belong to range g are ONE contiguous run of the row.  k_row_cuts reads idx once and
// leaves, per row, where each range's run starts; a (tile, range) workgroup of k_tile_runs then reads exactly its runs: the
// row of an entry comes from the loop (erow is not read), row_scale[row] is read once per row, and a workgroup's time is
// proportional to its own entries -- which makes narrower ranges (more workgroups for the 512 slots) affordable, and lets a
// term shard's workgroups outside [term_lo, term_hi) leave at once.  Counters / cursors, tile_seg, tile_post_base, segment
// alignment and padding are those of the streaming kernels; order inside a segment stays arbitrary.
//
// run_cut[(row - row0) * (n_ranges + 1) + g] = offset, from the first entry of the row's TILE, of the row's first entry whose
// term is >= g * range_terms (g = n_ranges: the row's end, or its first term outside [0, dim)).  32 bits: the host takes this
// build only while (longest row) x (rows per tile) < 2^32.  One 16-lane group per row.
constexpr int kRunRows = 4;       // rows in flight per lane group

__global__ void k_row_cuts(BuildArgs a, int32_t n_ranges, uint32_t *cut) {
  const int64_t row = a.row0 + ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / kGroup;
  const int gl = threadIdx.x % kGroup;
  if (row >= a.row1) return;
  const int64_t tb = a.rowptr[row / a.cb * a.cb], b = a.rowptr[row], e = a.rowptr[row + 1];
  uint32_t *c = cut + (row - a.row0) * (n_ranges + 1);
  const uint32_t rt = (uint32_t)a.range_terms;
  auto range_of = [&](int32_t t) { return (uint32_t)t < (uint32_t)a.dim ? (int32_t)((uint32_t)t / rt) : n_ranges; };  // (a term outside [0, dim) ends the last run)
  // entry k opens every range after its predecessor's up to its own (ranges without an entry: empty runs that start here)
  for (int64_t k = b + gl; k < e; k += kGroup) {
    const int32_t g = range_of(a.idx[k]);
    const int32_t gp = k > b ? range_of(a.idx[k - 1]) : -1;
    for (int32_t j = gp + 1; j <= g; ++j) c[j] = (uint32_t)(k - tb);
  }
  if (gl == 0) {
    const int32_t gp = e > b ? range_of(a.idx[e - 1]) : -1;
    for (int32_t j = gp + 1; j <= n_ranges; ++j) c[j] = (uint32_t)(e - tb);
  }
}

// MODE kRunHist: the histogram (tile_seg[.].y = segment lengths; with sub_cnt also the entries per sub-range); kRunScatter: the
// scatter (cursors start at tile_seg[.].x); kRunPartition: the first pass of the two-pass scatter (cursors per sub-range).
// L lanes per row (the host picks it from the mean run length), kRunRows rows in flight per lane group: the chain
// cut -> idx / val -> LDS atomic -> scattered store of one row overlaps that of the next three.  Runs longer than L are
// finished kRunRows chunks at a time.  The one-pass scatter costs what its 4-B stores cost (C3: 2.4 ms, 3.1 GB of 32-B
// partial writes for 0.45 GB of postings, whatever L, kRunRows or the range width); coarse renderings take the partition
// pass + k_tile_place_sub instead (0.9 + 0.3 ms).
constexpr int kRunHist = 0, kRunScatter = 1, kRunPartition = 2;
template <int MODE, int L>
__global__ __launch_bounds__(1024) void k_tile_runs(BuildArgs a, int64_t tile0, int32_t n_ranges) {
  extern __shared__ uint32_t run_lds[];  // [range_terms] counters / cursors
  constexpr bool SCATTER = MODE == kRunScatter, PART = MODE == kRunPartition, VALS = MODE != kRunHist;
  constexpr int U = kRunRows, GR = 1024 / L;
  const int tid = threadIdx.x;
  const int64_t tile = tile0 + blockIdx.x / n_ranges;
  const int32_t g = (int32_t)(blockIdx.x % n_ranges);
  const int32_t lo = g * a.range_terms;
  const uint32_t span = (uint32_t)(min(a.dim, lo + a.range_terms) - lo);
  uint2 *sg = a.tile_seg + tile * a.seg_stride + lo;
  if (lo >= a.term_hi || lo + (int32_t)span <= a.term_lo) {  // not a term of this handle in the range: every run is empty
    if (MODE == kRunHist) {
      for (uint32_t i = tid; i < span; i += 1024) sg[i] = make_uint2(0u, 0u);
      if (a.sub_cnt)
        for (uint32_t i = tid; i <= (span - 1) >> a.sub_shift; i += 1024) a.sub_cnt[(tile - tile0) * a.n_sub + (lo >> a.sub_shift) + i] = 0ull;
    }
    return;
  }
  // (partition: bucket starts relative to the workgroup's first bucket -- a tile's entries fit 32 bits)
  const int64_t sub0 = PART ? (tile - tile0) * a.n_sub + (lo >> a.sub_shift) : 0;
  const int64_t part_base = PART ? a.sub_base[sub0] : 0;
  if (PART) {
    for (uint32_t i = tid; i <= (span - 1) >> a.sub_shift; i += 1024) run_lds[i] = (uint32_t)(a.sub_base[sub0 + i] - part_base);
  } else {
    for (uint32_t i = tid; i < span; i += 1024) run_lds[i] = SCATTER ? sg[i].x : 0u;
  }
  __syncthreads();
  const int64_t rA = tile * a.cb, rB = min(a.row1, rA + (int64_t)a.cb);
  const int64_t eA = a.rowptr[rA];
  const uint32_t tile_e = (uint32_t)(a.rowptr[rB] - eA);  // no cut points beyond the tile's entries, whatever the table holds
  const int32_t *idx = a.idx + eA;
  const float *val = a.val + eA;
  const int32_t cw = n_ranges + 1;
  const uint32_t *cut = a.run_cut + (rA - a.row0) * cw + g;
  const int32_t nrows = (int32_t)(rB - rA);
  const int64_t pbase = SCATTER ? a.tile_post_base[tile] : 0;
  const bool scaled = VALS && a.coarse && a.row_scale;
  const int gi = tid / L, gl = tid % L;

  // U entries at once: every LDS atomic is issued before the first store waits for its position
  auto emit = [&](const int32_t (&t)[U], const float (&v)[U], const uint32_t (&local)[U], const float (&sc)[U]) {
    uint32_t pos[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if ((uint32_t)(t[u] - lo) < span) pos[u] = atomicAdd(&run_lds[PART ? (t[u] - lo) >> a.sub_shift : t[u] - lo], 1u);
    if (MODE == kRunHist) return;
    if (PART) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if ((uint32_t)(t[u] - lo) < span) {
          const float wv_ = sc[u] > 0.f ? v[u] / sc[u] : v[u];
          a.o_ent[part_base + pos[u]] =
              make_uint2((uint32_t)t[u], a.coarse_wide ? pack_coarse_wide(local[u], wv_) : pack_coarse(local[u] << a.coarse_shift, wv_));
        }
      }
      return;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if ((uint32_t)(t[u] - lo) < span) {
        if (a.coarse) {
          const float wv_ = sc[u] > 0.f ? v[u] / sc[u] : v[u];
          a.post_c[pbase + pos[u]] = a.coarse_wide ? pack_coarse_wide(local[u], wv_) : pack_coarse(local[u] << a.coarse_shift, wv_);
        } else {
          Posting p;
          p.slot = local[u];
          p.w = v[u];
          a.post[pbase + pos[u]] = p;
        }
      }
    }
  };
  auto load_cuts = [&](int32_t r0, uint32_t (&clo)[U], uint32_t (&chi)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int32_t r = r0 + u * GR;
      const bool in = r < nrows;
      clo[u] = in ? min(cut[(int64_t)r * cw], tile_e) : 0u;
      chi[u] = in ? min(cut[(int64_t)r * cw + 1], tile_e) : 0u;
    }
  };

  // the first chunk (L entries) of every run of an iteration's rows; the scale of a row travels with its entries
  auto load_heads = [&](int32_t r0, const uint32_t (&clo)[U], const uint32_t (&chi)[U], int32_t (&t)[U], float (&v)[U], float (&sc)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t k = clo[u] + gl;
      const bool in = k < chi[u];
      t[u] = in ? idx[k] : -1;
      v[u] = VALS && in ? val[k] : 0.f;
      sc[u] = scaled && in ? a.row_scale[rA + r0 + u * GR] : 1.0f;
    }
  };
  // Software pipeline, two iterations deep: the entries of the NEXT iteration's rows and the cuts of the one after are
  // requested before this iteration's atomics and stores.  Memory instructions retire in order (vmcnt): a load issued
  // behind a scattered store would be waited for only once that store has reached memory, a load issued ahead of it is not.
  uint32_t nlo[U], nhi[U], clo[U], chi[U];
  int32_t nt[U];
  float nv[U], nsc[U];
  load_cuts(gi, clo, chi);
  load_cuts(gi + GR * U, nlo, nhi);
  load_heads(gi, clo, chi, nt, nv, nsc);
  for (int32_t r0 = gi; r0 < nrows; r0 += GR * U) {
    uint32_t lo_c[U], hi_c[U], local[U];
    int32_t t[U];
    float v[U], sc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      lo_c[u] = clo[u];
      hi_c[u] = chi[u];
      t[u] = nt[u];
      v[u] = nv[u];
      sc[u] = nsc[u];
      local[u] = (uint32_t)(r0 + u * GR);
      clo[u] = nlo[u];
      chi[u] = nhi[u];
    }
    load_heads(r0 + GR * U, clo, chi, nt, nv, nsc);
    load_cuts(r0 + 2 * GR * U, nlo, nhi);
    emit(t, v, local, sc);
    // what is left of runs longer than L
#pragma unroll
    for (int u = 0; u < U; ++u) {
      uint32_t loc1[U];
      float sc1[U];
#pragma unroll
      for (int j = 0; j < U; ++j) {
        loc1[j] = local[u];
        sc1[j] = sc[u];
      }
      for (uint32_t k0 = lo_c[u] + L + gl; k0 < hi_c[u]; k0 += L * U) {
#pragma unroll
        for (int j = 0; j < U; ++j) {
          const uint32_t k = k0 + j * L;
          const bool in = k < hi_c[u];
          t[j] = in ? idx[k] : -1;
          v[j] = VALS && in ? val[k] : 0.f;
        }
        emit(t, v, loc1, sc1);
      }
    }
  }
  if (MODE != kRunHist) return;
  __syncthreads();
  for (uint32_t i = tid; i < span; i += 1024) sg[i] = make_uint2(0u, run_lds[i]);
  if (a.sub_cnt) {  // entries per sub-range: one wave per sub-range at a time (sub-ranges are multiples of 64 terms)
    const uint32_t n_sub_wg = ((span - 1) >> a.sub_shift) + 1;
    for (uint32_t sb = tid / kWave; sb < n_sub_wg; sb += 1024 / kWave) {
      uint32_t sum = 0;
      for (uint32_t i = (sb << a.sub_shift) + tid % kWave; i < min(span, (sb + 1) << a.sub_shift); i += kWave) sum += run_lds[i];
      for (int o = kWave / 2; o; o >>= 1) sum += (uint32_t)__shfl_xor((int)sum, o);
      if (tid % kWave == 0) a.sub_cnt[(tile - tile0) * a.n_sub + (lo >> a.sub_shift) + sb] = (unsigned long long)sum;
    }
  }
}

// Second pass of the two-pass scatter: workgroup (tile, sub-range) reads its bucket of {term, posting word} in one stream and
// places the words through LDS cursors.  Its corner of the posting array (C3: 256 terms x ~56 slots x 4 B = 57 KB) stays in
// the L2 while it is written, so memory sees whole lines: the one-pass scatter's 4-B stores land all over a 3.6-MB region
// per workgroup and reach memory as 32-B partial writes, 3.1 GB for 0.45 GB of postings (profiles/build_runs.md).
constexpr int kPlaceBlock = 512;
constexpr int kPlaceStage = 15360;  // words of the posting array a workgroup assembles in LDS (with the cursors: 64 KB, two workgroups per CU)
__global__ __launch_bounds__(kPlaceBlock) void k_tile_place_sub(BuildArgs a, int64_t tile0) {
  __shared__ uint32_t cur[kPlaceMaxTerms];
  __shared__ uint32_t stage[kPlaceStage];
  const int tid = threadIdx.x;
  const int64_t tile = tile0 + blockIdx.x / a.n_sub;
  const int32_t lo = (int32_t)(blockIdx.x % a.n_sub) << a.sub_shift;
  const uint32_t span = (uint32_t)(min(a.dim, lo + (1 << a.sub_shift)) - lo);
  const int64_t eA = a.sub_base[blockIdx.x], eB = a.sub_base[blockIdx.x + 1];
  if (eA >= eB) return;
  const uint2 *sg = a.tile_seg + tile * a.seg_stride + lo;
  // the sub-range's corner of the posting array: [first segment's start, the start of the segment behind the last one)
  const int64_t pbase = a.tile_post_base[tile];
  const uint32_t w0 = sg[0].x;
  const uint32_t w1 = lo + (int32_t)span < a.dim ? sg[span].x : (uint32_t)(a.tile_post_base[tile + 1] - pbase);
  // assembled in LDS (padding between the segments included: zero words) and written out in whole lines; a corner too large
  // for that (skewed terms) is written posting by posting
  const bool staged = w1 >= w0 && w1 - w0 <= (uint32_t)kPlaceStage;
  const uint32_t rel = staged ? w0 : 0u;
  for (uint32_t i = tid; i < span; i += kPlaceBlock) cur[i] = sg[i].x - rel;
  if (staged)
    for (uint32_t i = tid; i < w1 - w0; i += kPlaceBlock) stage[i] = 0u;
  __syncthreads();
  uint32_t *out = a.post_c + pbase;
  for (int64_t k = eA + tid; k < eB; k += 4 * kPlaceBlock) {
    uint2 e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = k + kPlaceBlock * j < eB ? a.o_ent[k + kPlaceBlock * j] : make_uint2(0xffffffffu, 0u);
    uint32_t pos[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (e[j].x - (uint32_t)lo < span) pos[j] = atomicAdd(&cur[e[j].x - (uint32_t)lo], 1u);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (e[j].x - (uint32_t)lo < span) {
        if (!staged) out[pos[j]] = e[j].y;
        else if (pos[j] < w1 - w0) stage[pos[j]] = e[j].y;
      }
    }
  }
  if (!staged) return;
  __syncthreads();
  for (uint32_t i = tid; i < w1 - w0; i += kPlaceBlock) out[w0 + i] = stage[i];
}

// ---------------------------------------------------------------------------------------------------------
// BUCKETED entries for the LDS build of LARGE dims (more than kBuildMaxRanges ranges of kBuildRange terms: vectorDim = 2^20,
// the reference's HashingTF default).  The LDS build re-reads a tile's entries once per term range -- 64 times at dim = 2^20
// -- which is why such dims kept the global-atomic kernels (two atomics per posting: 39 of the 161 ms of a C5-shaped step,
// 0.59 of configs[4]'s 13.9 s).  Here a tile's entries are first PARTITIONED by term range, a counting sort in two passes
// over (tile, slice) workgroups: count per range in LDS, one global atomic per (workgroup, range) to reserve a run of the
// range's bucket, scatter through LDS cursors.  The LDS build's workgroup (tile, range) then reads ITS bucket only
// (BuildArgs::ent_base).  Order inside a bucket -- hence inside a posting segment -- is whatever the atomics give, as it
// is with the atomic build.
struct BucketArgs {
  const int64_t *rowptr;
  const int32_t *idx;
  const float *val;
  const uint32_t *erow;
  int64_t row1;          // rows of the build end here
  int32_t cb, n_ranges, range_terms;
  int64_t tile0;
  unsigned long long *bucket_cnt;       // [tiles x n_ranges] entries per (tile, range)        (pass 1 out)
  const int64_t *bucket_base;           // [tiles x n_ranges + 1] their exclusive scan          (pass 2 in)
  unsigned long long *bucket_cur;       // [tiles x n_ranges] entries placed so far             (pass 2)
  int32_t *o_idx;
  uint32_t *o_erow;
  float *o_val;
};

template <bool SCATTER>
__global__ __launch_bounds__(1024) void k_bucket_pass(BucketArgs a) {
  __shared__ uint32_t cnt[kBucketMaxRanges];
  __shared__ int64_t base[kBucketMaxRanges];
  const int tid = threadIdx.x;
  const int64_t tl = blockIdx.x / kBucketSlices;  // tile of the build (0-based)
  const int sl = blockIdx.x % kBucketSlices;
  const int64_t rA = (a.tile0 + tl) * a.cb, rB = min(a.row1, rA + (int64_t)a.cb);
  const int64_t eA = a.rowptr[rA], eB = a.rowptr[rB];
  const int64_t per = (eB - eA + kBucketSlices - 1) / kBucketSlices;
  const int64_t k0 = eA + sl * per, k1 = min(eB, k0 + per);
  for (int i = tid; i < a.n_ranges; i += 1024) cnt[i] = 0u;
  __syncthreads();
  for (int64_t k = k0 + tid; k < k1; k += 1024) atomicAdd(&cnt[(uint32_t)a.idx[k] / (uint32_t)a.range_terms], 1u);
  __syncthreads();
  unsigned long long *const dst = (SCATTER ? a.bucket_cur : a.bucket_cnt) + tl * a.n_ranges;
  for (int i = tid; i < a.n_ranges; i += 1024) {
    const uint32_t c = cnt[i];
    if (c) {
      const unsigned long long at = atomicAdd(&dst[i], (unsigned long long)c);  // (pass 2: the start of this workgroup's run)
      if (SCATTER) base[i] = a.bucket_base[tl * a.n_ranges + i] + (int64_t)at;
    }
    if (SCATTER) cnt[i] = 0u;  // becomes the run's cursor
  }
  if (!SCATTER) return;
  __syncthreads();
  for (int64_t k = k0 + tid; k < k1; k += 1024) {
    const int32_t t = a.idx[k];
    const uint32_t r = (uint32_t)t / (uint32_t)a.range_terms;
    const int64_t p = base[r] + atomicAdd(&cnt[r], 1u);
    a.o_idx[p] = t;
    a.o_erow[p] = a.erow[k];
    a.o_val[p] = a.val[k];
  }
}

// per-tile minimum of the positive shard sub-norms (threshold scale of a tile in shard mode)
__global__ void k_tile_min_sub(const float *sub, int64_t n_rows, int32_t cb, float *tile_min, int64_t tile0) {
  const int64_t tile = tile0 + blockIdx.x;
  const int64_t r0 = tile * cb, r1 = r0 + cb < n_rows ? r0 + cb : n_rows;
  float m = 3.0e38f;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += blockDim.x) {
    const float v = sub[r];
    if (v > 0.f) m = fminf(m, v);
  }
  __shared__ float red[1024];
  red[threadIdx.x] = m;
  __syncthreads();
  for (int o = blockDim.x / 2; o; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] = fminf(red[threadIdx.x], red[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) tile_min[tile] = red[0] > 1.0e38f ? 0.f : red[0];
}

}  // namespace apss
