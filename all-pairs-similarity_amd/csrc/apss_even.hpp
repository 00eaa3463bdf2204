// k_probe_even: the FILTER pass of the two-pass join (k_probe_coarse's arithmetic and accumulators) restructured for
// THIN rounds -- a term shard (BASELINE.json configs[3]: a dozen terms per query and shard) or a sparse regime -- where a
// round carries a few hundred postings and its duration is a chain of serially issued instructions and latencies, not a
// throughput.  DESIGN.md 5a has the measurements behind every choice below.
//
// What k_probe_coarse pays per round whatever the round holds: every wave stages its own share of the query's terms
// (term k -> wave k % NW: descriptor loads, a wave-wide scan, strip writes for two live lanes), then adds, then -- after
// the first barrier -- an LDS read of the round's counters (survivors, overflow flag, long list), the report loop, the
// clears and the second barrier.  The T = 8 shard kernel measured 3,340 cycles per round (VALU and LDS half idle).
//
// Here:
//  * FIXED ROLES.  Waves 0 .. F-1 STAGE every round and never add; waves F .. NW-1 ADD every round and never stage;
//    each kind runs its own loop with the same two barriers per round.  F = ceil(longest query / (64 / G)), G = 1, 2 or 4
//    staging lanes per term.  A staging wave scans the round's chunk counts once, two rounds ahead, and deals the chunks
//    out over the A = NW - F adding waves in WHOLE WINDOW STEPS: chunk j -> step j / 8A, and inside the step adding wave
//    (j % 8A) / 8, lane group j % 8.  A round of `tot` chunks costs ceil(tot / 8) wave-steps, not A ceil(tot / 8A): the waves
//    behind the last chunk are one step short and skip it.
//  * NOTHING IS READ AFTER THE FIRST BARRIER.  Everything a round needs to know about itself is a fact of its staging
//    (chunks per wave, long segments, whether the window overflows -> whole-tile clear): an adding wave reads it one round
//    ahead, in the same LDS round trip as its next strip and the current adds.  A crossing is reported by the wave that
//    sees it (ballot-compacted append to the global list), not through an LDS list that every wave re-reads.
//    So an adding wave's round is: strip read + adds (one LDS round trip) -> next loads, tests -> barrier -> clears -> barrier.
//  * NO TRIPS THROUGH THE SCALAR UNIT ON THE HOT PATH.  Idle lanes add to spare LDS words / write spare strip entries
//    (selects on the address, no exec masks); first touches and crossings are counted per lane; one branch per round takes
//    everything unusual.  Loaded values are used a round after their load, by the next stage.  (The one deliberate
//    exception: the round's two fact words go to the scalar unit as loaded, two v_readfirstlane per round, and this wave's
//    chunks and steps are worked out there -- used a round later, so nothing waits for the hand-over; it took 18 vector
//    instructions off the round for 25 scalar ones, see strip_loads.)
//  * FEW VECTOR INSTRUCTIONS PER POSTING SLOT (LEAN: every instantiation with non-negative weights; the kernel is bound by the
//    vector instructions it issues).  A batch's crossings are found by the MAXIMUM of old + product over its postings, one
//    compare per batch; an idle lane's spare word is kept small and non-zero (set to 1 in every round's clear phase), so its
//    returned value needs no replacing -- it is never a first touch and its sum is far below any real threshold; first touches
//    are counted through their complement, min(old, 1) summed per lane, against the slots tested per round; and an adding
//    wave INVALIDATES the window entries of a strip it has just read (offset kStale), so that an entry the staging waves do
//    not rewrite two rounds later sends its load out of range by itself -- no slot-against-count test per window step.
//
// Pipeline (round v of a workgroup = one query against the tile's accumulators):
//   round v - 5 : staging waves load the row's extent                  (load_R)
//   round v - 4 :               load the query's terms                 (load_I)
//   round v - 3 :               load the (tile, term) descriptors      (load_P)
//   round v - 2 :               scan + write chunk descriptors into strips[v % 3], long segments into longs[v % 3]
//   round v - 1 : every adding wave reads its strip and the round's facts, starts its posting loads
//   round v     : adds + crossing tests (register window; chunks past the window straight from the strip), clear
// The two workgroup barriers of round v - 2 separate the strip writes from their readers; the ring of three keeps the
// strip of round v readable during round v while round v + 2 is being staged.
//
// TWO PLANES, ONE BARRIER PER ROUND (TWO: k_probe_planes, the plain 512-thread handle over <= 32768-row tiles whose sums fit a
// byte -- acc8_scale() in apss_filter_plan.hpp).  The second barrier of a round exists only because the clears write the plane the
// next round adds into.  With two planes of 8-bit sums in the same 64 KB, round v adds into plane v mod 2, and round v - 1 is
// cleared on the OTHER plane at the top of round v, directly ahead of round v's adds, from the posting registers that still
// hold it (the wfa / wfb set that round v's loads for v + 1 have not yet overwritten): one barrier and one drain of the LDS
// queue per round instead of two.  The barrier of round v separates adds(v) from clears(v), which run in round v + 1; the
// barrier of round v + 1 separates clears(v) from adds(v + 2), the next adds on that plane.  A `rare` round's whole-plane clear
// moves the same way and touches its own plane only.  Behind an item's last barrier comes the last round's clear, then the
// barrier every item ends with: the next item of a persistent workgroup finds both planes zero (`first` clears both).
// The kernel reads the index as k_probe_even<512, .., false, false, false> does (slot << 1 in a posting's low half), and a
// handle goes back to that kernel without a rebuild (drop_planes).  The planes are INTERLEAVED BY BYTE: slot s of plane p is
// byte 2 s + p, i.e. the two bytes of the 16-bit kernel's accumulator are the slot's two planes.  The add's word address is then
// the 16-bit kernel's (pcw & 0xfffc: the same banks), its shift 16 (s % 2) + 8 p is (pcw << 3) + 8 p (one v_lshl_add_u32 in
// place of the shift), and a clear is a byte store at (pcw & 0xffff) + p with p in the instruction's immediate offset: no
// vector instruction more than the 16-bit kernel issues.  (First built with plane p in the bytes [32768 p, 32768 p + cb): the
// word address (pcw >> 1) & 0x7ffc costs one instruction per posting more, and that took back all the barrier gave --
// profiles/even_planes.md.)  The price is the `rare` round's whole-plane clear: the other plane's bytes of the same words are
// live, so it is an atomic AND over the tile's words instead of 16-byte stores.
// WIPE (k_probe_planes<5>, <6>: windows of five steps or more).  The per-posting clears were two fifths of the kernel's LDS
// instructions, and round v - 1's plane is idle for the whole of round v: any wave can zero it with any instruction.  These
// instantiations keep the planes SEPARATE -- plane p is the bytes [32768 p, 32768 p + cb) of acc, byte `slot` of it the slot's
// sum; the spare words stay behind byte 65,536 -- and zero the idle plane WHOLE, ceil(cb / 256) stores of 256 zero bytes by
// ds_write_addtid_b32 (address = M0 + immediate + 4 lane: no address register, no bank conflict, two LDS cycles a store),
// dealt over all eight waves, the staging waves included, as the first LDS work of the round in either role (see wipe()).
// The index is still the 16-bit rendering and the handle still goes back to k_probe_even without a rebuild: the add's word
// address is (pcw >> 1) & 0x7ffc, its shift the low five bits of pcw << 2, the plane in the instruction's immediate offset.
// That is one vector instruction per posting more than the interleaved planes' add -- which by itself took back what the
// barrier gave -- and the one their clear spent on its byte address, which goes with the clear.
// clear_round keeps the spare words' reset only; a `rare` round needs no clear of its own (no atomic AND: the wipe takes its
// plane like any other); the clear behind an item's last barrier is a wipe of the last round's plane by all eight waves;
// `first` still zeroes both planes.
// The barrier argument, for the wipe: round v adds into plane v mod 2 and wipes the other.  wipe(v - 1), in round v, lies
// behind the barrier of round v - 1, which every adding wave passes with its adds of that round landed and tested, and
// ahead of the barrier of round v (each wave drains its own stores first: the compiler does not count them), behind which
// come the adds of round v + 1, the next on that plane.  Between those two barriers the only adds are round v's, on the other
// plane, 32,768 bytes away: a wipe and an add never share a word, and the stores' round-up past cb ends inside their plane.
// Narrower windows keep the interleaved planes and the per-posting clears: the wipe costs 2 ceil(cb / 256) LDS cycles per
// round whatever the round holds, the clears 7.4 x 2 U A, and no workload measured here takes a planes kernel of fewer than
// five steps, so nothing there could be confirmed.
// THE RING OF THREE under one barrier.  Between the barriers of rounds v - 1 and v every wave is in round v, and there the
// adding waves read ring slot v + 1 (their next strip and its facts; they invalidate the window entries they read) and,
// on `rare` paths, ring slot v (chunks past the window, long segments); the staging waves write ring slot v + 2 (strips,
// longs, the facts' counters) and zero facts[v], which was last read in round v - 1 and is counted into again in round
// v + 1 -- a barrier away on either side.  v, v + 1, v + 2 are distinct modulo 3, so no slot is read and written between the
// same two barriers, and what is staged in round v is read from round v + 1 on.  One exception: the adding waves' FIRST strip
// read (ring slot 0, in the prologue) already shares its interval with the staging waves' round v0, which zeroes facts[0] --
// so the facts of an item's first round are counted in facts[3], a slot no later round uses (zeroed at the item's start).
//
// A round whose chunks exceed the strips (A x SLOTS) or whose long segments exceed LONGCAP is flagged at staging and
// swept by the adding waves straight from the index (one term per wave at a time): slow, unbounded, never wrong.
// Queries of more than 64 x NW / 4 terms are not served (they stay with k_probe_coarse; apss_hip.hip chooses).
#pragma once
#include <type_traits>
#include "apss_kernels.hpp"

namespace apss {

// the launch's arguments where the kernel finds them: the kernarg segment (scalar loads), see probe_even_body
using ProbeArgsK = const __attribute__((address_space(4))) ProbeArgs;

template <int BLOCK, int U, int LONGCAP, bool SHARD, bool SIGNED, bool ACC8, bool MERGE, bool TWO = false>
__device__ __forceinline__ void probe_even_item(ProbeArgsK &a, const int tile, const int v0, const int v1, const bool own_tile, const bool first) {
  // one ITEM of the launch: the rounds [v0, v1) against candidate tile `tile` (`first`: this workgroup's first item)
  // (Tried for C3's full rounds: workgroups of TEN waves -- the eight adding waves of the 512-thread kernel plus two staging
  // waves, 87 VGPRs at five steps.  143 vs 111 ms: ten waves spread 3/3/2/2 over the SIMDs and the second workgroup of a CU
  // needs a SIMD to hold six of them, i.e. <= 80 VGPRs; it did not become resident.)
  constexpr int NW = BLOCK / kWave;
  static_assert(NW == 8 || NW == 16, "8 or 16 waves");
  constexpr int NS = NW - 1;  // strips per ring slot: one per adding wave (at least one wave stages)
  constexpr bool SLOT2 = BLOCK <= 512;
  constexpr uint32_t ABITS = ACC8 ? 8u : 16u;
  constexpr bool WIDE = ACC8 && BLOCK > 512;
  constexpr int CH = 16, LPC = CH / 2, GPW = kWave / LPC, WIN = GPW * U;
  constexpr int SLOTS = 2 * WIN < 48 ? 2 * WIN : (WIN > 48 ? WIN : 48);  // strip slots per wave and round (>= WIN)
  static_assert(SLOTS >= WIN, "the register window reads the first WIN slots of a strip");
  // A strip is stored GROUP-major: slot sl = u * GPW + g (window step u, lane group g) lives at entry g * GS + u, so that the
  // entries a lane group needs for two consecutive steps are adjacent and one ds_read_b128 fetches both (the adding waves'
  // strip reads were 23 % of the LDS instructions of a C3 round; GS even: 16-B alignment of every pair)
  // (the 1024-thread kernel's LDS is full to within a few hundred bytes: no padding there, pairs only where GS is even anyway)
  constexpr int GS = BLOCK > 512 ? SLOTS / GPW : ((SLOTS / GPW) + 1) & ~1;  // entries per lane group
  constexpr int SSZ = GPW * GS;                 // entries per strip
  static_assert(GPW == 8 && SLOTS % GPW == 0, "slot <-> (step, group) by shifts");
  constexpr int kLongLen = kLongLenW;
  constexpr int CBMAX = WIDE ? 131072 : (BLOCK <= 512 && !ACC8 ? 32768 : 65536);
  constexpr int APW = 32 / (int)ABITS;
  constexpr bool LEAN = !SIGNED;  // (signed sums are not monotone: a maximum of old + product says nothing about a crossing)
  // an idle lane adds 1 to the low accumulator of its spare word, which the NW - 1 adding waves' lanes of that number share:
  // set to 1 every round, it stays non-zero inside its ABITS bits
  static_assert(1 + (NW - 1) * 2 * U < (1 << (ACC8 ? 8 : 16)), "the spare words' low accumulators must not wrap within a round");
  // TWO PLANES (k_probe_planes, see the header): 8-bit sums over <= 32768-row tiles, read from the 16-bit rendering of the index
  // (slot << 1 in the low half of a posting); the planes are interleaved by BYTE: slot s of plane p is byte 2 s + p of acc
  // (U < 5; WIPE below)
  static_assert(!TWO || (BLOCK == 512 && ACC8 && !MERGE && !SIGNED && !SHARD), "two planes: the plain 512-thread kernel, 8-bit sums");
  // WIPE (windows of five steps or more, see the header): the planes are SEPARATE -- plane p is the bytes [32768 p, 32768 p + cb)
  // of acc -- and the idle one is zeroed whole, by all eight waves, instead of posting by posting
  constexpr bool WIPE = TWO && U >= 5;
  constexpr uint32_t kPlane = 32768u;  // WIPE: bytes from one plane to the other
  __shared__ __attribute__((aligned(16))) uint32_t acc[CBMAX / APW + kWave];  // (+ one spare word per lane: idle lanes add there)
  __shared__ __attribute__((aligned(16))) uint2 strips[3 * NS * SSZ + kWave];  // [3][NS][GPW][GS] {byte offset of the chunk's first posting, weight bits} (+ one spare entry per lane)
  __shared__ uint2 longs[3 * LONGCAP];
  __shared__ float long_w[3 * LONGCAP];
  __shared__ uint2 facts[4];  // per ring slot: {chunks of the round, bit 0: flagged for the direct sweep, bits 1..: long segments}
  __shared__ unsigned long long stat[4];
  unsigned char *const smem_raw = reinterpret_cast<unsigned char *>(acc);
  uint32_t *const facts_w = reinterpret_cast<uint32_t *>(facts);

  // (the thread index, opaque per item: what a lane derives from it -- the addresses of either role -- is otherwise hoisted
  // out of the persistent loop and stays live through both roles' loops; flagship instantiation: 116 vs 113 VGPRs, 25 vs 11
  // scalar spills)
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int wv = __builtin_amdgcn_readfirstlane(tid / kWave), ln = tid % kWave;
  const int cb = a.cb;
  const int F = a.flat_waves;   // waves that stage a round
  const int A = NW - F;         // waves that add a round (those not staging in it)
  const int CAP = A * SLOTS;    // chunks per round
  const uint32_t A8 = (uint32_t)A * (uint32_t)GPW;  // chunks of one window step of the whole round: 8 per adding wave
  const float rcpA8 = 1.0f / (float)A8;
  const uint32_t magicA8 = 0xffffffffu / A8 + 1u;  // x / 8A = umulhi(x, magic) for x < 2^16: magic x 8A - 2^32 is in [0, 8A]
  // lanes per term in a staging wave (1, 2 or 4): a staging lane writes the chunks k = sub, sub + G, ... of its term, so a
  // term of <= 2 G chunks costs every lane two strip writes and no loop (a wave issues its instructions one after another
  // whatever the number of live lanes: the staging wave's instruction count is on the round's critical path)
  const int LOGG = a.flat_group_log2, G = 1 << LOGG;
  const uint32_t sub = (uint32_t)ln & (uint32_t)(G - 1);
  // MERGED rounds (ProbeArgs::merge_log2 = m > 0): round v stages the terms of the M = 2^m query rows M v .. M v + M - 1 as
  // ONE row -- they are neighbours in the CSR arrays, so the merged row is the extent rowptr[M v] .. rowptr[M v + M) -- and a
  // candidate's accumulator holds the SUM of its M filter sums: an upper bound of each of them (non-negative weights), so a
  // candidate that stays below the threshold fails for every query of the round, and a crossing is reported for the round
  // (k_expand_merged turns it into M survivors; the exact pass / the shard's phase 2 prunes as ever).  a.nq, a.q_chunk and v
  // count ROUNDS; a.nq_rows the rows; a.q_val holds the rows' weights already divided by their shard factors.
  // NOT where a query meets ITSELF: a stored row's product with its own slot crosses the threshold by itself, and the crossing
  // would stand for its M - 1 neighbours too (one false survivor per query and shard).  A workgroup whose candidate tile holds
  // rows of its own chunk (the diagonal of a whole-store join, the last tiles of an appended batch) runs its rows ONE per round
  // (`mlog` = 0 for this workgroup, on the launch's smaller scale) and marks what it reports with kUnmergedBit.
  // (MERGE: instantiations of their own -- the handful of scalars this costs took the unmerged shard kernel to its SGPR limit: 13.0 -> 13.9 ms at T = 8)
  static_assert(!MERGE || SHARD, "merged rounds: term shards only");
  // (own_tile is decided per CELL of the launch's (tile, chunk) grid -- probe_even_body below, apss_worklist.hpp -- and the rounds
  // [v0, v1) of this item count rows then, merged rounds otherwise)
  const int mlaunch = MERGE ? a.merge_log2 : 0;
  const int mlog = own_tile ? 0 : mlaunch;
  const int nv = own_tile ? a.nq_rows : a.nq;
  const int qtile = (v0 << mlog) / cb;  // (symmetric joins: the item lies inside one tile)
  const int64_t tile_row0 = (int64_t)tile * cb;
  const int unmerged_mark = own_tile ? kUnmergedBit : 0;
  const uint32_t lo = (uint32_t)(ln % LPC);
  const float cxs = a.cx_scale;

  // (scalar loads, said to be so: inside the persistent loop these reads lie behind the last item's stores, the compiler no longer
  // proves them unclobbered and loads them into VECTOR registers -- and a buffer descriptor made of vector registers costs a
  // waterfall loop around every load through it)
  const int64_t qbase = uniform_load(a.q_rowptr + (MERGE ? min(v0 << mlog, a.nq_rows) : v0)), qend = uniform_load(a.q_rowptr + (MERGE ? min(v1 << mlog, a.nq_rows) : v1));
  const int64_t pbase = uniform_load(a.tile_post_base + tile), pend = uniform_load(a.tile_post_base + tile + 1);
  const __amdgpu_buffer_rsrc_t rs_qi =
      __builtin_amdgcn_make_buffer_rsrc((void *)(a.q_idx + qbase), 0, (int)((qend - qbase) * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_qv =
      __builtin_amdgcn_make_buffer_rsrc((void *)(a.q_val + qbase), 0, (int)((qend - qbase) * 4), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_tp = __builtin_amdgcn_make_buffer_rsrc(
      (void *)(a.tile_seg + (int64_t)tile * a.seg_stride), 0, (int)(a.seg_stride * 8), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_po =
      __builtin_amdgcn_make_buffer_rsrc((void *)(a.post_c + pbase), 0, (int)((pend - pbase) * 4), 0x00020000);
  constexpr uint32_t kOob = 0xfffffff0u;
  // LEAN: the offset of an invalidated strip entry, and what a round flagged for the direct sweep adds to every offset of its
  // window (its strips hold what was staged before the flag went up).  A tile's postings are < 2^29 bytes (apss_hip.hip takes
  // the two-pass path below 2^27 postings per tile), so with the lane's part (< 64) on top: kStale + .. in [2^31, 2^31 + 64),
  // valid + kSwept + .. in [2^30, 2^30 + 2^29 + 64), kStale + kSwept + .. in [3 * 2^30, 3 * 2^30 + 64) -- all out of range.
  constexpr uint32_t kStale = 0x80000000u, kSwept = 0x40000000u;
  constexpr uint32_t kRare = 0x80000000u;  // WaveWork::info: the round needs more than the register window (see strip_loads)
  constexpr uint32_t kCountMask = 0xffffu;  // WaveWork::info bits 16..19: window steps that hold chunks of this wave
  // A wave skips the window steps behind its last chunk (adds, tests, clears).  A wave otherwise issues all U steps whether
  // or not their slots hold postings, and the LDS pipeline pays for each; the windows of shards and of the sparse regime are
  // sized for the upper end of a varying term count (C5's shape: 244.5 -> 218.5 ms), and chunks are dealt in whole steps (see
  // put()), so the waves behind a round's last chunk are a step short of the others in every round.
  // The 1024-thread kernel and the plain handles only ever skip their LAST step (with every step behind a branch C5's shape
  // measured 245 vs 219 ms, C3 101.1 vs 102.4 ms); shard-rule launches any.
  // (Tried: logical wave = (rank + round) mod A, so that the waves of a round's extra step are not always those of the same
  // SIMDs.  C3: 49.3 vs 49.1 ms with it -- profiles/even_steps.md; not kept.)
  constexpr int kFirstSkippable = BLOCK > 512 || !SHARD ? U - 1 : 0;

  // (a later item of a persistent workgroup: the accumulators are zero behind the last round's second barrier; the strip
  // entries are made stale, the facts zero and the spare words 1 again)
  if (first) {
    for (int i = tid * 4; i < cb / APW; i += BLOCK * 4) *reinterpret_cast<uint4 *>(acc + i) = make_uint4(0u, 0u, 0u, 0u);
    if constexpr (TWO)  // (two bytes per slot: the second cb bytes; WIPE: the second plane)
      for (int i = tid * 4; i < cb / APW; i += BLOCK * 4) *reinterpret_cast<uint4 *>(acc + (WIPE ? (int)kPlane / 4 : cb / APW) + i) = make_uint4(0u, 0u, 0u, 0u);
  }
  if (tid < kWave) acc[CBMAX / APW + tid] = 1u;  // the spare words (LEAN: never zero in their low accumulator)
  if (LEAN) {  // no strip entry is valid before it is staged
    for (int i = tid; i < 3 * NS * SSZ; i += BLOCK) strips[i].x = kStale;
  }
  if (tid < 8) facts_w[tid] = 0;
  unsigned long long my_visits = 0;
  uint32_t my_cands = 0;
  uint32_t n_seen = 0;  // LEAN: window slots that were NOT a first touch, minus the window slots tested (mod 2^32)

  // WIPE: zeros over plane PL (0 | 1) of acc, ceil(cb / 256) stores of 256 bytes dealt over the eight waves, staging waves
  // included (a store's data goes to the LDS over one of two paths, one per pair of SIMDs, and a workgroup's consecutive
  // waves alternate between them): store k = wv + 8 j by wave wv.  ds_write_addtid_b32 writes the dword at
  // M0[15:0] + offset + 4 lane -- no address register, no bank conflict, half the cycles of a ds_write_b32.  M0 is the
  // compiler's: saved and restored inside the statement.  It holds the LDS address of acc + 256 wv; the immediate holds the
  // plane and the stride from one store of the wave to its next, 32768 PL + 2048 j (63,488 at the most).  M0's sixteen bits
  // hold that address wherever the compiler puts acc: whatever lies in front of it is some of this kernel's other LDS, and
  // the assertion below keeps all of that, with the 1,792 of the last wave, under 2^16.  A wave's stores go out four to a
  // statement, so up to three of them, and the last store of a plane, may lie past cb: with j <= 15 they stay inside the
  // plane's 32,768 bytes.  The compiler does not count these stores: wipe_wait() stands between them and the barrier.
  static_assert(!WIPE || sizeof(strips) + sizeof(longs) + sizeof(long_w) + sizeof(facts) + sizeof(stat) + 256 /* the body's */ + 256 * (NW - 1) < 65536,
                "M0[15:0] must hold the LDS address of acc + 256 wv wherever acc lies");
  const int wipe_n = WIPE ? ((cb + 255) >> 8) - wv : 0;  // this wave's stores per plane: j with 8 j < wipe_n (16 of a full tile's 128)
  const uint32_t wipe_m0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)acc + 256u * (uint32_t)wv;
  auto wipe = [&](auto plane_c) {
    constexpr int PL = (int)decltype(plane_c)::value * (int)kPlane;
    uint32_t zero = 0u;
    asm volatile("" : "+v"(zero));
    uint32_t keep;
    // (opaque here: the four comparisons below are otherwise hoisted out of the rounds as four lane masks, eight scalar
    // registers held across the item by a kernel that spills scalars as it is)
    int n = wipe_n;
    asm volatile("" : "+s"(n));
    // (the stores j = 4 JB .. 4 JB + 3 of this wave, if the first of them lies inside cb; written out four times: an asm
    // operand does not capture, so no lambda of its own)
#define APSS_WIPE_FOUR(JB)                                                                                                        \
  if (32 * (JB) < n)                                                                                                              \
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"                                                            \
                 "ds_write_addtid_b32 %1 offset:%3\n\tds_write_addtid_b32 %1 offset:%4\n\t"                                      \
                 "ds_write_addtid_b32 %1 offset:%5\n\tds_write_addtid_b32 %1 offset:%6\n\t"                                      \
                 "s_mov_b32 m0, %0"                                                                                              \
                 : "=&s"(keep)                                                                                                   \
                 : "v"(zero), "s"(wipe_m0), "i"(PL + 8192 * (JB)), "i"(PL + 8192 * (JB) + 2048), "i"(PL + 8192 * (JB) + 4096),   \
                   "i"(PL + 8192 * (JB) + 6144)                                                                                  \
                 : "memory")
    APSS_WIPE_FOUR(0);
    APSS_WIPE_FOUR(1);
    APSS_WIPE_FOUR(2);
    APSS_WIPE_FOUR(3);
#undef APSS_WIPE_FOUR
  };
  constexpr std::integral_constant<int, 0> plane0{};
  constexpr std::integral_constant<int, 1> plane1{};
  auto wipe_wait = [&] { asm volatile("s_waitcnt lgkmcnt(0)" : : : "memory"); };

  struct RowExt { int qb; int nnz; };  // as loaded: the low halves of the row's rowptr entries
  struct TermW { uint32_t term; float w, qs; bool valid; };
  struct Seg { uint32_t s, len; float w; };
  struct WaveWork {
    uint32_t info;     // (scalar) chunks of the round dealt to this wave | kRare
    uint32_t flags;    // (per lane, uniform) the round's flags as staged: bit 0 direct sweep, bits 1.. long segments
    apss_u32x2 pc[U];  // two coarse postings per lane and step
    float wq[U];       // query weight x cx_scale of the step's chunk
  };
  // Every stage only ISSUES its loads; whatever is computed from a loaded value is computed by the NEXT stage, a round
  // later (an operation on a value just loaded is a wait for the memory round trip, on the path to the barrier).  The
  // per-row facts -- row extent, shard factor -- are loaded by the staging lanes themselves as vector loads, after the
  // round's first adds: a scalar prefetched by every wave cost SGPRs the kernel does not have (the spill forced a wait
  // for the scalar load at the top of every round), and a vector load at the top of the round would sit in the in-order
  // wait for the round's postings.
  const int32_t *const rowptr_lo = reinterpret_cast<const int32_t *>(a.q_rowptr);
  const int qbase_lo = (int)(uint32_t)qbase;
  auto load_R = [&](int v) {  // raw: the low halves of rowptr[v], rowptr[v + 1]
    RowExt r;
    const int row_a = min(v, nv - 1) << mlog, row_b = MERGE ? min(row_a + (1 << mlog), a.nq_rows) : row_a + 1;
    r.qb = rowptr_lo[2 * row_a];
    r.nnz = rowptr_lo[2 * row_b];
    return r;
  };
  auto load_I = [&](const RowExt &r, const int fi, const int v) {
    TermW t;
    const int kterm = ((fi * kWave) >> LOGG) + (ln >> LOGG);
    const int nnz = v < v1 ? r.nnz - r.qb : 0;
    t.valid = kterm < nnz;
    const uint32_t off = t.valid ? (uint32_t)(r.qb - qbase_lo + kterm) * 4u : kOob;  // (< 2^31: a workgroup's slice of the batch)
    t.term = __builtin_amdgcn_raw_buffer_load_b32(rs_qi, off, 0, 0);
    t.w = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs_qv, off, 0, 0));
    t.qs = SHARD && !MERGE ? a.q_scale[min(v, nv - 1)] : 1.0f;  // shard rule: |q_g| / |q|, the query's half of the normalisation
    return t;
  };
  auto load_P = [&](const TermW &t) {
    Seg g;
    const apss_u32x2 sg = __builtin_amdgcn_raw_buffer_load_b64(rs_tp, t.valid ? t.term * 8u : kOob, 0, 0);
    g.s = sg.x;
    g.len = sg.y;
    // (rcp: 1 ulp; the coarse threshold's two units of slack cover the 2^-6 units it can add up to over a whole row)
    g.w = SHARD ? (t.qs > 0.f ? t.w * __builtin_amdgcn_rcpf(t.qs) : 0.f) : t.w;
    return g;
  };
  // Staging of one round by one of its F waves: a scan of the terms' chunk counts, the group shares its term's first
  // index through a DPP move, and every lane writes at most two descriptors -- to the strip, or to its own spare entry when
  // it has none (a select on the address, not an exec mask).  Everything unusual -- a long segment, a term of more than
  // 2 G chunks, a round that does not fit -- takes one branch.
  uint2 *const spare_item = strips + 3 * NS * SSZ + ln;
  // (`fs`: the facts' slot of the round, its ring slot but for an item's first round with TWO: see ONE BARRIER PER ROUND)
  auto flatten = [&](const Seg &g, const int ring, const int fs) {
    uint32_t len = g.len;
    my_visits += sub == 0u ? len : 0u;
    const bool is_long = len > (uint32_t)kLongLen;
    len = is_long ? 0u : len;
    const uint32_t nch = (len + CH - 1) / CH;
    // the term's first chunk index: a scan over the staging lanes plus ONE LDS atomic per wave on the round's counter (F > 1:
    // the waves' ranges interleave in whatever order; a returning atomic per TERM on that one address measured 45 vs 32 ms)
    const uint32_t mine = sub == 0u ? nch : 0u;  // a term counts once, in the first lane of its group
    const uint32_t incl = wave_incl_scan(mine);
    uint32_t base = 0;
    if (ln == kWave - 1) base = atomicAdd(&facts_w[2 * fs], incl);
    uint32_t j0 = (uint32_t)__builtin_amdgcn_readlane((int)base, kWave - 1) + incl - mine;
    if (LOGG == 2) j0 = (uint32_t)__builtin_amdgcn_update_dpp((int)j0, (int)j0, 0x00, 0xf, 0xf, false);       // quad_perm [0,0,0,0]
    else if (LOGG == 1) j0 = (uint32_t)__builtin_amdgcn_update_dpp((int)j0, (int)j0, 0xa0, 0xf, 0xf, false);  // quad_perm [0,0,2,2]
    const uint32_t wbits = __float_as_uint(cxs * g.w);
    uint2 *const st = strips + ring * (NS * SSZ);
    auto put = [&](const uint32_t k) {
      // chunk j of the round -> window step u = j / 8A; inside the step r = j % 8A: adding wave r / 8, lane group r % 8
      // ((j + 0.5) / 8A is at least 1 / 16A away from an integer: the float quotient truncates exactly for j < 2^16).
      // A function of j alone -- the staging lanes do not know the round's total -- and a wave's chunks are a prefix of
      // its slot order (slot = 8 u + group), as strip_loads, the invalidation and the rare path expect.
      const uint32_t j = min(j0 + k, (uint32_t)CAP - 1u);  // (a round that does not fit is flagged below; keep the store inside the strips)
      const uint32_t u = (uint32_t)(((float)j + 0.5f) * rcpA8);
      const uint32_t r = j - u * A8;
      uint2 *const dst = k < nch ? st + (r >> 3) * SSZ + (r & 7u) * GS + u : spare_item;
      *dst = make_uint2((g.s + k * CH) * 4u, wbits);
    };
    // chunks per term written without the loop: 8 with four lanes per term (two writes each), 6 with two, 3 with one
    const uint32_t two = LOGG == 2 ? 8u : (LOGG == 1 ? 6u : 3u);
    put(sub);
    put(sub + (uint32_t)G);
    if (LOGG < 2) put(sub + 2u * (uint32_t)G);
    const bool unfit = j0 + nch > (uint32_t)CAP;
    if (__any(is_long || unfit || nch > two)) {
      bool bad = unfit;
      if (is_long && sub == 0u) {
        const uint32_t k = atomicAdd(&facts_w[2 * fs + 1], 2u) >> 1;
        if (k < (uint32_t)LONGCAP) {
          longs[ring * LONGCAP + k] = make_uint2(g.s, g.len);
          long_w[ring * LONGCAP + k] = g.w;
        } else {
          bad = true;
        }
      }
      // the round is swept straight from the index; whatever was staged is ignored
      if (bad) atomicOr(&facts_w[2 * fs + 1], 1u);
      for (uint32_t k = two + sub; __any(k < nch); k += (uint32_t)G) put(k);
    }
  };
  // the next round of this wave, first half: the round's facts and this wave's strip (LDS reads, issued ahead of the
  // current round's adds so that one LDS round trip serves both)
  struct StripRead { uint2 fc; uint2 it[U]; };
  auto strip_read = [&](StripRead &sr, const int ring, const int rank, const int fs) {
    sr.fc = facts[fs];
    const uint2 *const st = strips + (ring * NS + rank) * SSZ + (ln / LPC) * GS;
    if constexpr (GS % 2 == 0) {
#pragma unroll
      for (int u = 0; u + 1 < U; u += 2) {
        const uint4 two = *reinterpret_cast<const uint4 *>(st + u);
        sr.it[u] = make_uint2(two.x, two.y);
        sr.it[u + 1] = make_uint2(two.z, two.w);
      }
      if (U & 1) sr.it[U - 1] = st[U - 1];
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) sr.it[u] = st[u];
    }
    if (LEAN) {
      // read: now invalid.  Lane i < WIN takes window slot i (entry (i % 8) * GS + i / 8, as the staging waves place it), the
      // others their spare entry; the staging of two rounds on rewrites the slots it fills, behind two barriers
      uint2 *const own = strips + (ring * NS + rank) * SSZ + (ln & 7) * GS + (ln >> 3);
      (ln < WIN ? own : spare_item)->x = kStale;
    }
  };
  // second half: every LPC lanes take one chunk of the strip and start its posting load.  What the next round branches on
  // (its steps; is it more than a register window?) is worked out on the scalar unit here, a round before its use.
  auto strip_loads = [&](WaveWork &f, StripRead &sr, const int rank) {
    // the facts are the same in every lane: they go to the scalar unit as they are, and what this wave makes of them costs
    // the vector unit nothing (C3, with the counts below on the VALU: 49.6 vs 49.1 ms)
    const uint32_t fx = (uint32_t)__builtin_amdgcn_readfirstlane((int)sr.fc.x), fy = (uint32_t)__builtin_amdgcn_readfirstlane((int)sr.fc.y);
    const uint32_t tot = (fy & 1u) ? 0u : fx;  // (a round flagged for the direct sweep has no chunks)
    // the round's `full` whole steps hold 8 chunks of every wave; the `rem` chunks of the step behind them go to the waves
    // of rank 0, 1, .. eight at a time: the waves behind the last of them are a step short
    const uint32_t full = __umulhi(tot, magicA8);
    const int rem = (int)(tot - full * A8) - GPW * rank;  // ... from this wave's place on
    const uint32_t mine = (uint32_t)GPW * full + (uint32_t)min(max(rem, 0), GPW);
    const bool rare = fy != 0u || tot > (uint32_t)(A * WIN);
    const uint32_t steps = min(full + (rem > 0 ? 1u : 0u), (uint32_t)U);
    f.info = mine | (rare ? kRare : 0u) | (steps << 16);
    f.flags = sr.fc.y;
#pragma unroll
    for (int u = 0; u < U; ++u) asm volatile("" : "+v"(sr.it[u].x), "+v"(sr.it[u].y));
    const uint32_t lane_off = lo * 8u + (LEAN && (fy & 1u) ? kSwept : 0u);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      // a posting word of zero is no posting (segments are zero-padded to whole chunks; out-of-range reads return zero);
      // a strip slot past the wave's last chunk holds a stale descriptor: its load is sent out of range (LEAN: it was
      // invalidated when it was read, see strip_read)
      f.wq[u] = __uint_as_float(sr.it[u].y);
      const uint32_t off = LEAN ? sr.it[u].x + lane_off : ((uint32_t)(u * GPW + ln / LPC) < mine ? sr.it[u].x + lo * 8u : kOob);
      f.pc[u] = __builtin_amdgcn_raw_buffer_load_b64(rs_po, off, 0, 0);
    }
  };

  // FIXED ROLES: waves 0 .. F-1 stage every round and never add, waves F .. NW-1 add every round and never stage.  The two
  // kinds run their own loops (same two barriers per round): no per-round role arithmetic on the scalar unit, and the
  // compiler allocates registers for one job at a time.
  // BARRIER PAIRING.  The two sides execute `__syncthreads()` at different places of the source: HIP only promises a barrier
  // for one textual call reached by all threads; gfx950's s_barrier counts arriving WAVES, whichever s_barrier instruction
  // they execute, so what must hold -- and does, by construction -- is that every wave of the workgroup executes the same
  // NUMBER of barriers: 2 before the loops (the prologue below, executed by all), then exactly 2 per query v in [v0, v1) on
  // both sides (staging: one iteration per v; adding: the loop steps by two and leaves after round v when v + 1 >= v1, so an
  // odd count ends after its last round), then the epilogue's.  No path inside a round skips a barrier (`rare` rounds clear
  // the whole tile between the same two).  tests/test_gpu_even.py::test_chunk_shapes_pin_the_barrier_pairing runs chunks of
  // one, two and three queries, a short last chunk and one- and two-row batches.
  // TWO: the same with ONE barrier per query on both sides -- 2 in the prologue, 1 per v in [v0, v1) (staging: behind the
  // round's staging; adding: behind the round's adds and tests, the only one in `round`), then the same epilogue; the clears
  // are in no barrier's way (tests/test_gpu_even_planes.py runs the same chunk shapes).
  // (Tried: a staging wave taking TWO sets of terms per round -- half the staging waves, one more adding wave; C3 7 x 5
  // window steps instead of 6 x 6.  The second set's registers tipped the kernel into scratch: 140 vs 101 ms.)
  const bool stager = wv < F;
  const int rank = wv - F;  // an adding wave's rank
  WaveWork wfa, wfb;
  if constexpr (TWO) {  // "the round before the item's first": no chunks, idle lanes (its clear writes zeros over zeros)
    wfb.info = 0u;
#pragma unroll
    for (int u = 0; u < U; ++u) wfb.pc[u] = apss_u32x2{0u, 0u};
  }
  constexpr int slack = 2;  // (k_probe_coarse: the soundness argument of the coarse threshold)
  const int thr_c = (int)a.cx_theta - slack;
  const uint32_t thr1 = (uint32_t)max(thr_c, 1) - 1u;
  {
    // rounds v0 and v0 + 1 are staged before the loops start
    const TermW I0 = load_I(load_R(v0), wv, v0), I1 = load_I(load_R(v0 + 1), wv, v0 + 1);
    const Seg P0 = load_P(I0), P1 = load_P(I1);
    __syncthreads();
    if (stager) {
      flatten(P0, 0, TWO ? 3 : 0);
      flatten(P1, 1, 1);
    }
    __syncthreads();
    if (!stager) {
      StripRead sr;
      strip_read(sr, 0, rank, TWO ? 3 : 0);
      strip_loads(wfa, sr, rank);
    }
  }

  if (stager) {
    // ---- staging waves: round v loads the row extent of v + 5, the terms of v + 4, the descriptors of v + 3 and
    // stages v + 2 (every value is used a round after its load) ----
    RowExt R4 = load_R(v0 + 4);
    TermW Ic = load_I(load_R(v0 + 3), wv, v0 + 3);
    Seg Pc = load_P(load_I(load_R(v0 + 2), wv, v0 + 2));
    int r0 = 0;
    uint32_t idle = kPlane;  // WIPE: the plane this round does not add into (the item's first round adds into plane 0)
    for (int v = v0; v < v1; ++v) {
      const int r2 = r0 == 0 ? 2 : r0 - 1;  // (v + 2) % 3
      const RowExt R5 = load_R(v + 5);
      const TermW In = load_I(R4, wv, v + 4);
      const Seg Pn = load_P(Ic);
      if constexpr (WIPE) {  // this wave's share of the last round's clear (first thing in the round: see `round`)
        if (idle) wipe(plane1);
        else wipe(plane0);
        idle ^= kPlane;
      }
      flatten(Pc, r2, r2);
      if constexpr (TWO) {
        if (tid == 0) facts[r0] = make_uint2(0u, 0u);  // (read one round ago; staged again in the next round: a barrier either way)
        if constexpr (WIPE) wipe_wait();
        __syncthreads();  // the round's one barrier
      } else {
        __syncthreads();  // every add of the round has landed
        if (tid == 0) facts[r0] = make_uint2(0u, 0u);  // (read one round ago; staged again in the next round)
        __syncthreads();  // cleared: the next query starts from zero
      }
      R4 = R5;
      Ic = In;
      Pc = Pn;
      r0 = r0 == 2 ? 0 : r0 + 1;
    }
  } else {
    // ---- adding waves ----
    const int atid = tid - F * kWave, ABLOCK = A * kWave;  // thread index / count among the adding waves (sweeps, whole-tile clears)
    // TWO: the clear of a round whose postings `w` still holds, on that round's plane P (0 | 1), and the spare words' reset
    // (1 in either plane's byte)
    // (WIPE: the spare words only -- the plane is wiped whole, whatever kind of round it held, see wipe())
    auto clear_round = [&](const WaveWork &w, const uint32_t P) {
      *reinterpret_cast<uint32_t *>(smem_raw + (uint32_t)(CBMAX / APW) * 4u + (uint32_t)ln * 4u) = 0x0101u;
      if constexpr (WIPE) return;
      if ((w.info & kRare) != 0u) {
        // its postings were not all in registers: the whole plane -- its bytes of every word, by an atomic AND that leaves the
        // other plane's live sums alone (no value comes back: ds_and_b32)
        const uint32_t keep = P ? 0x00ff00ffu : 0xff00ff00u;
        for (int i = atid; i < cb / 2; i += ABLOCK) __hip_atomic_fetch_and(acc + i, keep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      } else {
        const int n = (int)((w.info >> 16) & 0xfu);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (u >= kFirstSkippable && u >= n) break;
          // (an idle lane clears slot 0 of the plane: that round's sum, or zero)
          smem_raw[(w.pc[u].x & 0xffffu) + P] = 0;
          smem_raw[(w.pc[u].y & 0xffffu) + P] = 0;
        }
      }
    };
    auto round = [&](auto plane, WaveWork &w0, WaveWork &w2, const int v, const int r0) {
      // TWO: this round's plane, a constant of each half of the loop below: it goes into the shift of an add and into the
      // immediate offset of a clear
      constexpr uint32_t P = TWO ? (uint32_t)decltype(plane)::value : 0u;
      const int r1 = r0 == 2 ? 0 : r0 + 1;
      const int q = v;
      // a crossing, reported by the wave that sees it (uniform control flow: one global atomic per wave and call)
      auto report = [&](const bool cross, const uint32_t slot, const uint32_t sum) {
        bool ok = cross;
        if (ok && mlog == 0) ok = a.ext_id[tile_row0 + slot] != a.q_ext[q];  // (merged rounds: k_expand_merged excludes)
        const uint64_t o = wave_append(ok, &a.counters[kCtrResults]);
        if (ok && o < a.res_cap) {
          a.res_q[o] = q | unmerged_mark;
          a.res_c[o] = (int32_t)(tile_row0 + slot);
          a.res_s[o] = (float)sum / cxs;  // coarse score at the crossing, replaced by k_rescore
        }
      };
      // the same from divergent control flow (sweeps): one atomic per lane
      auto report_lane = [&](const uint32_t slot, const uint32_t sum) {
        if (mlog != 0 || a.ext_id[tile_row0 + slot] != a.q_ext[q]) {
          const uint64_t o = atomicAdd(&a.counters[kCtrResults], 1ull);
          if (o < a.res_cap) {
            a.res_q[o] = q | unmerged_mark;
            a.res_c[o] = (int32_t)(tile_row0 + slot);
            a.res_s[o] = (float)sum / cxs;
          }
        }
      };
      auto slot_of = [&](const uint32_t pcw) { return WIDE ? pcw >> 15 : (SLOT2 && (!ACC8 || TWO) ? (pcw & 0xffffu) >> 1 : pcw & 0xffffu); };
      auto prod = [&](const uint32_t pcw, const float wqs) {
        const float x = __builtin_fmaf(wqs, __half2float(__ushort_as_half((unsigned short)(WIDE ? pcw & 0x7fffu : pcw >> 16))), 1.0f);
        return SIGNED ? (uint32_t)max((int)x, 1) : (uint32_t)x;
      };
      auto half_of = [&](const uint32_t old_word, const uint32_t pcw) {
        if (WIDE) return __builtin_amdgcn_ubfe(old_word, (pcw >> 12) & 24u, 8u);
        if (WIPE) return __builtin_amdgcn_ubfe(old_word, pcw << 2, 8u);  // (byte slot % 4 of the plane's word: 8 (slot % 4) in the low five bits)
        if (TWO) return __builtin_amdgcn_ubfe(old_word, (pcw << 3) + 8u * P, 8u);  // (bit 0 of a posting is zero: 16 (slot % 2) + 8 P in the low five bits)
        return SLOT2 ? __builtin_amdgcn_ubfe(old_word, pcw << 3, ABITS) : (old_word >> ((pcw & 1u) << 4)) & 0xffffu;
      };
      constexpr int BATCH = 3;  // (one batch of all six steps of C3's window: no change, 101.1 ms)
      // An idle lane (zero word) adds into ITS OWN spare word behind the accumulators (a select on the address) instead of
      // being masked off: an exec mask around each atomic is a trip VALU -> scalar unit -> VALU (compare, s_and_saveexec,
      // s_or) that cost ~64 cycles of the wave's serial issue per posting slot (profiles/microbench/issue_rate.hip).  Its
      // "old value" is replaced by thr1 + 1 afterwards: never a first touch (not 0), never a crossing (thr1 - old wraps).
      // (LEAN, window path: not replaced -- the spare word's low accumulator is in [1, 2 U (NW - 1)], see check_batch)
      const uint32_t spare = (uint32_t)(CBMAX / APW) * 4u + (uint32_t)ln * 4u;
      auto add_or_spare = [&](const uint32_t pcw, const uint32_t p) -> uint32_t {
        if constexpr (WIPE) {
          // byte `slot` of plane P: the word at (slot & ~3) = (pcw >> 1) & 0x7ffc, shift 8 (slot % 4) = the low five bits of
          // pcw << 2 (bit 0 of a posting is zero), the plane in the instruction's immediate offset.  One vector instruction
          // more than the interleaved planes' add -- the one their clear spent on its address.  An idle lane adds 1 to byte 0
          // of its spare word in either plane's rounds (its address less the plane's offset: the immediate puts it back)
          const uint32_t at = pcw ? (pcw >> 1) & 0x7ffcu : spare - kPlane * P;
          return atomicAdd(reinterpret_cast<uint32_t *>(smem_raw + kPlane * P + at), p << ((pcw << 2) & 31u));
        }
        if constexpr (TWO) {
          // byte 2 slot + P: the word of the 16-bit kernel's address, shift 16 (slot % 2) + 8 P -- instruction for instruction
          // the 16-bit add ((pcw << 3) + 8 P is one v_lshl_add_u32); an idle lane adds 1 to its spare word's byte P
          return atomicAdd(reinterpret_cast<uint32_t *>(smem_raw + (pcw ? pcw & 0xfffcu : spare)), p << (((pcw << 3) + 8u * P) & 31u));
        }
        const uint32_t addr = WIDE ? (pcw >> 15) & 0x1fffcu : (SLOT2 ? pcw & 0xfffcu : ((pcw & 0xffffu) >> 1) * 4u);
        const uint32_t sh = WIDE ? (pcw >> 12) & 24u : (SLOT2 ? (pcw << 3) & 31u : (pcw & 1u) << 4);
        return atomicAdd(reinterpret_cast<uint32_t *>(smem_raw + (pcw ? addr : spare)), p << sh);
      };
      // two postings of a sweep the same way: no masks around the atomics, one (rare, divergent) branch for both crossings
      auto visit2 = [&](const uint32_t x, const uint32_t y, const float wqs) {
        const uint32_t px = prod(x, wqs), py = prod(y, wqs);
        // (LEAN: a sweep's idle lanes add nothing -- the spare words' bound is the window's)
        uint32_t ox = add_or_spare(x, LEAN && x == 0u ? 0u : px), oy = add_or_spare(y, LEAN && y == 0u ? 0u : py);
        ox = x ? half_of(ox, x) : thr1 + 1u;
        oy = y ? half_of(oy, y) : thr1 + 1u;
        my_cands += (ox == 0u ? 1u : 0u) + (oy == 0u ? 1u : 0u);
        if ((thr1 - ox < px) | (thr1 - oy < py)) {
          if (thr1 - ox < px) report_lane(slot_of(x), ox + px);
          if (thr1 - oy < py) report_lane(slot_of(y), oy + py);
        }
      };
      const int n_steps = (int)((w0.info >> 16) & 0xfu);  // (scalar: a branch on it costs no trip from the VALU)
      if (LEAN) n_seen -= 2u * (uint32_t)max(n_steps, kFirstSkippable);  // the slots the batches below test
      auto issue_batch = [&](const int u0, uint32_t (&p0)[BATCH], uint32_t (&p1)[BATCH], uint32_t (&o0)[BATCH], uint32_t (&o1)[BATCH]) {
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
          const int u = u0 + j;
          if (u >= kFirstSkippable && u >= n_steps) break;  // (one forward exit: the steps behind this wave's last chunk)
          if (u < U) {
            p0[j] = prod(w0.pc[u].x, w0.wq[u]);
            p1[j] = prod(w0.pc[u].y, w0.wq[u]);
            o0[j] = add_or_spare(w0.pc[u].x, p0[j]);
            o1[j] = add_or_spare(w0.pc[u].y, p1[j]);
          }
        }
      };
      auto check_batch = [&](const int u0, uint32_t (&p0)[BATCH], uint32_t (&p1)[BATCH], uint32_t (&o0)[BATCH], uint32_t (&o1)[BATCH]) {
        if constexpr (LEAN) {
          // one add per posting and one max per pair: the largest old + product of the batch passes thr1 iff some add of it
          // crossed or landed on a sum that had crossed before (true pairs only; the exact test is below, where it is rare).
          // An idle lane's old value is its spare word's: >= 1, so it counts itself as seen, and its sum is a few hundred at
          // the most -- below it, a threshold merely sends the batch through the exact test.
          uint32_t top = 0;
#pragma unroll
          for (int j = 0; j < BATCH; ++j) {
            const int u = u0 + j;
            if (u >= kFirstSkippable && u >= n_steps) break;
            if (u < U) {
              o0[j] = half_of(o0[j], w0.pc[u].x);
              o1[j] = half_of(o1[j], w0.pc[u].y);
              // (written out: the compiler turns min(old, 1) back into a compare, a select and a carry chain with its waits)
              uint32_t s0, s1;
              asm("v_min_u32 %0, 1, %1" : "=v"(s0) : "v"(o0[j]));
              asm("v_min_u32 %0, 1, %1" : "=v"(s1) : "v"(o1[j]));
              n_seen += s0 + s1;
              top = max(max(top, o0[j] + p0[j]), o1[j] + p1[j]);
            }
          }
          if (__any(top > thr1)) {
#pragma unroll
            for (int j = 0; j < BATCH; ++j) {
              const int u = u0 + j;
              if (u >= kFirstSkippable && u >= n_steps) break;
              if (u < U) {
                const uint32_t a0 = w0.pc[u].x ? o0[j] : thr1 + 1u, a1 = w0.pc[u].y ? o1[j] : thr1 + 1u;  // (an idle lane never crosses)
                report(thr1 - a0 < p0[j], slot_of(w0.pc[u].x), a0 + p0[j]);
                report(thr1 - a1 < p1[j], slot_of(w0.pc[u].y), a1 + p1[j]);
              }
            }
          }
          return;
        }
        // first touches and crossings are counted per lane (VALU only); one trip to the scalar unit per batch decides
        // whether any lane crossed
        uint32_t n_cross = 0;
#pragma unroll
        for (int j = 0; j < BATCH; ++j) {
          const int u = u0 + j;
          if (u >= kFirstSkippable && u >= n_steps) break;
          if (u < U) {
            o0[j] = w0.pc[u].x ? half_of(o0[j], w0.pc[u].x) : thr1 + 1u;
            o1[j] = w0.pc[u].y ? half_of(o1[j], w0.pc[u].y) : thr1 + 1u;
            my_cands += (o0[j] == 0u ? 1u : 0u) + (o1[j] == 0u ? 1u : 0u);
            n_cross += (thr1 - o0[j] < p0[j] ? 1u : 0u) + (thr1 - o1[j] < p1[j] ? 1u : 0u);
          }
        }
        if (__any(n_cross != 0u)) {
#pragma unroll
          for (int j = 0; j < BATCH; ++j) {
            const int u = u0 + j;
            if (u >= kFirstSkippable && u >= n_steps) break;
            if (u < U) {
              report(thr1 - o0[j] < p0[j], slot_of(w0.pc[u].x), o0[j] + p0[j]);
              report(thr1 - o1[j] < p1[j], slot_of(w0.pc[u].y), o1[j] + p1[j]);
            }
          }
        }
      };
      // TWO: the round before this one is cleared here, on the OTHER plane, from the registers that still hold its postings
      // (strip_loads below overwrites them), directly ahead of this round's adds: one drain serves both
      if constexpr (TWO) clear_round(w2, P ^ 1u);
      // WIPE: this wave's share of that clear, the first LDS work of the round in either role: behind the barrier the LDS
      // queue is empty, and the stores are through before the round's first adds come back.  (Every other place tried for
      // them, and every smaller set of waves, measured slower on C3, the staging waves alone slower than the per-posting
      // clears: profiles/even_wipe.md, section 1)
      if constexpr (WIPE) wipe(std::integral_constant<int, (int)(P ^ 1u)>{});
      StripRead sr;
      strip_read(sr, r1, rank, r1);
      {
        uint32_t p0[BATCH], p1[BATCH], o0[BATCH], o1[BATCH];
        issue_batch(0, p0, p1, o0, o1);
        // (nothing that waits for the strip or the facts may be scheduled ahead of the adds' issue)
        asm volatile("" : "+v"(sr.fc.x), "+v"(sr.fc.y) : : "memory");
        __builtin_amdgcn_sched_barrier(0);
        strip_loads(w2, sr, rank);
        check_batch(0, p0, p1, o0, o1);
      }
#pragma unroll
      for (int u0 = BATCH; u0 < U; u0 += BATCH) {
        uint32_t p0[BATCH], p1[BATCH], o0[BATCH], o1[BATCH];
        issue_batch(u0, p0, p1, o0, o1);
        check_batch(u0, p0, p1, o0, o1);
      }
      const bool rare = (w0.info & kRare) != 0u;  // more than the register windows: one branch per round
      if (rare) {
        const uint32_t flags = (uint32_t)__builtin_amdgcn_readfirstlane((int)w0.flags);
        const int mc = (int)(w0.info & kCountMask);
        if (mc > WIN) {  // chunks past the register window: straight from this wave's strip
          const uint2 *const st = strips + (r0 * NS + rank) * SSZ;
          for (int c0 = WIN; c0 < mc; c0 += GPW) {
            const int c = c0 + ln / LPC;
            const int cc = min(c, SLOTS - 1);
            const uint2 it = st[(cc & 7) * GS + (cc >> 3)];
            const apss_u32x2 two = __builtin_amdgcn_raw_buffer_load_b64(rs_po, c < mc ? it.x + lo * 8u : kOob, 0, 0);
            visit2(two.x, two.y, __uint_as_float(it.y));
          }
        }
        if (flags & 1u) {  // flagged at staging: every term straight from the index, one term per adding wave at a time
          RowExt cur = load_R(v);
          cur.nnz -= cur.qb;
          cur.qb -= qbase_lo;
          const float qsv = SHARD && !MERGE ? uniform_load(a.q_scale + v) : 1.0f;
          const float iq = qsv > 0.f ? 1.0f / qsv : 0.f;
          for (int k = rank; k < cur.nnz; k += A) {
            const uint32_t off = (uint32_t)(cur.qb + k) * 4u;
            const uint32_t term = __builtin_amdgcn_raw_buffer_load_b32(rs_qi, off, 0, 0);
            const float wq_ = cxs * __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs_qv, off, 0, 0)) * iq;
            const apss_u32x2 sg = __builtin_amdgcn_raw_buffer_load_b64(rs_tp, term * 8u, 0, 0);
            for (uint32_t p = 2u * (uint32_t)ln; p < sg.y; p += 2u * kWave) {
              const apss_u32x2 two = __builtin_amdgcn_raw_buffer_load_b64(rs_po, (sg.x + p) * 4u, 0, 0);
              visit2(two.x, p + 1u < sg.y ? two.y : 0u, wq_);
            }
          }
        } else {
          const uint32_t n_long = min(flags >> 1, (uint32_t)LONGCAP);
          for (uint32_t j = 0; j < n_long; ++j) {  // long segments: swept by all adding waves, two postings per lane and pass
            const uint2 sgm = longs[r0 * LONGCAP + j];
            const float wq_ = cxs * long_w[r0 * LONGCAP + j];
            for (uint32_t k = 2u * (uint32_t)atid; k < sgm.y; k += 2u * (uint32_t)ABLOCK) {
              const apss_u32x2 a0 = __builtin_amdgcn_raw_buffer_load_b64(rs_po, (sgm.x + k) * 4u, 0, 0);
              visit2(a0.x, k + 1u < sgm.y ? a0.y : 0u, wq_);
            }
          }
        }
      }
      if constexpr (WIPE) wipe_wait();  // (the stores of the round's top: long landed, but the compiler does not know of them)
      __syncthreads();  // every add of the round has landed
      if constexpr (TWO) return;  // (the round's one barrier: its clear is the next round's first act)

      if (LEAN) *reinterpret_cast<uint32_t *>(smem_raw + spare) = 1u;  // the idle lanes' word starts every round at 1
      if (rare) {  // (long or direct sweeps, or chunks past the window: their postings are not in registers) whole-tile clear
        for (int i = atid * 4; i < cb / APW; i += ABLOCK * 4) *reinterpret_cast<uint4 *>(acc + i) = make_uint4(0u, 0u, 0u, 0u);
      } else {
        unsigned short *acc16w = reinterpret_cast<unsigned short *>(acc);
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (u >= kFirstSkippable && u >= n_steps) break;
          // unconditional: an idle lane (zero word) clears slot 0, which is zero at the end of a query either way
          if (WIDE) {
            smem_raw[w0.pc[u].x >> 15] = 0;
            smem_raw[w0.pc[u].y >> 15] = 0;
          } else if (SLOT2 && ACC8) {
            smem_raw[w0.pc[u].x & 0xffffu] = 0;
            smem_raw[w0.pc[u].y & 0xffffu] = 0;
          } else if (SLOT2) {
            *reinterpret_cast<unsigned short *>(smem_raw + (w0.pc[u].x & 0xffffu)) = 0;
            *reinterpret_cast<unsigned short *>(smem_raw + (w0.pc[u].y & 0xffffu)) = 0;
          } else {
            acc16w[w0.pc[u].x & 0xffffu] = 0;
            acc16w[w0.pc[u].y & 0xffffu] = 0;
          }
        }
      }
      __syncthreads();  // cleared: the next query starts from zero
    };
    int r0 = 0;
    constexpr std::integral_constant<int, 0> even_round{};
    constexpr std::integral_constant<int, TWO ? 1 : 0> odd_round{};
    for (int v = v0; v < v1; v += 2) {
      round(even_round, wfa, wfb, v, r0);
      r0 = r0 == 2 ? 0 : r0 + 1;
      if (v + 1 >= v1) break;
      round(odd_round, wfb, wfa, v + 1, r0);
      r0 = r0 == 2 ? 0 : r0 + 1;
    }
    if constexpr (TWO && !WIPE) {  // the last round's clear, behind its barrier: a later item of this workgroup finds both planes zero
      if ((v1 - v0) & 1) clear_round(wfa, 0u);
      else clear_round(wfb, 1u);
    }
  }
  if constexpr (WIPE) {  // the same as a wipe of the last round's plane, by every wave (both roles are behind the item's last barrier)
    if ((v1 - v0) & 1) wipe(plane0);
    else wipe(plane1);
    wipe_wait();
  }
  __syncthreads();
  if (tid < 3) stat[tid] = 0;
  __syncthreads();
  atomicAdd(&stat[0], my_visits);
  atomicAdd(&stat[1], (unsigned long long)(my_cands - n_seen));
  __syncthreads();
  if (tid == 0) {
    const unsigned long long twice = a.tri && tile < qtile ? 2ull : 1ull;  // (both counts are symmetric in the two tiles)
    atomicAdd(&a.counters[kCtrVisits], stat[0] * twice);
    atomicAdd(&a.counters[kCtrCands], stat[1] * twice);
    atomicAdd(&a.counters[kCtrDevVisits], stat[0]);
  }
}

// PERSISTENT LAUNCH (ProbeArgs::items; apss_worklist.hpp).  The launch holds as many workgroups as the chip keeps
// resident; each takes the next ITEM {tile, rounds [v0, v1)} of the launch's work list -- one lane, a returning global atomic
// on a.work_ctr -- runs it as the grid launch's workgroup ran its cell, and comes back for another until the list is spent.
// The index reaches the other waves through LDS behind a barrier that EVERY wave executes (BARRIER PAIRING above: one more
// per take, in every wave, the failed last take included).  No workgroup ever waits for another one -- no spin, no flag, no
// grid barrier; all a workgroup shares with the others is the counter -- so a launch of more workgroups than are resident
// is merely wasteful (the surplus starts when a slot falls free and finds the list spent), never stuck.
// Between items only what an item's start needs is redone (probe_even_item, `first`).  Everything per item -- tile, rounds,
// own_tile, the buffer descriptors -- is re-derived from the item, on the scalar unit.  Statistics are flushed per item
// (`twice` depends on the item's tile).  Without a list (APSS_DEBUG=no_persist) workgroup b runs the one cell that blockIdx
// names, derived here as work_cell() derives it on the host, and leaves.
template <int BLOCK, int U, int LONGCAP, bool SHARD, bool SIGNED, bool ACC8, bool MERGE, bool TWO = false>
__device__ __forceinline__ void probe_even_body(const ProbeArgs &a) {
  // the grid launch's one cell, worked out before the loop and handed to it in three scalars (left inside the loop the
  // derivation is a loop invariant: hoisted with its intermediate values, 64-bit quotients among them, and kept across the item)
  int g_tile = 0, g_v0 = 0, g_v1 = 0;
  if (!a.items) {
    const int cb = a.cb, mlaunch = MERGE ? a.merge_log2 : 0;
    const int tile = a.tile0 + blockIdx.x / a.n_chunks;
    const int c0 = (blockIdx.x % a.n_chunks) * a.q_chunk;
    const int row_lo = c0 << mlaunch, row_hi = MERGE ? min(a.nq_rows, (c0 + a.q_chunk) << mlaunch) : 0;  // this workgroup's query rows
    const bool own_tile = mlaunch != 0 && a.q_slot_base >= 0 && (a.q_slot_base + row_lo) / cb <= tile && tile <= (a.q_slot_base + row_hi - 1) / cb;
    if (a.tri && tile > row_lo / cb) return;  // the mirrored half (ProbeArgs::tri): before any barrier, the whole workgroup
    g_tile = tile | (own_tile ? kUnmergedBit : 0);  // (tiles number far below 2^30)
    g_v0 = own_tile ? row_lo : c0;
    g_v1 = own_tile ? row_hi : min(a.nq, c0 + a.q_chunk);
    asm volatile("" : "+s"(g_tile), "+s"(g_v0), "+s"(g_v1));
  }
  __shared__ int next_item;
  for (bool first = true;; first = false) {
    int tile, v0, v1;
    bool own_tile;
    if (a.items) {
      if (threadIdx.x == 0) next_item = (int)atomicAdd(a.work_ctr, 1ull);
      __syncthreads();  // (the next write of next_item lies behind the item's own barriers)
      const int idx = __builtin_amdgcn_readfirstlane(next_item);
      if (idx >= a.n_items) return;
      const ProbeItem *const it = a.items + idx;  // (16 B: one scalar load)
      tile = uniform_load(&it->tile);
      v0 = uniform_load(&it->v0);
      v1 = uniform_load(&it->v1);
      own_tile = uniform_load(&it->own) != 0;
    } else {
      if (!first) return;
      tile = g_tile & ~kUnmergedBit;
      v0 = g_v0;
      v1 = g_v1;
      own_tile = (g_tile & kUnmergedBit) != 0;
    }
    // The item reads the launch's arguments through a pointer to the kernarg segment (the kernel's one parameter lies at its
    // start) that is opaque per item: read through `a` they are loop invariants, hoisted out of this loop and kept in SGPRs
    // across the whole item on top of what the item derives from them -- the kernels sit at their SGPR limit as it is
    // (DESIGN.md 5a): 48 scalar spills in the flagship instantiation against 11 this way (the grid launch had 3).
    ProbeArgsK *ak = reinterpret_cast<ProbeArgsK *>(reinterpret_cast<uintptr_t>(__builtin_amdgcn_kernarg_segment_ptr()));
    asm volatile("" : "+s"(ak));
    probe_even_item<BLOCK, U, LONGCAP, SHARD, SIGNED, ACC8, MERGE, TWO>(*ak, tile, v0, v1, own_tile, first);
  }
}

template <int BLOCK, int U, int LONGCAP, bool SHARD, bool SIGNED, bool ACC8>
__global__ __launch_bounds__(BLOCK, BLOCK <= 512 ? 2 * BLOCK / 256 : BLOCK / 256) void k_probe_even(const ProbeArgs a) {
  probe_even_body<BLOCK, U, LONGCAP, SHARD, SIGNED, ACC8, false>(a);
}

// the same rounds with M = 2^merge_log2 neighbouring query rows each (a term shard's thin rounds; see MERGED rounds above)
template <int U, bool ACC8>
__global__ __launch_bounds__(512, 4) void k_probe_even_merged(const ProbeArgs a) {
  probe_even_body<512, U, 128, true, false, ACC8, true>(a);
}

// the plain 512-thread rounds with TWO PLANES of 8-bit sums over <= 32768-row tiles and one barrier per round (see the header)
template <int U>
__global__ __launch_bounds__(512, 4) void k_probe_planes(const ProbeArgs a) {
  probe_even_body<512, U, 128, false, false, true, false, true>(a);
}

}  // namespace apss
