package cpslab.gpu

/** JNI face of libapss_hip.so (include/apss.h); see all-pairs-similarity_amd/jvm/apss_jni.c.
  * Not compiled in the build image (no JVM there); it is the binding a maintainer adds to `core/`. */
object NativeApss {
  System.loadLibrary("apss_jni")
  val FLAG_VALUE_PRUNE = 1
  val FLAG_ADMISSION = 2
  val FLAG_NORMALIZE = 4
  val FLAG_NO_SYMMETRY = 64 // a batch that is the whole store is probed in both directions, as IndexingWorkerActor does (include/apss.h)
  val TOP_K_MAX = 1024
  /** headTerms: dense-head block of the library (0 = it decides from the term distribution, -1 = never).
    * topK: 0 = every pair >= theta; 1 .. TOP_K_MAX = at most that many candidates per query, the best by (score descending,
    * candidate id ascending), the results grouped by query in rank order (apss_set_top_k).  A topK the library refuses
    * fails the create: 0 is returned and lastError(0) says why.
    * topKTileCut: 0 = off; 1 = with topK > 0 and theta <= 0 the probe kernel cuts every (query row, tile) round to the pairs
    * that can be among a query's topK before it writes them (apss_set_top_k_tile_cut): the same reply, a shorter list to cut */
  @native def create(dim: Int, theta: Double, indexThreshold: Double, flags: Int, device: Int, topKTileCut: Int,
                     headTerms: Int, topKWindowPairs: Long, topK: Int): Long
  val TOP_PAIRS_MAX = 1 << 20
  /** the global top-K (include/apss.h, apss_set_top_pairs; one handle only, a group has none): 0 = off; 1 .. TOP_PAIRS_MAX = every
    * later reply holds the `pairs` best pairs of its whole batch, by (score descending, query id, candidate id ascending), in
    * that order -- behind topK's per-query cut when both are set.  Travels through `submit` (mode 7 of apss_jni.c): no further
    * native entry point.  Returns 0 or a negative status (lastError(h) says why) */
  def setTopPairs(h: Long, pairs: Long): Int =
    submit(h, 7, Array(0L, 0L), new Array[Int](0), new Array[Double](0), Array(pairs)).toInt
  /** near-duplicate groups (include/apss.h, apss_set_components; one handle only, a group has none): on = the connected
    * components of the graph "stored vector - stored vector, edge = a pair of a reply" are kept on the device across calls; off
    * frees them.  Travels through `submit` (mode 8 of apss_jni.c): no further native entry point.  0 or a negative status */
  def setComponents(h: Long, on: Boolean): Int =
    submit(h, 8, Array(0L, 0L), new Array[Int](0), new Array[Double](0), Array(if (on) 1L else 0L)).toInt
  /** the groups across remove and compact (include/apss.h, apss_set_components_repair; one handle only): 0 = off; maxRows in
    * 1 .. 2^31 - 1 = a remove re-joins the live vectors of the groups it touched, at most maxRows of them (more: every group is
    * forgotten, as with 0), and a compaction keeps the groups.  Travels through `submit` (mode 10 of apss_jni.c).  0 or a negative
    * status */
  def setComponentsRepair(h: Long, maxRows: Long): Int =
    submit(h, 10, Array(0L, 0L), new Array[Int](0), new Array[Double](0), Array(maxRows)).toInt
  /** the groups as they are now: for every store slot, in slot order, (the smallest slot of its component | -1 for a removed
    * vector, the id of the vector in that slot | the removed vector's own).  Rides on `submit` (mode 9: apss_components_get, the
    * slots labelled) and on `fetch` with minus that count (apss_components_fetch).  null when the setting is off or on an error
    * (lastError(h) says why) */
  def components(h: Long): (Array[Int], Array[Long]) = {
    val rows = submit(h, 9, Array(0L), new Array[Int](0), new Array[Double](0), new Array[Long](0))
    if (rows < 0) return null
    val label = new Array[Long](rows.toInt); val rep = new Array[Long](rows.toInt)
    if (rows > 0 && fetch(h, -rows, label, rep, new Array[Float](rows.toInt)) != 0) return null
    (label.map(_.toInt), rep)
  }
  @native def destroy(h: Long): Unit
  @native def lastError(h: Long): String
  /** mode 0 insert, 1 query on the frozen index, 2 insert-and-query; returns #results or a negative status */
  @native def submit(h: Long, mode: Int, rowptr: Array[Long], indices: Array[Int], values: Array[Double],
                     ids: Array[Long]): Long
  @native def fetch(h: Long, count: Long, outQ: Array[Long], outC: Array[Long], outScore: Array[Float]): Int
  // ---- removal of stored vectors (include/apss.h, apss_remove / apss_compact / apss_set_auto_compact; one handle only, a group
  // has none).  They travel through `submit` (modes 3, 4, 5 of apss_jni.c): no further native entry point.
  /** forget every stored vector whose id is in `ids`: later replies hold no pair with them.  Returns the rows newly marked or a
    * negative status; ids that are unknown, removed already or repeated count for nothing */
  def remove(h: Long, ids: Array[Long]): Long =
    submit(h, 3, new Array[Long](ids.length + 1), new Array[Int](0), new Array[Double](0), ids)
  /** rebuild store and index from the live vectors, on the device; the last results are gone.  0 or a negative status */
  def compact(h: Long): Int = submit(h, 4, Array(0L), new Array[Int](0), new Array[Double](0), new Array[Long](0)).toInt
  /** cpslab.allpair.gpu.autoCompact: compact before an insert once more than `fraction` (in [0, 1); 0 = off) of the stored
    * vectors is removed.  0 or a negative status */
  def setAutoCompact(h: Long, fraction: Double): Int = submit(h, 5, Array(0L, 1L), Array(0), Array(fraction), Array(0L)).toInt
  /** "what is similar to these vectors that you already hold?" (include/apss.h, apss_query_stored; one handle only): every live
    * stored vector whose id is in `ids` is queried against the store exactly as it is stored, on the device; nothing is
    * inserted.  Travels through `submit` (mode 6 of apss_jni.c).  Returns #results (then `fetch`) or a negative status; ids that
    * are unknown, removed or repeated ask nothing more */
  def queryStored(h: Long, ids: Array[Long]): Long =
    submit(h, 6, new Array[Long](ids.length + 1), new Array[Int](0), new Array[Double](0), ids)
  /** name the dense-head block's terms instead of the library's policy (include/apss.h, apss_set_head_terms; a handle made by
    * `create` holds the whole term space: part = 0, nParts = 1); empty handle only.  Returns 0 or a negative status.
    * (Term-sharded deployments do not call this: a group -- createGroup -- gives its members their shares itself.) */
  @native def setHeadTerms(h: Long, terms: Array[Int], part: Int, nParts: Int): Int
  /** how many of the 256 columns of a head of more than 256 terms are FOLDED columns: 64 | 128 | 192 (0 = the default, 128);
    * the other 256 - columns most frequent terms keep a column each.  Takes effect at the next setHeadTerms */
  @native def setHeadFold(h: Long, columns: Int): Int
  /** the block's terms, chosen by the library or set by setHeadTerms (what one shard's policy decided is what its peers are given) */
  @native def headTerms(h: Long): Array[Int]

  // ---- apss_group: the term-sharded index of one node behind one object (include/apss.h).  Member i lives on devices(i) and
  // owns a contiguous term range cut on the first batch; every batch is handed WHOLE to every member; the exchange of the
  // members' answers (all-gather of candidate lists, RCCL all-reduce of per-candidate partial scores) runs below this call.
  val GROUP_FORCE_EXCHANGE = 1
  val GROUP_NO_RCCL = 2
  val GROUP_ADAPT_LAYOUT = 4 // re-decide term cuts and shared head as the store grows (include/apss.h)
  /** returns the group's handle or 0 (groupLastError(0) says why).  topK as for `create` (apss_group_set_top_k: the cut runs
    * behind the members' exchange); a grid (rowRanges > 1) supports only topK = 0 */
  @native def createGroup(dim: Int, theta: Double, indexThreshold: Double, flags: Int, devices: Array[Int], headTerms: Int,
                          groupFlags: Int, topK: Int): Long
  val GROUP_NO_SYMMETRIC_RANGES = 8 // grids: every cell meets every other row range, nothing is mirrored
  /** A T x D grid (apss_group_create_grid): devices.length = T x rowRanges, member (row range j, term range i) lives on
    * devices(j * T + i); a batch's rows are spread over the row ranges, every call answers as one handle would.  rowRanges
    * (1..64) travels in bits 16..23 of createGroup's groupFlags: one native entry point creates both shapes.
    * Returns 0 when rowRanges does not divide devices.length (and as createGroup). */
  def createGroupGrid(dim: Int, theta: Double, indexThreshold: Double, flags: Int, devices: Array[Int], headTerms: Int,
                      groupFlags: Int, rowRanges: Int, topK: Int = 0): Long =
    if (rowRanges < 1 || rowRanges > 64 || devices.length % rowRanges != 0) 0L
    else createGroup(dim, theta, indexThreshold, flags, devices, headTerms, (groupFlags & 0xffff) | (rowRanges << 16), topK)
  @native def destroyGroup(g: Long): Unit
  @native def groupLastError(g: Long): String
  /** mode 0 insert, 1 query on the frozen index, 2 insert-and-query; returns #results or a negative status */
  @native def groupSubmit(g: Long, mode: Int, rowptr: Array[Long], indices: Array[Int], values: Array[Double],
                          ids: Array[Long]): Long
  @native def groupFetch(g: Long, count: Long, outQ: Array[Long], outC: Array[Long], outScore: Array[Float]): Int
  /** out(0..8) = members, exchange (0 none, 1 copies, 2 RCCL), head terms, rows, candidates summed over the members, distinct
    * candidates, result pairs, bytes all-gathered per member, bytes all-reduced -- of the last call */
  @native def groupStats(g: Long, out: Array[Long]): Int
}
