package cpslab.deploy.server

import scala.collection.mutable
import scala.concurrent.duration._
import scala.language.postfixOps

import akka.actor.{Actor, ActorSelection, Cancellable, ReceiveTimeout}
import com.typesafe.config.Config
import cpslab.gpu.NativeApss
import cpslab.message._

/** Drop-in for IndexingWorkerActor (core/src/main/scala/cpslab/deploy/server/IndexingWorkerActor.scala): same
  * messages in (IndexData, IOTicket, ReceiveTimeout, Test), same SimilarityOutput out, same config keys; the
  * vectorsStore / invertedIndex / calculateSimilarity loop is replaced by one JNI call per batch.
  * EntryProxyActor.handleDataPacket keeps sending it IndexData; with the GPU index a single worker per entry is enough
  * (maxIndexEntryActorNum = 1, maxShardNum = 1), since every worker of the reference recomputes the same full score anyway;
  * the term sharding of a multi-GPU node happens INSIDE the library (cpslab.allpair.gpu.devices, below).
  * Source only: not compiled in the build image (no JVM there). */
private class GpuIndexingWorkerActor(conf: Config) extends Actor {
  val similarityThreshold = conf.getDouble("cpslab.allpair.similarityThreshold")
  val vectorDim = conf.getInt("cpslab.allpair.vectorDim")
  val outputWritingDuration = conf.getLong("cpslab.allpair.outputIODuration")
  val writeBuffer = new mutable.HashMap[String, mutable.HashMap[String, Double]]
  private val expDuration = conf.getLong("cpslab.allpair.benchmark.expDuration")
  // WriteWorkerActor.scala:35,188-194 drops entries <= indexThreshold before a vector reaches this actor; the key is read here
  // too so that a deployment that feeds the actor directly gets the same pruning on the device
  private val indexThreshold =
    if (conf.hasPath("cpslab.allpair.indexThreshold")) conf.getDouble("cpslab.allpair.indexThreshold") else 0.0
  // Where the index lives.  cpslab.allpair.gpu.devices = [0, 1, .., 7]: the term-sharded index of the node -- one member per
  // listed GPU owning a contiguous term range, the exchange of partial scores over RCCL below the JNI boundary (apss_group,
  // include/apss.h): the reference's own fan-out of a DataPacket to maxShardNum x maxIndexEntryActorNum term workers
  // (WriteWorkerActor.scala:164-183, EntryProxyActor.scala:37-49) done inside the library.  One entry, or only
  // cpslab.allpair.gpu.device: one handle in one GPU's HBM.
  private val devices: Array[Int] =
    if (conf.hasPath("cpslab.allpair.gpu.devices")) {
      val l = conf.getIntList("cpslab.allpair.gpu.devices"); Array.tabulate(l.size)(i => l.get(i).intValue)
    } else Array(if (conf.hasPath("cpslab.allpair.gpu.device")) conf.getInt("cpslab.allpair.gpu.device") else 0)
  private val headTerms = if (conf.hasPath("cpslab.allpair.gpu.headTerms")) conf.getInt("cpslab.allpair.gpu.headTerms") else 0
  private val flags = if (indexThreshold > 0.0) NativeApss.FLAG_VALUE_PRUNE else 0
  // cpslab.allpair.gpu.rowRanges = D (default 1): the listed GPUs form a T x D grid, T = devices.length / D term ranges x D row
  // ranges -- the reference's second sharding level (EntryProxyActor.scala:37-49) as ranges of rows; member (row range j, term
  // range i) on devices(j * T + i).  Not with adaptiveLayout (a grid is given its cuts by name or keeps the first batch's).
  private val rowRanges = if (conf.hasPath("cpslab.allpair.gpu.rowRanges")) conf.getInt("cpslab.allpair.gpu.rowRanges") else 1
  require(rowRanges >= 1 && devices.length % rowRanges == 0, "cpslab.allpair.gpu.rowRanges must divide the number of devices")
  private val grouped = devices.length > 1
  // cpslab.allpair.gpu.adaptiveLayout = true: the group re-decides its term cuts and shared head as the index grows
  // (APSS_GROUP_ADAPT_LAYOUT): a stream of single vectors from an empty index does not keep its first message's layout
  private val groupFlags =
    if (conf.hasPath("cpslab.allpair.gpu.adaptiveLayout") && conf.getBoolean("cpslab.allpair.gpu.adaptiveLayout"))
      NativeApss.GROUP_ADAPT_LAYOUT
    else 0
  // cpslab.allpair.gpu.topK = k (default 0: every pair >= similarityThreshold, as the reference): each query's reply holds at
  // most k candidates, the best by (score descending, candidate id ascending).  A grid (rowRanges > 1) does not support it: the
  // worker says so and runs with 0
  private val topKConf = if (conf.hasPath("cpslab.allpair.gpu.topK")) conf.getInt("cpslab.allpair.gpu.topK") else 0
  private val topK = if (grouped && rowRanges > 1 && topKConf != 0) {
    System.err.println("GpuIndexingWorkerActor: cpslab.allpair.gpu.topK is not supported with cpslab.allpair.gpu.rowRanges > 1; running with 0")
    0
  } else topKConf
  // cpslab.allpair.gpu.topKWindowPairs = P (default 0: off; one GPU only): with topK > 0 a call is joined and cut in windows of
  // query rows that hold at most about P uncut pairs each (apss_set_top_k_window) -- what makes similarityThreshold = 0 fit
  private val topKWindowPairs =
    if (conf.hasPath("cpslab.allpair.gpu.topKWindowPairs")) conf.getLong("cpslab.allpair.gpu.topKWindowPairs") else 0L
  // cpslab.allpair.gpu.topKTileCut = true (default false: off; one GPU only): with topK > 0 and similarityThreshold <= 0 the
  // probe kernel cuts every (query row, tile) round to the pairs that can be among a query's topK before it writes them
  // (apss_set_top_k_tile_cut) -- the same reply
  private val topKTileCut =
    if (conf.hasPath("cpslab.allpair.gpu.topKTileCut") && conf.getBoolean("cpslab.allpair.gpu.topKTileCut")) 1 else 0
  private val handle =
    if (grouped && rowRanges > 1)
      NativeApss.createGroupGrid(vectorDim, similarityThreshold, indexThreshold, flags, devices, headTerms, groupFlags, rowRanges, topK)
    else if (grouped) NativeApss.createGroup(vectorDim, similarityThreshold, indexThreshold, flags, devices, headTerms, groupFlags, topK)
    else NativeApss.create(vectorDim, similarityThreshold, indexThreshold, flags, devices(0), topKTileCut, headTerms, topKWindowPairs, topK)
  require(handle != 0L, if (grouped) NativeApss.groupLastError(0L) else NativeApss.lastError(0L))
  // cpslab.allpair.gpu.topPairs = K (default 0: off; one GPU only): a reply holds the K best pairs of its whole batch, by (score
  // descending, query id, candidate id ascending) -- apss_set_top_pairs, behind topK's per-query cut when both are set.  A value
  // the library refuses fails the construction; with several GPUs the worker says so and runs with 0
  private val topPairs = if (conf.hasPath("cpslab.allpair.gpu.topPairs")) conf.getLong("cpslab.allpair.gpu.topPairs") else 0L
  if (grouped && topPairs != 0L)
    System.err.println("GpuIndexingWorkerActor: cpslab.allpair.gpu.topPairs needs one GPU (cpslab.allpair.gpu.devices with one entry); running with 0")
  if (!grouped && topPairs != 0L)
    require(NativeApss.setTopPairs(handle, topPairs) == 0, NativeApss.lastError(handle))
  // cpslab.allpair.gpu.components = true (default false: off; one GPU only): the near-duplicate groups of everything the worker
  // holds -- the connected components of the graph whose edges are the pairs of its replies -- are kept on the device
  // (apss_set_components) and read with NativeApss.components(handle).  With several GPUs the worker says so and runs without
  private val components =
    conf.hasPath("cpslab.allpair.gpu.components") && conf.getBoolean("cpslab.allpair.gpu.components")
  if (grouped && components)
    System.err.println("GpuIndexingWorkerActor: cpslab.allpair.gpu.components needs one GPU (cpslab.allpair.gpu.devices with one entry); running without")
  if (!grouped && components)
    require(NativeApss.setComponents(handle, true) == 0, NativeApss.lastError(handle))
  // cpslab.allpair.gpu.componentsRepairRows = N (default 0: off; one GPU only, with components): a withdrawal re-joins the live
  // vectors of the groups it touched, at most N of them, instead of forgetting every group, and a compaction keeps the groups
  // (apss_set_components_repair)
  private val componentsRepairRows =
    if (conf.hasPath("cpslab.allpair.gpu.componentsRepairRows")) conf.getLong("cpslab.allpair.gpu.componentsRepairRows") else 0L
  if (grouped && componentsRepairRows != 0L)
    System.err.println("GpuIndexingWorkerActor: cpslab.allpair.gpu.componentsRepairRows needs one GPU (cpslab.allpair.gpu.devices with one entry); running with 0")
  if (!grouped && componentsRepairRows != 0L)
    require(NativeApss.setComponentsRepair(handle, componentsRepairRows) == 0, NativeApss.lastError(handle))
  /** the near-duplicate groups: for every store slot (smallest slot of its component | -1 for a withdrawn vector, the name of the
    * vector in that slot); null when cpslab.allpair.gpu.components is off */
  def groups(): (Array[Int], Array[String]) =
    if (grouped || !components) null
    else Option(NativeApss.components(handle)).map { case (label, rep) => (label, rep.map(i => nameOf(i.toInt))) }.orNull
  // cpslab.allpair.gpu.autoCompact = f (default 0: off; one GPU only): vectors withdrawn with NativeApss.remove keep their slots
  // until more than the fraction f of the stored vectors is removed; the next IndexData then compacts the store first
  // (apss_set_auto_compact).  The reference has no removal: it stops indexing after expDuration instead (below)
  private val autoCompact =
    if (conf.hasPath("cpslab.allpair.gpu.autoCompact")) conf.getDouble("cpslab.allpair.gpu.autoCompact") else 0.0
  if (!grouped && autoCompact != 0.0)
    require(NativeApss.setAutoCompact(handle, autoCompact) == 0, NativeApss.lastError(handle))
  /** withdraw vectors by their String ids (unknown ids are ignored); returns the vectors newly removed */
  def removeVectors(names: Iterable[String]): Long =
    if (grouped) throw new UnsupportedOperationException("removal needs one GPU (cpslab.allpair.gpu.devices with one entry)")
    else NativeApss.remove(handle, names.flatMap(idOf.get).toArray)
  /** "what is similar to these vectors that you already hold?" (apss_query_stored): the stored vectors named here are queried
    * against the store as they are stored, nothing is inserted, and the SimilarityOutput is replied the way the IndexData handler
    * replies its own.  Unknown names are ignored; every known name gets an entry, possibly empty */
  def similarTo(names: Iterable[String]): Unit = {
    if (grouped) throw new UnsupportedOperationException("similarTo needs one GPU (cpslab.allpair.gpu.devices with one entry)")
    val ids = names.flatMap(idOf.get).toArray
    val n = NativeApss.queryStored(handle, ids)
    if (n < 0) throw new IllegalArgumentException(lastError)
    val q = new Array[Long](n.toInt); val c = new Array[Long](n.toInt); val s = new Array[Float](n.toInt)
    if (n > 0) fetch(n, q, c, s)
    val out = new mutable.HashMap[String, mutable.HashMap[String, Double]]
    ids.foreach(i => out.getOrElseUpdate(nameOf(i.toInt), new mutable.HashMap[String, Double]))
    for (i <- 0 until n.toInt) out(nameOf(q(i).toInt)) += nameOf(c(i).toInt) -> s(i).toDouble
    reply(out)
  }
  private def reply(out: mutable.HashMap[String, mutable.HashMap[String, Double]]): Unit =
    if (replyTo.isDefined) {
      if (outputWritingDuration <= 0) replyTo.get ! SimilarityOutput(out, System.currentTimeMillis())
      else for ((q, m) <- out; (c, s) <- m) writeBuffer.getOrElseUpdate(q, new mutable.HashMap[String, Double]) += c -> s
    }
  private def submit(mode: Int, rowptr: Array[Long], indices: Array[Int], values: Array[Double], ids: Array[Long]): Long =
    if (grouped) NativeApss.groupSubmit(handle, mode, rowptr, indices, values, ids)
    else NativeApss.submit(handle, mode, rowptr, indices, values, ids)
  private def fetch(n: Long, q: Array[Long], c: Array[Long], s: Array[Float]): Int =
    if (grouped) NativeApss.groupFetch(handle, n, q, c, s) else NativeApss.fetch(handle, n, q, c, s)
  private def lastError: String = if (grouped) NativeApss.groupLastError(handle) else NativeApss.lastError(handle)
  private val idOf = new mutable.HashMap[String, Long]
  private val nameOf = new mutable.ArrayBuffer[String]
  private var stopUpdateIndex = false
  var replyTo: Option[ActorSelection] = None
  var ioTask: Cancellable = null

  if (expDuration > 0) context.setReceiveTimeout(expDuration milliseconds)

  override def preStart(): Unit = {
    import context.dispatcher
    replyTo = Some(context.actorSelection(conf.getString("cpslab.allpair.outputActor")))
    if (outputWritingDuration > 0) {
      ioTask = context.system.scheduler.schedule(0 milliseconds, outputWritingDuration milliseconds, self, IOTicket)
    }
  }

  override def postStop(): Unit = if (grouped) NativeApss.destroyGroup(handle) else NativeApss.destroy(handle)

  private def runBatch(vectors: Set[cpslab.vector.SparseVectorWrapper]):
      mutable.HashMap[String, mutable.HashMap[String, Double]] = {
    // The whole vector is indexed and scored here, so it must arrive ONCE: with maxShardNum > 1 the reference sends the
    // same full vector in one DataPacket per shard, each naming that shard's dims in wrapper.indices
    // (WriteWorkerActor.scala:166-179), and it would be stored and queried once per packet.  Deploy with
    // cpslab.allpair.maxShardNum = 1 (and maxIndexEntryActorNum = 1): INTEGRATION.md.
    vectors.foreach(w => require(w.indices.size == w.sparseVector._2.indices.length,
      "GpuIndexingWorkerActor needs the whole vector in one DataPacket: set cpslab.allpair.maxShardNum = 1"))
    val batch = vectors.toArray.map(_.sparseVector)           // (String id, SparseVector)
    val rowptr = new Array[Long](batch.length + 1)
    val ids = new Array[Long](batch.length)
    for (i <- batch.indices) {
      require(batch(i)._2.size == vectorDim, s"vector1 size: ${batch(i)._2.size}, vector2 size: $vectorDim")
      rowptr(i + 1) = rowptr(i) + batch(i)._2.indices.length
      ids(i) = idOf.getOrElseUpdate(batch(i)._1, { nameOf += batch(i)._1; (nameOf.length - 1).toLong })
    }
    val indices = batch.flatMap(_._2.indices)
    val values = batch.flatMap(_._2.values)
    val n = submit(if (stopUpdateIndex) 1 else 2, rowptr, indices, values, ids)
    if (n < 0) throw new IllegalArgumentException(lastError)
    val q = new Array[Long](n.toInt); val c = new Array[Long](n.toInt); val s = new Array[Float](n.toInt)
    if (n > 0) fetch(n, q, c, s)
    val out = new mutable.HashMap[String, mutable.HashMap[String, Double]]
    batch.foreach(b => out.getOrElseUpdate(b._1, new mutable.HashMap[String, Double]))
    for (i <- 0 until n.toInt) out(nameOf(q(i).toInt)) += nameOf(c(i).toInt) -> s(i).toDouble
    out
  }

  def receive: Receive = {
    case IndexData(vectors) =>
      try {
        reply(runBatch(vectors))
      } catch {
        case e: Exception => e.printStackTrace()
      }
    case IOTicket =>
      if (writeBuffer.nonEmpty) {
        replyTo.get ! SimilarityOutput(writeBuffer.clone(), System.currentTimeMillis())
        writeBuffer.clear()
      }
    case ReceiveTimeout => stopUpdateIndex = true
    case t @ Test(_) => replyTo.get ! t
  }
}
