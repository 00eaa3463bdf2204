"""Python face of one device-resident index (one IndexingWorkerActor's state on one MI355X).

Mirrors the seam the C ABI replaces -- `case IndexData(vectors)` of
core/src/main/scala/cpslab/deploy/server/IndexingWorkerActor.scala:123-137 -- and nothing else.  All compute
is in libapss_hip.so; errors surface as ApssError carrying the library's message."""
import ctypes as C

import numpy as np

from . import _lib


class ApssError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("apss error %d: %s" % (code, msg))
        self.code = code


def _np(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a.size else C.c_void_p(0)


class ApssIndex:
    def __init__(self, dim, theta, device=0, tile_rows=0, term_range=None, flags=0, index_threshold=0.0,
                 capacity_rows=0, capacity_nnz=0, head_terms=0, top_k=0, top_k_window=0, top_k_tile_cut=False,
                 auto_compact=0.0, top_pairs=0, components=False, components_repair=0):
        L = _lib.lib()
        cfg = _lib.Config()
        cfg.struct_size = C.sizeof(_lib.Config)
        cfg.dim = int(dim)
        cfg.theta = float(theta)
        cfg.index_threshold = float(index_threshold)
        cfg.flags = int(flags)
        cfg.device_id = int(device)
        cfg.term_lo, cfg.term_hi = (0, 0) if term_range is None else (int(term_range[0]), int(term_range[1]))
        cfg.tile_rows = int(tile_rows)
        cfg.head_terms = int(head_terms)  # dense-head block: 0 auto, -1 never, 64 | 128 | 256 forced
        cfg.capacity_rows = int(capacity_rows)
        cfg.capacity_nnz = int(capacity_nnz)
        h = C.c_void_p()
        rc = L.apss_create(C.byref(cfg), C.byref(h))
        if rc != _lib.OK:
            raise ApssError(rc, (L.apss_last_error(None) or b"").decode())
        self._h = h
        self._L = L
        self.dim, self.theta = int(dim), float(theta)
        self._device = int(device)
        if top_k or top_k_window or top_k_tile_cut or auto_compact or top_pairs or components or components_repair:
            try:
                if auto_compact:
                    self.set_auto_compact(auto_compact)
                if top_k_window:
                    self.set_top_k_window(top_k_window)
                if top_k_tile_cut:
                    self.set_top_k_tile_cut(True)
                if top_k:
                    self.set_top_k(top_k)
                if top_pairs:
                    self.set_top_pairs(top_pairs)
                if components:
                    self.set_components(True)
                if components_repair:
                    self.set_components_repair(components_repair)
            except ApssError:
                self.close()
                raise

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None):
            self._L.apss_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chk(self, rc):
        if rc != _lib.OK:
            raise ApssError(rc, (self._L.apss_last_error(self._h) or b"").decode())

    # -- host-pointer path (numpy in / numpy out)
    def _csr(self, ids, rowptr, indices, values):
        ids, rowptr = _np(ids, np.int64), _np(rowptr, np.int64)
        indices, values = _np(indices, np.int32), _np(values, np.float64)
        if rowptr.size != ids.size + 1:
            raise ValueError("rowptr must have len(ids) + 1 entries")
        return ids, rowptr, indices, values

    def insert(self, ids, rowptr, indices, values):
        """buildInvertedIndex(batch), IWA:61-71"""
        ids, rowptr, indices, values = self._csr(ids, rowptr, indices, values)
        self._chk(self._L.apss_insert(self._h, ids.size, _ptr(rowptr), _ptr(indices), _ptr(values), _ptr(ids)))

    def query(self, ids, rowptr, indices, values):
        """querySimilarItems(batch) on the frozen index (IWA:74-111 with stopUpdateIndex)"""
        ids, rowptr, indices, values = self._csr(ids, rowptr, indices, values)
        n = C.c_int64(0)
        self._chk(self._L.apss_query(self._h, ids.size, _ptr(rowptr), _ptr(indices), _ptr(values), _ptr(ids), C.byref(n)))
        return self.fetch()

    def insert_and_query(self, ids, rowptr, indices, values):
        """the IndexData handler, IWA:123-137"""
        ids, rowptr, indices, values = self._csr(ids, rowptr, indices, values)
        n = C.c_int64(0)
        self._chk(self._L.apss_insert_and_query(self._h, ids.size, _ptr(rowptr), _ptr(indices), _ptr(values), _ptr(ids),
                                                C.byref(n)))
        return self.fetch()

    def self_join(self, fetch=True):
        n = C.c_int64(0)
        self._chk(self._L.apss_self_join(self._h, C.byref(n)))
        return self.fetch() if fetch else n.value

    def result_count(self):
        n = C.c_int64(0)
        self._chk(self._L.apss_result_count(self._h, C.byref(n)))
        return n.value

    def fetch(self):
        """(query ext ids, candidate ext ids, scores) of the last query-type call"""
        n = self.result_count()
        q, c, s = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.float32)
        if n:
            self._chk(self._L.apss_fetch_results(self._h, 0, n, _ptr(q), _ptr(c), _ptr(s)))
        return q, c, s

    def size(self):
        r, z = C.c_int64(0), C.c_int64(0)
        self._chk(self._L.apss_size(self._h, C.byref(r), C.byref(z)))
        return r.value, z.value

    def stats(self):
        st = _lib.Stats()
        st.struct_size = C.sizeof(_lib.Stats)
        self._chk(self._L.apss_stats_get(self._h, C.byref(st)))
        d = {k: getattr(st, k) for k, _ in _lib.Stats._fields_}
        d["probe_kernel"] = d["probe_kernel"].decode()
        return d

    def set_top_k(self, k):
        """per-query top-k for the query-type calls made from now on (0: off); the list then comes grouped by query row, in
        rank order (score descending, candidate id ascending, slot ascending)"""
        self._chk(self._L.apss_set_top_k(self._h, int(k)))

    def topk_info(self):
        """what the per-query top-k did in the last query-type call (apss_topk_info)"""
        ti = _lib.TopkInfo()
        ti.struct_size = C.sizeof(_lib.TopkInfo)
        self._chk(self._L.apss_topk_get(self._h, C.byref(ti)))
        return {k: getattr(ti, k) for k, _ in _lib.TopkInfo._fields_}

    def set_top_k_window(self, pairs):
        """with top-k on: join and cut the query-type calls made from now on in windows of consecutive query rows, so that the
        handle never holds more than about `pairs` uncut pairs (0: off).  Same list, element by element"""
        self._chk(self._L.apss_set_top_k_window(self._h, int(pairs)))

    def topk_window_info(self):
        """how the last query-type call was windowed (apss_topk_window_info; windows = 0: it was not)"""
        wi = _lib.TopkWindowInfo()
        wi.struct_size = C.sizeof(_lib.TopkWindowInfo)
        self._chk(self._L.apss_topk_window_get(self._h, C.byref(wi)))
        return {k: getattr(wi, k) for k, _ in _lib.TopkWindowInfo._fields_}

    def set_top_k_tile_cut(self, on):
        """with top-k on: a call that runs the theta <= 0 kernel cuts every (query row, tile) round to the pairs that can be
        among a row's k best before it writes them (False: off).  Same list, element by element"""
        self._chk(self._L.apss_set_top_k_tile_cut(self._h, 1 if on else 0))

    def topk_tile_cut_info(self):
        """what the cut inside the probe did in the last query-type call (apss_topk_tile_cut_info)"""
        ci = _lib.TopkTileCutInfo()
        ci.struct_size = C.sizeof(_lib.TopkTileCutInfo)
        self._chk(self._L.apss_topk_tile_cut_get(self._h, C.byref(ci)))
        return {k: getattr(ci, k) for k, _ in _lib.TopkTileCutInfo._fields_}

    def topk_window_cuts(self):
        """the last call's windows as windows + 1 ascending row offsets of its batch (empty: it was not windowed)"""
        n = C.c_int64(0)
        self._chk(self._L.apss_topk_window_cuts(self._h, 0, None, C.byref(n)))
        cuts = np.zeros(n.value, dtype=np.int64)
        if n.value:
            self._chk(self._L.apss_topk_window_cuts(self._h, n.value, _ptr(cuts), C.byref(n)))
        return cuts

    def remove(self, ids):
        """mark every stored row whose external id is in `ids` (numpy / a sequence, or an int64 torch tensor on this handle's
        GPU) as removed: query-type calls made from now on answer as if those rows were not stored.  Returns the rows newly
        marked (ids that are not stored, already removed or repeated count for nothing)"""
        n = C.c_int64(0)
        if hasattr(ids, "data_ptr"):
            import torch
            assert ids.dtype == torch.int64 and ids.is_cuda and ids.is_contiguous()
            ptr = C.c_void_p(ids.data_ptr()) if ids.numel() else C.c_void_p(0)
            self._chk(self._L.apss_remove_dev(self._h, ids.numel(), ptr, C.byref(n)))
        else:
            ids = _np(ids, np.int64)
            self._chk(self._L.apss_remove(self._h, ids.size, _ptr(ids), C.byref(n)))
        return n.value

    def compact(self):
        """the store becomes its live rows in stored order and the index is rebuilt, on the device (apss_compact); the last
        call's results are gone afterwards.  Nothing marked: a no-op"""
        self._chk(self._L.apss_compact(self._h))

    def set_auto_compact(self, fraction):
        """compact at the start of an insert-type call once more than `fraction` of the stored rows is marked (0: off)"""
        self._chk(self._L.apss_set_auto_compact(self._h, float(fraction)))

    def removal_info(self):
        """marks, compactions and what the last query-type call dropped (apss_removal_info)"""
        ri = _lib.RemovalInfo()
        ri.struct_size = C.sizeof(_lib.RemovalInfo)
        self._chk(self._L.apss_removal_get(self._h, C.byref(ri)))
        return {k: getattr(ri, k) for k, _ in _lib.RemovalInfo._fields_}

    def query_stored(self, ids, fetch=True):
        """what is similar to the vectors already stored under `ids` (numpy / a sequence, or an int64 torch tensor on this
        handle's GPU): every live stored row with one of these ids becomes a row of the query batch, in stored order, gathered on
        the device exactly as it is stored (no second normalisation, prune or admission).  Ids that are not stored, removed or
        repeated select nothing more.  Returns the pairs (fetch=True) or (rows of the batch, pairs)"""
        rows, n = C.c_int64(0), C.c_int64(0)
        if hasattr(ids, "data_ptr"):
            import torch
            assert ids.dtype == torch.int64 and ids.is_cuda and ids.is_contiguous()
            ptr = C.c_void_p(ids.data_ptr()) if ids.numel() else C.c_void_p(0)
            self._chk(self._L.apss_query_stored_dev(self._h, ids.numel(), ptr, C.byref(rows), C.byref(n)))
        else:
            ids = _np(ids, np.int64)
            self._chk(self._L.apss_query_stored(self._h, ids.size, _ptr(ids), C.byref(rows), C.byref(n)))
        return self.fetch() if fetch else (rows.value, n.value)

    def stored_query_info(self):
        """what the last query_stored selected and gathered (apss_stored_query_info)"""
        qi = _lib.StoredQueryInfo()
        qi.struct_size = C.sizeof(_lib.StoredQueryInfo)
        self._chk(self._L.apss_stored_query_get(self._h, C.byref(qi)))
        return {k: getattr(qi, k) for k, _ in _lib.StoredQueryInfo._fields_}

    def set_top_pairs(self, K):
        """global top-K for the query-type calls made from now on (0: off): a call's final list becomes its K best pairs in rank
        order (score descending, then query id, candidate id, query row, slot ascending), selected on the device"""
        self._chk(self._L.apss_set_top_pairs(self._h, int(K)))

    def top_pairs_info(self):
        """what the global top-K did in the last query-type call (apss_top_pairs_info)"""
        ti = _lib.TopPairsInfo()
        ti.struct_size = C.sizeof(_lib.TopPairsInfo)
        self._chk(self._L.apss_top_pairs_get(self._h, C.byref(ti)))
        return {k: getattr(ti, k) for k, _ in _lib.TopPairsInfo._fields_}

    def set_components(self, on):
        """near-duplicate groups (apss_set_components): on = the connected components of the graph "stored row - stored row, edge =
        a pair of a call's final list" are kept on the device across calls; off (the default) frees them"""
        self._chk(self._L.apss_set_components(self._h, 1 if on else 0))

    def set_components_repair(self, max_rows):
        """keep the groups across remove and compact (apss_set_components_repair): a remove re-joins the live rows of the components
        it touched, at most `max_rows` of them (more: today's reset to singletons), and a compaction renumbers the forest; 0 (the
        default): off"""
        self._chk(self._L.apss_set_components_repair(self._h, int(max_rows)))

    def components_repair_info(self):
        """the setting, what the last remove's repair did and the totals since create (apss_components_repair_info)"""
        ri = _lib.ComponentsRepairInfo()
        ri.struct_size = C.sizeof(_lib.ComponentsRepairInfo)
        self._chk(self._L.apss_components_repair_get(self._h, C.byref(ri)))
        return {k: getattr(ri, k) for k, _ in _lib.ComponentsRepairInfo._fields_}

    def components_info(self):
        """the structure's state and what the last calls did to it (apss_components_info); brings the labels up to date"""
        ci = _lib.ComponentsInfo()
        ci.struct_size = C.sizeof(_lib.ComponentsInfo)
        self._chk(self._L.apss_components_get(self._h, C.byref(ci)))
        return {k: getattr(ci, k) for k, _ in _lib.ComponentsInfo._fields_}

    def components(self, offset=0, count=None):
        """(labels int32, rep_ext int64) of the slots [offset, offset + count) (default: all): the smallest slot of every slot's
        component and that slot's external id; a removed row: -1 and its own id (apss_components_fetch)"""
        if count is None:
            count = self.size()[0] - offset
        labels, rep = np.zeros(max(count, 0), np.int32), np.zeros(max(count, 0), np.int64)
        self._chk(self._L.apss_components_fetch(self._h, int(offset), int(count), _ptr(labels), _ptr(rep)))
        return labels, rep

    def components_dev(self):
        """the labels where they live: an int32 torch tensor over the device array, no copy (apss_components_dev; valid until the
        next insert, query-type call, remove, compact, clear or set_components)"""
        import torch
        p, rows = C.c_void_p(), C.c_int64(0)
        self._chk(self._L.apss_components_dev(self._h, C.byref(p), C.byref(rows)))
        if not rows.value:
            return torch.empty(0, dtype=torch.int32, device="cuda:%d" % self._device)

        class _View:  # (torch reads the array interface: the tensor aliases the handle's memory)
            __cuda_array_interface__ = {"shape": (rows.value,), "typestr": "<i4", "data": (p.value, False), "version": 2, "strides": None}
        return torch.as_tensor(_View(), device="cuda:%d" % self._device)

    def set_head_terms(self, terms, part=0, n_parts=1, fold_columns=0):
        """dense-head block named by the caller (every term shard of a join gets the same terms; shard `part` of `n_parts`
        multiplies its share of the candidate tiles); fold_columns: how many of a wide head's 256 columns are folded ones
        (64 | 128 | 192; 0: the default, 128); empty handle only"""
        t = _np(terms, np.int32)
        self._chk(self._L.apss_set_head_fold(self._h, int(fold_columns)))
        self._chk(self._L.apss_set_head_terms(self._h, t.size, _ptr(t), int(part), int(n_parts)))

    def head_terms(self):
        n = C.c_int32(0)
        out = np.zeros(32768, np.int32)
        self._chk(self._L.apss_get_head_terms(self._h, out.size, _ptr(out), C.byref(n)))
        return out[:n.value].copy()

    def clear(self):
        self._chk(self._L.apss_clear(self._h))

    # -- device-pointer path (torch tensors on this handle's GPU; torch is plumbing only)
    def set_stream(self, cuda_stream_handle):
        """run on this HIP stream (0 = the default stream, where torch works unless told otherwise)"""
        self._chk(self._L.apss_set_stream(self._h, C.c_void_p(cuda_stream_handle), 0))

    def use_own_stream(self):
        self._chk(self._L.apss_set_stream(self._h, C.c_void_p(0), 1))

    @staticmethod
    def _dev(rowptr, indices, values, ids):
        import torch
        assert rowptr.dtype == torch.int64 and indices.dtype == torch.int32
        assert values.dtype == torch.float32 and ids.dtype == torch.int64
        for t in (rowptr, indices, values, ids):
            assert t.is_cuda and t.is_contiguous()
        return (ids.numel(), indices.numel(), C.c_void_p(rowptr.data_ptr()), C.c_void_p(indices.data_ptr()),
                C.c_void_p(values.data_ptr()), C.c_void_p(ids.data_ptr()))

    def insert_dev(self, ids, rowptr, indices, values):
        n, nnz, rp, ix, vl, ex = self._dev(rowptr, indices, values, ids)
        self._chk(self._L.apss_insert_dev(self._h, n, nnz, rp, ix, vl, ex))

    def query_dev(self, ids, rowptr, indices, values):
        n, nnz, rp, ix, vl, ex = self._dev(rowptr, indices, values, ids)
        out = C.c_int64(0)
        self._chk(self._L.apss_query_dev(self._h, n, nnz, rp, ix, vl, ex, C.byref(out)))
        return out.value

    def insert_and_query_dev(self, ids, rowptr, indices, values):
        n, nnz, rp, ix, vl, ex = self._dev(rowptr, indices, values, ids)
        out = C.c_int64(0)
        self._chk(self._L.apss_insert_and_query_dev(self._h, n, nnz, rp, ix, vl, ex, C.byref(out)))
        return out.value

    def results_dev(self):
        """raw device pointers (q_row int32*, c_slot int32*, score float*, n) of the last results"""
        a, b, c, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64(0)
        self._chk(self._L.apss_results_dev(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        return a.value, b.value, c.value, n.value

    def results_to(self, q_row=None, c_slot=None, score=None, offset=0):
        """copy the last results into torch device tensors (int32, int32, float32) without leaving the GPU"""
        n = max(t.numel() for t in (q_row, c_slot, score) if t is not None)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else C.c_void_p(0)  # noqa: E731
        self._chk(self._L.apss_results_copy_dev(self._h, offset, n, ptr(q_row), ptr(c_slot), ptr(score)))

    def partial_scores_dev(self, q_row, c_slot, out):
        import torch
        assert q_row.dtype == torch.int32 and c_slot.dtype == torch.int32 and out.dtype == torch.float32
        self._chk(self._L.apss_partial_scores_dev(self._h, q_row.numel(), C.c_void_p(q_row.data_ptr()),
                                                  C.c_void_p(c_slot.data_ptr()), C.c_void_p(out.data_ptr())))


class ApssGroup:
    """Python face of apss_group (include/apss.h): the term-sharded index of one node -- `devices[i]` holds member i's
    term range -- behind one object; the members' exchange (all-gather of candidate lists, all-reduce of partial scores)
    runs below the C ABI (RCCL when every member has its own GPU, device-to-device copies when members share one).
    Mirrors WriteWorkerActor.scala:164-183 + EntryProxyActor.scala:37-49 + IndexingWorkerActor.scala:122-137.
    row_ranges = D > 1: a T x D grid (apss_group_create_grid), T = len(devices) / D term ranges x D row ranges, member
    (j, i) = row range j, term range i on devices[j * T + i]; every call answers as one plain handle would."""

    def __init__(self, dim, theta, devices, flags=0, index_threshold=0.0, tile_rows=0, head_terms=0, group_flags=0,
                 term_cuts=None, capacity_rows=0, capacity_nnz=0, row_ranges=1, top_k=0):
        L = _lib.lib()
        cfg = _lib.Config()
        cfg.struct_size = C.sizeof(_lib.Config)
        cfg.dim, cfg.theta, cfg.index_threshold = int(dim), float(theta), float(index_threshold)
        cfg.flags, cfg.tile_rows, cfg.head_terms = int(flags), int(tile_rows), int(head_terms)
        cfg.capacity_rows, cfg.capacity_nnz = int(capacity_rows), int(capacity_nnz)
        devs = _np(devices, np.int32)
        g = C.c_void_p()
        row_ranges = int(row_ranges)
        if row_ranges >= 1 and devs.size % row_ranges:
            raise ValueError("len(devices) must be term ranges x row_ranges")
        # (row_ranges = 1 goes through apss_group_create_grid too: the two entry points are one)
        rc = L.apss_group_create_grid(C.byref(cfg), devs.size // row_ranges if row_ranges >= 1 else 0, row_ranges, _ptr(devs),
                                      int(group_flags), C.byref(g))
        if rc != _lib.OK:
            raise ApssError(rc, (L.apss_group_last_error(None) or b"").decode())
        self._g, self._L = g, L
        self.dim, self.theta, self.n_members = int(dim), float(theta), int(devs.size)
        self.row_ranges, self.term_ranges = row_ranges, int(devs.size) // row_ranges
        if term_cuts is not None:
            cuts = _np(term_cuts, np.int32)
            if cuts.size != self.term_ranges + 1:
                raise ValueError("term_cuts must have one entry more than there are term ranges")
            self._chk(L.apss_group_set_term_cuts(self._g, _ptr(cuts)))
        if top_k:
            try:
                self.set_top_k(top_k)
            except ApssError:
                self.close()
                raise

    def close(self):
        if getattr(self, "_g", None):
            self._L.apss_group_destroy(self._g)
            self._g = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _chk(self, rc):
        if rc != _lib.OK:
            raise ApssError(rc, (self._L.apss_group_last_error(self._g) or b"").decode())

    _csr = ApssIndex._csr

    def insert(self, ids, rowptr, indices, values):
        ids, rowptr, indices, values = self._csr(ids, rowptr, indices, values)
        self._chk(self._L.apss_group_insert(self._g, ids.size, _ptr(rowptr), _ptr(indices), _ptr(values), _ptr(ids)))

    def query(self, ids, rowptr, indices, values):
        ids, rowptr, indices, values = self._csr(ids, rowptr, indices, values)
        n = C.c_int64(0)
        self._chk(self._L.apss_group_query(self._g, ids.size, _ptr(rowptr), _ptr(indices), _ptr(values), _ptr(ids), C.byref(n)))
        return self.fetch()

    def insert_and_query(self, ids, rowptr, indices, values, fetch=True):
        """the IndexData handler on every member + the exchange, IWA:123-137"""
        ids, rowptr, indices, values = self._csr(ids, rowptr, indices, values)
        n = C.c_int64(0)
        self._chk(self._L.apss_group_insert_and_query(self._g, ids.size, _ptr(rowptr), _ptr(indices), _ptr(values), _ptr(ids),
                                                      C.byref(n)))
        return self.fetch() if fetch else n.value

    def insert_and_query_dev(self, per_member):
        """per_member: for every member (ids int64, rowptr int64, indices int32, values fp32) torch tensors on ITS device"""
        n = nnz = None
        tabs = [(C.c_void_p * self.n_members)() for _ in range(4)]
        for i, (ids, rowptr, indices, values) in enumerate(per_member):
            m, z, rp, ix, vl, ex = ApssIndex._dev(rowptr, indices, values, ids)
            assert n in (None, m) and nnz in (None, z), "every member is handed the same batch"
            n, nnz = m, z
            tabs[0][i], tabs[1][i], tabs[2][i], tabs[3][i] = rp, ix, vl, ex
        out = C.c_int64(0)
        self._chk(self._L.apss_group_insert_and_query_dev(self._g, n, nnz, tabs[0], tabs[1], tabs[2], tabs[3], C.byref(out)))
        return out.value

    def result_count(self):
        n = C.c_int64(0)
        self._chk(self._L.apss_group_result_count(self._g, C.byref(n)))
        return n.value

    def fetch(self):
        n = self.result_count()
        q, c, s = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.float32)
        if n:
            self._chk(self._L.apss_group_fetch_results(self._g, 0, n, _ptr(q), _ptr(c), _ptr(s)))
        return q, c, s

    def clear(self):
        self._chk(self._L.apss_group_clear(self._g))

    def stats(self):
        st = _lib.GroupStats()
        st.struct_size = C.sizeof(_lib.GroupStats)
        self._chk(self._L.apss_group_stats_get(self._g, C.byref(st)))
        d = {k: getattr(st, k) for k, _ in _lib.GroupStats._fields_}
        d["term_cuts"] = list(st.term_cuts[: self.term_ranges + 1])
        return d

    def set_top_k(self, k):
        """per-query top-k of the group's answers (apss_group_set_top_k; not on a grid with more than one row range)"""
        self._chk(self._L.apss_group_set_top_k(self._g, int(k)))

    def topk_info(self):
        ti = _lib.TopkInfo()
        ti.struct_size = C.sizeof(_lib.TopkInfo)
        self._chk(self._L.apss_group_topk_get(self._g, C.byref(ti)))
        return {k: getattr(ti, k) for k, _ in _lib.TopkInfo._fields_}

    def grid(self):
        """the grid's shape and what its row ranges did in the last call (apss_group_grid_get)"""
        gr = _lib.GroupGrid()
        gr.struct_size = C.sizeof(_lib.GroupGrid)
        self._chk(self._L.apss_group_grid_get(self._g, C.byref(gr)))
        d = {k: getattr(gr, k) for k, _ in _lib.GroupGrid._fields_}
        d["rows_in_range"] = list(gr.rows_in_range[: self.row_ranges])
        return d

    def relayout(self, cuts=None):
        """re-decide the layout from the stored rows now (apss_group_relayout): cuts=None decides cuts and dense head, explicit
        cuts (n_members + 1 entries) re-decide only the head; the store is rebuilt when the layout changes"""
        if cuts is None:
            self._chk(self._L.apss_group_relayout(self._g, None))
            return
        cuts = _np(cuts, np.int32)
        if cuts.size != self.term_ranges + 1:
            raise ValueError("cuts must have one entry more than there are term ranges")
        self._chk(self._L.apss_group_relayout(self._g, _ptr(cuts)))

    def layout(self):
        """the layout and its re-layout history (apss_group_layout_get; dfsq is computed on the device at this call)"""
        lo = _lib.GroupLayout()
        lo.struct_size = C.sizeof(_lib.GroupLayout)
        self._chk(self._L.apss_group_layout_get(self._g, C.byref(lo)))
        d = {k: getattr(lo, k) for k, _ in _lib.GroupLayout._fields_}
        d["term_cuts"] = list(lo.term_cuts[: self.term_ranges + 1])
        d["dfsq"] = list(lo.dfsq[: self.n_members])
        return d

    def member_stats(self, member):
        st = _lib.Stats()
        st.struct_size = C.sizeof(_lib.Stats)
        self._chk(self._L.apss_group_member_stats(self._g, int(member), C.byref(st)))
        d = {k: getattr(st, k) for k, _ in _lib.Stats._fields_}
        d["probe_kernel"] = d["probe_kernel"].decode()
        return d
