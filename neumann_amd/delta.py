"""Delta vectors (tensor_store/src/delta_vector.rs:72-643) behind libneumann_gpu.so: `ArchetypeRegistry` (nmn_archetypes) and
`DeltaSet` (nmn_delta_set, N delta rows held together), bit for bit on the device and on the library's host path (docs/delta.md).

    reg = ArchetypeRegistry(dim=128, max_archetypes=64)
    reg.discover_archetypes(rows, 16)
    deltas = reg.encode_batch(rows, threshold=1e-3)
    scores = deltas.dot_dense(queries)              # [nq][n]
"""
import ctypes as C

import numpy as np

from . import _capi

MAX_DIMENSION = 65535
DELTA_VECTOR_BYTES = 72       # size_of::<DeltaVector>() on a 64-bit target (docs/delta.md §1)
ALWAYS_DEVICE, NEVER_DEVICE = 0, 2 ** 64 - 1


class DeltaVectorError(_capi.NeumannGpuError):
    """DeltaVectorError (delta_vector.rs:42-61) and the refusals of from_parts; the text is the reference's Display where it has one"""

    def __init__(self, text, status=_capi.ERR_INVALID_ARGUMENT):
        RuntimeError.__init__(self, text)
        self.status = status


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def _check(status):
    if status == _capi.ERR_INVALID_ARGUMENT:
        raise DeltaVectorError(_capi.load().nmn_last_error().decode(errors="replace"))
    _capi.check(status)


def _rows(rows, dim, what="rows"):
    r = np.ascontiguousarray(rows, dtype=np.float32)
    if r.ndim == 1 and (r.size == dim or dim == 0):
        r = r[None, :]
    if r.size == 0:
        r = r.reshape(0, dim)
    if r.ndim != 2 or r.shape[1] != dim:
        raise DeltaVectorError(f"{what} must be [n][{dim}], got {tuple(r.shape)}", _capi.ERR_DIMENSION_MISMATCH)
    return r


def _stream(stream):
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream if stream is None else stream)


def default_options():
    """nmn_delta_options_default -> min_device_rows"""
    o = _capi.DeltaOptions()
    _capi.load().nmn_delta_options_default(C.byref(o))
    return int(o.min_device_rows)


def limits():
    """(max_dimension, lds_query_dim, archetype_tile, scan_block) of the device path (nmn_delta_limits)"""
    v = [C.c_uint32() for _ in range(4)]
    _capi.check(_capi.load().nmn_delta_limits(*[C.byref(x) for x in v]))
    return tuple(int(x.value) for x in v)


def search_limits():
    """(select_chunk_rows, select_max_k, block_budget_bytes, sort_single_query_rows) of DeltaSet.search on the device
    (nmn_deltaset_limits): the rows a step of the select workgroup reads, the largest k it serves (above: the sort of the large-k
    path), the bytes of score words a block of queries of the host-buffer form may fill, and the rows from which a call of one
    query takes the sort as well"""
    a, b, c, d = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
    _capi.check(_capi.load().nmn_deltaset_limits(C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
    return int(a.value), int(b.value), int(c.value), int(d.value)


def _metric(metric):
    if metric not in ("dot", "cosine"):
        raise DeltaVectorError(f"metric must be \"dot\" or \"cosine\", got {metric!r}")
    return int(metric == "cosine")


class CoverageStats:
    """CoverageStats (delta_vector.rs:677-687)"""

    def __init__(self, avg_similarity=0.0, avg_compression_ratio=0.0, avg_delta_nnz=0.0, archetype_usage=()):
        self.avg_similarity = np.float32(avg_similarity)
        self.avg_compression_ratio = np.float32(avg_compression_ratio)
        self.avg_delta_nnz = np.float32(avg_delta_nnz)
        self.archetype_usage = [int(x) for x in archetype_usage]

    def __repr__(self):
        return (f"CoverageStats(avg_similarity={self.avg_similarity}, avg_compression_ratio={self.avg_compression_ratio}, "
                f"avg_delta_nnz={self.avg_delta_nnz}, archetype_usage={self.archetype_usage})")


class ArchetypeRegistry:
    """ArchetypeRegistry (delta_vector.rs:421-643) for rows of `dim` floats.  min_device_rows: calls of fewer rows run on the
    library's host path (same bits); None keeps the library's default."""

    def __init__(self, dim, max_archetypes, device=-1, min_device_rows=None):
        self._lib = _capi.load()
        self._h = C.c_void_p()
        _check(self._lib.nmn_archetypes_create(int(dim), int(max_archetypes), int(device), C.byref(self._h)))
        self.dim = int(dim)
        self.max_archetypes = int(max_archetypes)
        if min_device_rows is not None:
            self.set_min_device_rows(min_device_rows)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.nmn_archetypes_destroy(h)

    def set_min_device_rows(self, rows):
        o = _capi.DeltaOptions(min_device_rows=int(rows))
        _check(self._lib.nmn_archetypes_set_options(self._h, C.byref(o)))

    def __len__(self):
        return int(self._lib.nmn_archetypes_len(self._h))

    def is_empty(self):
        return len(self) == 0

    def register(self, archetype):
        """register (442-452) -> the id, None at max_archetypes"""
        return self.register_batch(_rows(archetype, self.dim, "an archetype"))[0]

    def register_batch(self, rows):
        r = _rows(rows, self.dim)
        ids = np.empty(r.shape[0], dtype=np.int64)
        _check(self._lib.nmn_archetypes_register(self._h, _p(r), r.shape[0], _p(ids)))
        return [None if i < 0 else int(i) for i in ids]

    def discover_archetypes(self, vectors, k, max_iterations=100, convergence_threshold=1e-4, seed=42, init_method="kmeans++"):
        """discover_archetypes (566-592) with KMeansConfig's fields -> how many were added"""
        r = _rows(vectors, self.dim, "vectors")
        opt = _capi.KMeansOptions(max_iterations=int(max_iterations), convergence_threshold=float(convergence_threshold),
                                  seed=int(seed), init_method=0 if init_method == "random" else 1)
        added = C.c_uint64()
        _check(self._lib.nmn_archetypes_discover(self._h, _p(r), r.shape[0], int(k), C.byref(opt), C.byref(added)))
        return int(added.value)

    def get(self, archetype_id):
        out = np.empty(self.dim, dtype=np.float32)
        st = self._lib.nmn_archetypes_get(self._h, int(archetype_id), _p(out)) if archetype_id >= 0 else _capi.ERR_NOT_FOUND
        if st == _capi.ERR_NOT_FOUND:
            return None
        _check(st)
        return out

    def magnitude_sq(self, archetype_id):
        out = C.c_float()
        st = self._lib.nmn_archetypes_magnitude_sq(self._h, int(archetype_id), C.byref(out)) if archetype_id >= 0 else _capi.ERR_NOT_FOUND
        if st == _capi.ERR_NOT_FOUND:
            return None
        _check(st)
        return np.float32(out.value)

    def find_best_batch(self, vectors):
        """find_best_archetype (480-513) of every row -> (ids int64 [n], sims f32 [n]); ids are -1 on an empty registry"""
        r = _rows(vectors, self.dim, "vectors")
        ids = np.full(r.shape[0], -1, dtype=np.int64)
        sims = np.zeros(r.shape[0], dtype=np.float32)
        _check(self._lib.nmn_archetypes_find_best(self._h, _p(r), r.shape[0], _p(ids), _p(sims)))
        return ids, sims

    def find_best_archetype(self, vector):
        """-> (id, similarity) or None"""
        ids, sims = self.find_best_batch(_rows(vector, self.dim, "a vector")[:1])
        return None if ids[0] < 0 else (int(ids[0]), np.float32(sims[0]))

    def encode_batch(self, vectors, threshold, with_magnitude=False):
        """encode_batch (598-607) -> DeltaSet (its compression ratios: DeltaSet.compression_ratio()); empty on an empty registry"""
        r = _rows(vectors, self.dim, "vectors")
        h = C.c_void_p()
        _check(self._lib.nmn_archetypes_encode_batch(self._h, _p(r), r.shape[0], C.c_float(threshold), int(bool(with_magnitude)), C.byref(h)))
        return DeltaSet(self, h)

    def encode(self, vector, threshold, with_magnitude=False):
        """encode (517-526) -> a DeltaSet of one row, None on an empty registry"""
        s = self.encode_batch(_rows(vector, self.dim, "a vector")[:1], threshold, with_magnitude)
        return s if len(s) else None

    def decode(self, deltas):
        """decode (530-533) of every row -> f32 [n][dim]"""
        return deltas.to_dense()

    def dot_delta_dense(self, deltas, query):
        """dot_delta_dense (537-540) of every row with one query -> f32 [n]"""
        return deltas.dot_dense(query)[0]

    def dot_deltas_same_archetype(self, a, b, pairs=None):
        """dot_deltas_same_archetype (544-552) -> (f32 [n_pairs], ok bool [n_pairs]); ok is False where the reference returns None.
        pairs: [n_pairs][2] rows of a and b; None pairs row i with row i."""
        if a.registry is not self or b.registry is not self:
            raise DeltaVectorError("the delta sets belong to another registry")
        if pairs is None:
            m = min(len(a), len(b))
            pairs = np.stack([np.arange(m), np.arange(m)], axis=1)
        pr = np.ascontiguousarray(pairs, dtype=np.uint64).reshape(-1, 2)
        out = np.zeros(pr.shape[0], dtype=np.float32)
        ok = np.zeros(pr.shape[0], dtype=np.uint8)
        _check(self._lib.nmn_delta_set_dot_same_archetype(a._h, b._h, _p(pr), pr.shape[0], _p(out), _p(ok)))
        return out, ok.astype(bool)

    def analyze_coverage(self, vectors, threshold):
        """analyze_coverage (614-643) -> CoverageStats"""
        r = _rows(vectors, self.dim, "vectors")
        st = _capi.CoverageStats()
        usage = np.zeros(max(len(self), 1), dtype=np.uint64)
        _check(self._lib.nmn_archetypes_analyze_coverage(self._h, _p(r), r.shape[0], C.c_float(threshold), C.byref(st), _p(usage)))
        if r.shape[0] == 0 or len(self) == 0:
            return CoverageStats()
        return CoverageStats(st.avg_similarity, st.avg_compression_ratio, st.avg_delta_nnz, usage[:len(self)])

    # -- stream-ordered forms on torch tensors ---------------------------------------------------------------------------------
    def to_device(self):
        """make the registry resident (blocks); needed again after a register"""
        _check(self._lib.nmn_archetypes_to_device(self._h))
        return self

    def find_best_device(self, vectors, stream=None):
        """nmn_archetypes_find_best_device on an f32 tensor [n][dim] of the registry's device: enqueued, not waited for ->
        (ids int64 tensor [n], sims f32 tensor [n])"""
        import torch
        assert vectors.dtype == torch.float32 and vectors.is_contiguous() and vectors.shape[-1] == self.dim
        n = vectors.numel() // self.dim
        ids = torch.empty(n, dtype=torch.int64, device=vectors.device)
        sims = torch.empty(n, dtype=torch.float32, device=vectors.device)
        _check(self._lib.nmn_archetypes_find_best_device(self._h, C.c_void_p(vectors.data_ptr()), n, C.c_void_p(ids.data_ptr()),
                                                         C.c_void_p(sims.data_ptr()), _stream(stream)))
        return ids, sims

    def encode_batch_device(self, vectors, threshold, with_magnitude=False, stream=None, return_assignments=False):
        """nmn_deltaset_encode_device on an f32 tensor [n][dim] of the registry's device (the registry resident: to_device) -> a
        resident DeltaSet without host arrays; with return_assignments (DeltaSet, ids int64 tensor [n], sims f32 tensor [n]).  The
        call waits once on the stream, for the two totals that size the set, and returns with the rest enqueued.  The rows must stay
        as they are until the stream has run the call"""
        import torch
        assert vectors.dtype == torch.float32 and vectors.is_contiguous() and vectors.shape[-1] == self.dim
        n = vectors.numel() // self.dim
        ids = torch.empty(n, dtype=torch.int64, device=vectors.device) if return_assignments else None
        sims = torch.empty(n, dtype=torch.float32, device=vectors.device) if return_assignments else None
        h = C.c_void_p()
        _check(self._lib.nmn_deltaset_encode_device(self._h, C.c_void_p(vectors.data_ptr()), n, C.c_float(threshold), int(bool(with_magnitude)),
                                                    None if ids is None else C.c_void_p(ids.data_ptr()),
                                                    None if sims is None else C.c_void_p(sims.data_ptr()), _stream(stream), C.byref(h)))
        s = DeltaSet(self, h)
        return (s, ids, sims) if return_assignments else s


class DeltaSet:
    """N DeltaVectors (delta_vector.rs:72-417) against one registry: archetype id per row, CSR offsets, u16 positions, f32 deltas
    and the optional cached magnitudes.  Immutable."""

    def __init__(self, registry, handle):
        self.registry = registry
        self._lib = registry._lib
        self._h = handle

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.nmn_delta_set_destroy(h)

    @classmethod
    def from_parts(cls, registry, archetype_ids, indptr, positions, deltas, cached_magnitudes=None, has_cached=None):
        """from_parts (170-205) for every row; unsorted and repeated positions are kept.  Refuses an unregistered archetype id, an
        indptr that does not ascend and a position that is not below the dimension."""
        ids = np.ascontiguousarray(archetype_ids, dtype=np.uint64).ravel()
        ptr = np.ascontiguousarray(indptr, dtype=np.uint64).ravel()
        if ptr.size != ids.size + 1:
            raise DeltaVectorError(f"indptr must hold {ids.size + 1} offsets, got {ptr.size}")
        if np.asarray(positions).size and (np.asarray(positions).min() < 0 or np.asarray(positions).max() > 65535):
            bad = int(np.asarray(positions).max())
            raise DeltaVectorError(f"delta set: position {bad} is not below the dimension {registry.dim}")
        pos = np.ascontiguousarray(positions, dtype=np.uint16).ravel()
        dl = np.ascontiguousarray(deltas, dtype=np.float32).ravel()
        if pos.size != dl.size or (ptr.size and int(ptr.max()) > pos.size):
            raise DeltaVectorError(f"positions ({pos.size}) and deltas ({dl.size}) must both hold indptr's {int(ptr.max())} entries")
        cm = None if cached_magnitudes is None else np.ascontiguousarray(cached_magnitudes, dtype=np.float32).ravel()
        hc = None if has_cached is None else np.ascontiguousarray(has_cached, dtype=np.uint8).ravel()
        if (cm is not None and cm.size != ids.size) or (hc is not None and hc.size != ids.size):
            raise DeltaVectorError("cached_magnitudes and has_cached hold one value per row")
        h = C.c_void_p()
        _check(registry._lib.nmn_delta_set_from_parts(registry._h, ids.size, _p(ids), _p(ptr), _p(pos), _p(dl), _p(cm), _p(hc), C.byref(h)))
        return cls(registry, h)

    def __len__(self):
        return int(self._lib.nmn_delta_set_len(self._h))

    @property
    def nnz(self):
        return int(self._lib.nmn_delta_set_nnz(self._h))

    @property
    def host_arrays_present(self):
        """False while a set made on the device holds no host copy of its arrays (nmn_deltaset_host_arrays_present)"""
        return bool(self._lib.nmn_deltaset_host_arrays_present(self._h))

    @property
    def dimension(self):
        return self.registry.dim

    def arrays(self):
        """-> dict of copies: archetype_ids u64 [n], indptr u64 [n + 1], positions u16 [nnz], deltas f32 [nnz], cached_magnitudes f32
        [n], has_cached bool [n], sorted bool [n]"""
        n, nnz = len(self), self.nnz
        a = dict(archetype_ids=np.zeros(n, dtype=np.uint64), indptr=np.zeros(n + 1, dtype=np.uint64), positions=np.zeros(nnz, dtype=np.uint16),
                 deltas=np.zeros(nnz, dtype=np.float32), cached_magnitudes=np.zeros(n, dtype=np.float32), has_cached=np.zeros(n, dtype=np.uint8),
                 sorted=np.zeros(n, dtype=np.uint8))
        _check(self._lib.nmn_delta_set_arrays(self._h, *[_p(v) for v in a.values()]))
        a["has_cached"], a["sorted"] = a["has_cached"].astype(bool), a["sorted"].astype(bool)
        return a

    archetype_ids = property(lambda self: self.arrays()["archetype_ids"])
    indptr = property(lambda self: self.arrays()["indptr"])
    positions = property(lambda self: self.arrays()["positions"])
    deltas = property(lambda self: self.arrays()["deltas"])
    cached_magnitudes = property(lambda self: self.arrays()["cached_magnitudes"])
    has_cached = property(lambda self: self.arrays()["has_cached"])

    def row_nnz(self):
        return np.diff(self.indptr.astype(np.int64))

    def compression_ratio(self):
        out = np.zeros(len(self), dtype=np.float32)
        _check(self._lib.nmn_delta_set_compression_ratio(self._h, _p(out)))
        return out

    def memory_bytes(self):
        out = np.zeros(len(self), dtype=np.uint64)
        _check(self._lib.nmn_delta_set_memory_bytes(self._h, _p(out)))
        return out

    def to_dense(self):
        """to_dense (209-217) of every row -> f32 [n][dim]"""
        out = np.zeros((len(self), self.registry.dim), dtype=np.float32)
        _check(self._lib.nmn_delta_set_decode(self._h, _p(out)))
        return out

    def magnitudes(self):
        """magnitude (260-267) of every row -> f32 [n]"""
        out = np.zeros(len(self), dtype=np.float32)
        _check(self._lib.nmn_delta_set_magnitudes(self._h, _p(out)))
        return out

    def _score(self, fn, queries):
        q = _rows(queries, self.registry.dim, "queries")
        out = np.zeros((q.shape[0], len(self)), dtype=np.float32)
        _check(fn(self._h, _p(q), q.shape[0], _p(out)))
        return out

    def dot_dense(self, queries):
        """dot_dense (309-312) of every row with every query -> f32 [nq][n]"""
        return self._score(self._lib.nmn_delta_set_dot_dense, queries)

    def cosine_similarity_dense(self, queries):
        """cosine_similarity_dense (374-388), query_magnitude = sqrt(sum q * q) -> f32 [nq][n]"""
        return self._score(self._lib.nmn_delta_set_cosine_dense, queries)

    # -- stream-ordered forms on torch tensors ---------------------------------------------------------------------------------
    def to_device(self):
        """make the set and its registry resident (blocks)"""
        _check(self._lib.nmn_delta_set_to_device(self._h))
        return self

    def scratch_floats(self, nq):
        """the floats of scratch a stream-ordered score of nq queries overwrites: nq x (archetypes + 1)"""
        return int(nq) * (len(self.registry) + 1)

    def _score_device(self, fn, queries, out, stream, scratch):
        import torch
        assert queries.dtype == torch.float32 and queries.is_contiguous() and queries.shape[-1] == self.registry.dim
        nq = queries.numel() // self.registry.dim
        if scratch is None:
            # allocated on torch's current stream.  Enqueued on that stream (stream=None) the allocator reuses the block in stream
            # order, after the kernels; on a raw stream of the caller's the block is recorded on it, so it is not recycled early
            scratch = torch.empty(self.scratch_floats(nq), dtype=torch.float32, device=queries.device)
            if stream is not None:
                scratch.record_stream(torch.cuda.ExternalStream(int(stream), device=queries.device))
        assert scratch.dtype == torch.float32 and scratch.is_contiguous() and scratch.numel() >= self.scratch_floats(nq)
        if out is None:
            out = torch.empty((nq, len(self)), dtype=torch.float32, device=queries.device)
        _check(fn(self._h, C.c_void_p(queries.data_ptr()), nq, C.c_void_p(scratch.data_ptr()), C.c_void_p(out.data_ptr()), _stream(stream)))
        return out

    def dot_dense_device(self, queries, out=None, stream=None, scratch=None):
        """nmn_delta_set_dot_dense_device on an f32 tensor [nq][dim]: enqueued, not waited for -> f32 tensor [nq][n].  scratch: an
        f32 tensor of scratch_floats(nq) the caller keeps alive until the kernels have run; None allocates one per call"""
        return self._score_device(self._lib.nmn_delta_set_dot_dense_device, queries, out, stream, scratch)

    def cosine_similarity_dense_device(self, queries, out=None, stream=None, scratch=None):
        return self._score_device(self._lib.nmn_delta_set_cosine_dense_device, queries, out, stream, scratch)

    # -- top-k (docs/delta.md §8) --------------------------------------------------------------------------------------------------
    def search(self, queries, k, metric="dot"):
        """the first min(k, n) rows per query under (score descending, row ascending; -0.0 = +0.0; every NaN alike, below -inf), the
        score being dot_dense's ("dot") or cosine_similarity_dense's ("cosine") -> (rows int64 [nq][k], scores f32 [nq][k], counts
        uint32 [nq]); the unused slots hold row -1 and score -inf.  The scores are the rows' own bits."""
        q = _rows(queries, self.registry.dim, "queries")
        nq, k = q.shape[0], int(k)
        rows = np.full((nq, max(k, 0)), 2 ** 64 - 1, dtype=np.uint64)
        scores = np.full((nq, max(k, 0)), -np.inf, dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        _check(self._lib.nmn_deltaset_search(self._h, _p(q), nq, max(k, 0), _metric(metric), _p(rows), _p(scores), _p(counts)))
        return rows.view(np.int64), scores, counts

    def search_scratch_bytes(self, nq, k):
        """the bytes of scratch a stream-ordered search of nq queries overwrites (nmn_deltaset_search_scratch_bytes)"""
        return int(self._lib.nmn_deltaset_search_scratch_bytes(self._h, int(nq), int(k)))

    def search_device(self, queries, k, metric="dot", stream=None, scratch=None):
        """nmn_deltaset_search_device on an f32 tensor [nq][dim]: enqueued, not waited for -> (rows int64 tensor [nq][k], scores f32
        tensor [nq][k], counts int32 tensor [nq]).  scratch: a uint8 tensor of search_scratch_bytes(nq, k) the caller keeps alive until
        the kernels have run; None allocates one per call, as the stream-ordered scores do"""
        import torch
        assert queries.dtype == torch.float32 and queries.is_contiguous() and queries.shape[-1] == self.registry.dim
        nq, k = queries.numel() // self.registry.dim, int(k)
        need = self.search_scratch_bytes(nq, k)
        if scratch is None:
            scratch = torch.empty(max(need, 16), dtype=torch.uint8, device=queries.device)
            if stream is not None:
                scratch.record_stream(torch.cuda.ExternalStream(int(stream), device=queries.device))
        assert scratch.dtype == torch.uint8 and scratch.is_contiguous()
        rows = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=queries.device)
        scores = torch.empty((nq, max(k, 0)), dtype=torch.float32, device=queries.device)
        counts = torch.empty(nq, dtype=torch.int32, device=queries.device)
        _check(self._lib.nmn_deltaset_search_device(self._h, C.c_void_p(queries.data_ptr()), nq, max(k, 0), _metric(metric),
                                                    C.c_void_p(scratch.data_ptr()), scratch.numel(), C.c_void_p(rows.data_ptr()),
                                                    C.c_void_p(scores.data_ptr()), C.c_void_p(counts.data_ptr()), _stream(stream)))
        return rows, scores, counts
