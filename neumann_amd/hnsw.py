"""HNSW graph index searched on the GPU — host wrapper of `nmn_hnsw_*` (include/neumann_gpu.h).

Mirrors `tensor_store::HNSWIndex` with dense or 8-bit quantized storage (tensor_store/src/hnsw.rs:1554-2335): `insert` builds the graph on the
host in the reference's order (level generator, search_layer with ef_construction, stable pruning), `search` /
`search_device` run `search_with_ef` as one HIP kernel launch per chunk of queries, one query per wave.  Answers are the
reference's bit for bit, ties included (docs/hnsw.md)."""
import ctypes as C
import math

import numpy as np

from . import _capi
from .flat_index import DistanceMetric, GpuFlatIndex, _stream_ptr


class HNSWConfig:
    """HNSWConfig (hnsw.rs:1434-1551)."""

    def __init__(self, m=16, m0=None, ef_construction=200, ef_search=50, ml=None, sparsity_threshold=0.5, max_nodes=10_000_000,
                 distance_metric=DistanceMetric.Cosine, storage="dense"):
        self.m = int(m)
        self.m0 = 2 * self.m if m0 is None else int(m0)
        self.ef_construction = int(ef_construction)
        self.ef_search = int(ef_search)
        self.ml = 1.0 / math.log(self.m) if ml is None else float(ml)
        self.sparsity_threshold = float(sparsity_threshold)
        self.max_nodes = int(max_nodes)
        self.distance_metric = DistanceMetric(int(distance_metric))
        # the older home of HNSWStorageStrategy: GpuHnsw(config) serves "dense" here and refuses the others.  The strategy's home
        # is HNSWBuildOptions.storage / GpuHnsw(..., storage=...), as in the reference.
        self.storage = storage

    @classmethod
    def default(cls):
        return cls()

    @classmethod
    def high_recall(cls):  # hnsw.rs:1508-1519
        return cls(m=32, m0=64, ef_construction=400, ef_search=200)

    @classmethod
    def high_speed(cls):  # hnsw.rs:1523-1534
        return cls(m=8, m0=16, ef_construction=100, ef_search=20)

    def with_distance_metric(self, metric):  # hnsw.rs:1547-1550
        self.distance_metric = DistanceMetric(int(metric))
        return self

    def _c(self):
        try:
            storage = {"dense": _capi.HNSW_STORAGE_DENSE, "auto": _capi.HNSW_STORAGE_AUTO,
                       "quantized": _capi.HNSW_STORAGE_QUANTIZED}[self.storage]
        except KeyError:
            raise _capi.NeumannGpuError(_capi.ERR_CONFIGURATION, f"unknown HNSW storage strategy {self.storage!r}")
        return _capi.HnswConfig(m=self.m, m0=self.m0, ef_construction=self.ef_construction, ef_search=self.ef_search, ml=self.ml,
                                max_nodes=self.max_nodes, sparsity_threshold=self.sparsity_threshold,
                                distance_metric=int(self.distance_metric), storage=storage, reserved=0)

    @classmethod
    def _from_c(cls, c):
        return cls(m=c.m, m0=c.m0, ef_construction=c.ef_construction, ef_search=c.ef_search, ml=c.ml,
                   sparsity_threshold=c.sparsity_threshold, max_nodes=c.max_nodes, distance_metric=c.distance_metric)


_STORAGE = {"dense": _capi.HNSW_STORAGE_DENSE, "auto": _capi.HNSW_STORAGE_AUTO, "quantized": _capi.HNSW_STORAGE_QUANTIZED,
            "binary": _capi.HNSW_STORAGE_BINARY}
_BINARY_THRESHOLD = {"sign": _capi.BINARY_SIGN, "mean": _capi.BINARY_MEAN, "median": _capi.BINARY_MEDIAN}


def _storage_code(storage):
    try:
        return _STORAGE[storage]
    except KeyError:
        raise _capi.NeumannGpuError(_capi.ERR_CONFIGURATION, f"unknown HNSW storage strategy {storage!r}")


def _csr(indptr, positions, values, n):
    """the CSR triple of a sparse call as contiguous (indptr u64, positions u32, values f32); `n`: what the message calls the row count"""
    ip = np.ascontiguousarray(indptr, dtype=np.uint64).reshape(-1)
    pos = np.ascontiguousarray(positions, dtype=np.uint32).reshape(-1)
    val = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    if ip.size == 0 or pos.size != val.size or (ip.size and int(ip.max()) > pos.size):
        raise _capi.NeumannGpuError(_capi.ERR_INVALID_ARGUMENT, f"indptr [{n} + 1] into positions / values of one length")
    return ip, pos, val


def _per_query(k, ef, kstride, nq, what):
    """the arrays of a _multi call -> (k u32 [nq], ef u32 [nq] or None, kstride: max(k) when None); `what`: the message of a wrong length"""
    kk = np.ascontiguousarray(k, dtype=np.uint32).reshape(-1)
    ee = None if ef is None else np.ascontiguousarray(ef, dtype=np.uint32).reshape(-1)
    if kk.size != nq or (ee is not None and ee.size != nq):
        raise _capi.NeumannGpuError(_capi.ERR_INVALID_ARGUMENT, what)
    return kk, ee, int(kk.max()) if kstride is None and nq else int(kstride or 1)


def _host_out(nq, k):
    """what a host call answers into: (ids u64 [nq,k], scores f32 [nq,k], counts u32 [nq], stats), a row at least one slot long"""
    kk = max(k, 1)
    return (np.empty((nq, kk), dtype=np.uint64), np.empty((nq, kk), dtype=np.float32), np.empty(nq, dtype=np.uint32),
            _capi.SearchStats())


def _device_out(out, nq, k, device):
    """`out` of a _device call, or (ids int64 [nq,k], scores f32 [nq,k], counts int32 [nq]) allocated on `device`"""
    import torch

    if out is not None:
        ids, sc, counts = out
        return ids, sc, counts
    kk = max(k, 1)
    return (torch.empty((nq, kk), dtype=torch.int64, device=device), torch.empty((nq, kk), dtype=torch.float32, device=device),
            torch.empty((nq,), dtype=torch.int32, device=device))


def _device_csr(indptr_t, positions_t, values_t):
    """the CSR of a sparse _device call checked -> (indptr, positions, values, nq, nnz_total): contiguous device tensors, int64
    indptr [nq + 1] read as u64, int32 positions read as u32, float32 values of the same length"""
    import torch

    for t, dt, what in ((indptr_t, torch.int64, "indptr must be a contiguous int64 device tensor [nq + 1]"),
                        (positions_t, torch.int32, "positions must be a contiguous int32 device tensor"),
                        (values_t, torch.float32, "values must be a contiguous float32 device tensor")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dt and t.is_contiguous() and t.dim() == 1):
            raise _capi.NeumannGpuError(_capi.ERR_INVALID_ARGUMENT, what)
    if indptr_t.numel() < 1 or positions_t.numel() != values_t.numel():
        raise _capi.NeumannGpuError(_capi.ERR_INVALID_ARGUMENT, "indptr is [nq + 1]; positions and values have one length")
    return indptr_t, positions_t, values_t, indptr_t.numel() - 1, positions_t.numel()


def _device_status(status, nq, device):
    """`status` of a sparse _device call (int32 [nq]), or one allocated on `device`"""
    import torch

    return status if status is not None else torch.empty((nq,), dtype=torch.int32, device=device)


def sparse_canonicalise_device(dim, indptr_t, positions_t, values_t, max_nnz=None, dense=True, stream=None):
    """SparseVector::try_from_parts, magnitude and to_dense of CSR queries in torch device tensors, in stream order
    (nmn_sparse_canonicalise_device; docs/hnsw.md §22): int64 `indptr_t` [nq + 1] read as u64, int32 `positions_t` read as u32,
    float32 `values_t`; `max_nnz`: the bound on one query's raw entries (None: min(dim, 4096)).  Enqueued on `stream` (None:
    torch's current stream), nothing is read back.  Returns a dict of device tensors: off int64 [nq + 1], entries int32 [nnz, 2]
    ({position, value bits}, the first off[nq] rows are written), mag f32 [nq], dup int32 [nq], dense f32 [nq, dim] (None with
    `dense` false), status int32 [nq] (0 served, 1 a position >= dim, 2 the range or the count)."""
    import torch

    ip, pos, val, nq, nnz = _device_csr(indptr_t, positions_t, values_t)
    dev, dim = ip.device, int(dim)
    out = {
        "off": torch.empty((nq + 1,), dtype=torch.int64, device=dev),
        "entries": torch.empty((max(nnz, 1), 2), dtype=torch.int32, device=dev),
        "mag": torch.empty((nq,), dtype=torch.float32, device=dev),
        "dup": torch.empty((nq,), dtype=torch.int32, device=dev),
        "dense": torch.empty((nq, dim), dtype=torch.float32, device=dev) if dense else None,
        "status": torch.empty((nq,), dtype=torch.int32, device=dev),
    }
    _capi.check(_capi.load().nmn_sparse_canonicalise_device(
        dim, C.c_void_p(ip.data_ptr()), C.c_void_p(pos.data_ptr()), C.c_void_p(val.data_ptr()), nq, nnz,
        0 if max_nnz is None else int(max_nnz), C.c_void_p(out["off"].data_ptr()), C.c_void_p(out["entries"].data_ptr()),
        C.c_void_p(out["mag"].data_ptr()), C.c_void_p(out["dup"].data_ptr()),
        C.c_void_p(out["dense"].data_ptr()) if dense else None, C.c_void_p(out["status"].data_ptr()),
        dev.index if dev.index is not None else -1, _stream_ptr(stream)))
    return out


class HNSWBuildOptions:
    """HNSWBuildOptions (vector_engine/src/lib.rs:848-932): a storage strategy ("dense", "auto", "quantized") and an HNSWConfig."""

    def __init__(self, storage="dense", hnsw_config=None):
        self.storage = storage
        self.hnsw_config = hnsw_config or HNSWConfig()

    @classmethod
    def default(cls):  # lib.rs:860-867
        return cls("dense", HNSWConfig.default())

    new = default

    @classmethod
    def memory_optimized(cls):  # lib.rs:880-885
        return cls("quantized", HNSWConfig.high_speed())

    @classmethod
    def high_recall(cls):  # lib.rs:891-896
        return cls("dense", HNSWConfig.high_recall())

    @classmethod
    def sparse_optimized(cls):  # lib.rs:902-907
        return cls("auto", HNSWConfig.default())

    def with_storage(self, storage):  # lib.rs:911-914
        self.storage = storage
        return self

    def with_hnsw_config(self, config):  # lib.rs:918-921
        self.hnsw_config = config
        return self

    def with_sparsity_threshold(self, threshold):  # lib.rs:928-931
        self.hnsw_config.sparsity_threshold = float(threshold)
        return self


class GpuHnsw:
    def __init__(self, dim, config=None, capacity_hint=0, device=-1, storage=None, binary_threshold=None):
        """storage None: nmn_hnsw_create (config.storage, dense only).  storage "dense" / "quantized": the strategy of
        HNSWBuildOptions through nmn_hnsw_create_with_storage (config.storage is not read; "auto" is refused).  storage "binary":
        every node EmbeddingStorage::Binary(BinaryVector::from_dense(row, threshold)) through nmn_hnsw_create_binary,
        binary_threshold "sign" (the default), "mean" or "median" (docs/hnsw.md §18)."""
        self._lib = _capi.load()
        self._h = None
        self.config = config or HNSWConfig()
        self.dim = int(dim)
        cfg = self.config._c()
        h = C.c_void_p()
        if binary_threshold is not None and storage != "binary":
            raise _capi.NeumannGpuError(_capi.ERR_CONFIGURATION, "binary_threshold goes with storage='binary'")
        if storage is None:
            _capi.check(self._lib.nmn_hnsw_create(C.byref(cfg), self.dim, int(capacity_hint), int(device), C.byref(h)))
        elif storage == "binary":
            try:
                method = _BINARY_THRESHOLD[binary_threshold or "sign"]
            except KeyError:
                raise _capi.NeumannGpuError(_capi.ERR_CONFIGURATION, f"unknown binary threshold {binary_threshold!r}")
            cfg.storage = _capi.HNSW_STORAGE_DENSE
            _capi.check(self._lib.nmn_hnsw_create_binary(C.byref(cfg), method, self.dim, int(capacity_hint), int(device), C.byref(h)))
        else:
            cfg.storage = _capi.HNSW_STORAGE_DENSE
            _capi.check(self._lib.nmn_hnsw_create_with_storage(C.byref(cfg), _storage_code(storage), self.dim, int(capacity_hint),
                                                               int(device), C.byref(h)))
        self._h = h

    def save(self, path):
        """Graph, level generator state and rows -> `path` (nmn_hnsw_save; the format is docs/hnsw.md §10).  Searches may run
        meanwhile, inserts wait."""
        _capi.check(self._lib.nmn_hnsw_save(self._h, str(path).encode()))

    @classmethod
    def load(cls, path, device=-1, capacity_hint=0, max_file_bytes=0, max_entries=0):
        """nmn_hnsw_load: no build — graph, rows and generator state come back exactly as saved, so searches answer the same bits
        and `insert` continues where the saved index would have.  `config`, `dim` and `storage` are the file's.  Every index of
        the file is checked on the host before anything reaches the GPU; a damaged file is ERR_SERIALIZATION."""
        lib = _capi.load()
        h = C.c_void_p()
        _capi.check(lib.nmn_hnsw_load(str(path).encode(), int(device), int(capacity_hint), int(max_file_bytes), int(max_entries),
                                      C.byref(h)))
        g = cls.__new__(cls)
        g._lib, g._h = lib, h
        g._adopt_config()
        return g

    def _adopt_config(self):
        """config and dim as the handle holds them (nmn_hnsw_get_config)"""
        c = _capi.HnswConfig()
        _capi.check(self._lib.nmn_hnsw_get_config(self._h, C.byref(c)))
        self.config = HNSWConfig._from_c(c)
        self.config.storage = {v: k for k, v in _STORAGE.items()}[int(c.storage)]
        self.dim = int(self._lib.nmn_hnsw_dim(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.nmn_hnsw_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return int(self._lib.nmn_hnsw_len(self._h))

    @property
    def entry_point(self):
        """node id of the entry point, None while the index is empty"""
        e = int(self._lib.nmn_hnsw_entry_point(self._h))
        return None if e == 0xFFFFFFFFFFFFFFFF else e

    @property
    def max_layer(self):
        return int(self._lib.nmn_hnsw_max_layer(self._h))

    @property
    def hbm_bytes(self):
        return int(self._lib.nmn_hnsw_hbm_bytes(self._h))

    def _rows(self, rows):
        """rows or queries -> contiguous f32 [n, dim] (a single one: [1, dim]), the dimension checked"""
        r = np.ascontiguousarray(rows, dtype=np.float32)
        if r.ndim == 1:
            r = r[None, :]
        if r.shape[1] != self.dim:
            raise _capi.NeumannGpuError(_capi.ERR_DIMENSION_MISMATCH, f"expected {self.dim}, got {r.shape[1]}")
        return r

    def _device_queries(self, queries_t, k):
        """the queries of a _device call checked -> (contiguous f32 device tensor [nq, dim], nq, int(k))"""
        import torch

        if not (isinstance(queries_t, torch.Tensor) and queries_t.is_cuda):
            raise _capi.NeumannGpuError(_capi.ERR_INVALID_ARGUMENT, "queries must be a device tensor")
        if queries_t.dtype != torch.float32 or not queries_t.is_contiguous():
            raise _capi.NeumannGpuError(_capi.ERR_INVALID_ARGUMENT, "queries must be contiguous float32")
        if queries_t.dim() == 1:
            queries_t = queries_t[None, :]
        nq, k = queries_t.shape[0], int(k)
        if queries_t.shape[1] != self.dim:
            raise _capi.NeumannGpuError(_capi.ERR_DIMENSION_MISMATCH, f"expected {self.dim}")
        return queries_t, nq, k

    def insert(self, rows):
        """HNSWIndex::insert for each row in order; returns the node ids."""
        r = self._rows(rows)
        ids = np.empty(r.shape[0], dtype=np.uint64)
        _capi.check(self._lib.nmn_hnsw_insert(self._h, C.c_void_p(r.ctypes.data), r.shape[0], C.c_void_p(ids.ctypes.data)))
        return ids

    def insert_bulk(self, rows):
        """`insert` with the searches of every new node walked on the GPU, a batch of nodes per launch, and committed on the host
        in order (nmn_hnsw_insert_bulk, docs/hnsw.md §19): the same graph, ids and generator state; returns the node ids."""
        r = self._rows(rows)
        ids = np.empty(r.shape[0], dtype=np.uint64)
        _capi.check(self._lib.nmn_hnsw_insert_bulk(self._h, C.c_void_p(r.ctypes.data), r.shape[0], C.c_void_p(ids.ctypes.data)))
        return ids

    def set_bulk_policy(self, batch=0, min_nodes=0):
        """how `insert_bulk` cuts its batches, never what it builds: nodes per launch (0 = adaptive, 8 at first, 4 .. 256) and
        the graph size from which the device walks (0 = 100 000)"""
        _capi.check(self._lib.nmn_hnsw_set_bulk_policy(self._h, int(batch), int(min_nodes)))

    def bulk_stats(self):
        """counters of `insert_bulk`, cumulative per handle, as a dict: batches, walks, accepted, conflicts, overflowed
        (accepted + conflicts + overflowed == walks), host_nodes, patched_lists"""
        st = _capi.HnswBulkStats()
        _capi.check(self._lib.nmn_hnsw_get_bulk_stats(self._h, C.byref(st)))
        return {n: int(getattr(st, n)) for n, _ in st._fields_}

    def bulk_trace(self):
        """the batches of the last `insert_bulk` call -> f32 [batches, 5]: nodes walked, nodes walked again on the host,
        milliseconds of the walk launch, of validation and commits, of the patch"""
        cnt = C.c_uint64()
        _capi.check(self._lib.nmn_hnsw_get_bulk_trace(self._h, None, 0, C.byref(cnt)))
        out = np.empty((cnt.value, 5), dtype=np.float32)
        if cnt.value:
            _capi.check(self._lib.nmn_hnsw_get_bulk_trace(self._h, C.c_void_p(out.ctypes.data), cnt.value, C.byref(cnt)))
        return out

    def insert_sparse(self, indptr, positions, values):
        """HNSWIndex::insert_sparse for each CSR row in order (nmn_hnsw_insert_sparse); returns the node ids.  Row i is the
        (position, value) pairs [indptr[i], indptr[i + 1]), made a SparseVector as try_from_parts does (`search_sparse`'s rules);
        the node is stored Sparse and scored by SparseVector's own arithmetic (docs/hnsw.md §15).  Dense handles only."""
        ip, pos, val = _csr(indptr, positions, values, "n")
        n = ip.size - 1
        ids = np.empty(n, dtype=np.uint64)
        _capi.check(self._lib.nmn_hnsw_insert_sparse(self._h, C.c_void_p(ip.ctypes.data), C.c_void_p(pos.ctypes.data),
                                                     C.c_void_p(val.ctypes.data), n, C.c_void_p(ids.ctypes.data)))
        return ids

    def insert_auto(self, rows):
        """HNSWIndex::insert_auto for each row in order (nmn_hnsw_insert_auto): a row whose share of zeros reaches
        config.sparsity_threshold is stored Sparse(from_dense(row)), every other Dense; returns the node ids."""
        r = self._rows(rows)
        ids = np.empty(r.shape[0], dtype=np.uint64)
        _capi.check(self._lib.nmn_hnsw_insert_auto(self._h, C.c_void_p(r.ctypes.data), r.shape[0], C.c_void_p(ids.ctypes.data)))
        return ids

    def sparse_row(self, node):
        """the stored entries of a Sparse node -> (positions u32, values f32), in SparseVector order; None for a Dense node"""
        nnz = C.c_uint32()
        _capi.check(self._lib.nmn_hnsw_sparse_row(self._h, int(node), None, None, 0, C.byref(nnz)))
        if nnz.value == 0xFFFFFFFF:
            return None
        pos = np.empty(nnz.value, dtype=np.uint32)
        val = np.empty(nnz.value, dtype=np.float32)
        _capi.check(self._lib.nmn_hnsw_sparse_row(self._h, int(node), C.c_void_p(pos.ctypes.data), C.c_void_p(val.ctypes.data),
                                                  nnz.value, C.byref(nnz)))
        return pos, val

    def levels(self):
        out = np.empty(len(self), dtype=np.uint32)
        _capi.check(self._lib.nmn_hnsw_levels(self._h, C.c_void_p(out.ctypes.data), out.size))
        return out

    def neighbors(self, node, layer):
        """neighbour ids of `node` on `layer`, ascending (empty above the node's level)"""
        cap = max(self.config.m, self.config.m0)
        out = np.empty(cap, dtype=np.uint64)
        cnt = C.c_uint32()
        _capi.check(self._lib.nmn_hnsw_neighbors(self._h, int(node), int(layer), C.c_void_p(out.ctypes.data), cap, C.byref(cnt)))
        return out[:cnt.value].copy()

    def vectors(self):
        """the flat index holding the rows (node id == row), valid until the next insert; None on a quantized or binary handle"""
        v = self._lib.nmn_hnsw_vectors(self._h)
        return GpuFlatIndex._view(v, self) if v else None

    @property
    def storage(self):
        """"dense", "quantized" or "binary": the handle's one storage"""
        code = int(self._lib.nmn_hnsw_storage(self._h))
        return {v: k for k, v in _STORAGE.items()}[code]

    def quantized_row(self, node):
        """the node's ScalarQuantizedVector -> (codes u8 [dim], scale f32, min_val f32)"""
        codes = np.empty(self.dim, dtype=np.uint8)
        scale, mn = C.c_float(), C.c_float()
        _capi.check(self._lib.nmn_hnsw_quantized_row(self._h, int(node), C.c_void_p(codes.ctypes.data), C.byref(scale), C.byref(mn)))
        return codes, np.float32(scale.value), np.float32(mn.value)

    @property
    def binary_threshold(self):
        """"sign", "mean" or "median" on a binary handle, None on any other"""
        code = int(self._lib.nmn_hnsw_binary_threshold(self._h))
        return {v: k for k, v in _BINARY_THRESHOLD.items()}.get(code)

    def binary_row(self, node):
        """the node's BinaryVector -> u64 words [ceil(dim / 64)], bit i of word i // 64 = element i above the threshold"""
        words = np.empty((self.dim + 63) // 64, dtype=np.uint64)
        _capi.check(self._lib.nmn_hnsw_binary_row(self._h, int(node), C.c_void_p(words.ctypes.data), words.size))
        return words

    def get_vector(self, node):
        """HNSWIndex::get_vector: the row as inserted (dense), to_dense() of a sparse node, dequantize() (quantized), or the
        +1.0 / -1.0 row of to_dense() (binary)"""
        out = np.empty(self.dim, dtype=np.float32)
        _capi.check(self._lib.nmn_hnsw_get_vector(self._h, int(node), C.c_void_p(out.ctypes.data)))
        return out

    def memory_stats(self):
        """HNSWIndex::memory_stats (hnsw.rs:2733-2768) as a dict"""
        st = _capi.HnswMemStats()
        _capi.check(self._lib.nmn_hnsw_memory_stats(self._h, C.byref(st)))
        return {n: int(getattr(st, n)) for n, _ in st._fields_}

    def set_heap_capacity(self, results=0, candidates=0):
        """entries of the two heaps a wave keeps in LDS (0 = default); what outgrows them goes to the spill launch"""
        _capi.check(self._lib.nmn_hnsw_set_heap_capacity(self._h, int(results), int(candidates)))

    def search(self, queries, k, ef=None, with_stats=False):
        """-> (ids u64 [nq,k], scores f32 [nq,k], counts u32 [nq]); HNSWIndex::search_with_ef per query (ef None: ef_search)."""
        q = self._rows(queries)
        nq, k = q.shape[0], int(k)
        ids, sc, counts, st = _host_out(nq, k)
        _capi.check(self._lib.nmn_hnsw_search(self._h, C.c_void_p(q.ctypes.data), nq, k, 0 if ef is None else int(ef),
                                              C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data),
                                              C.c_void_p(counts.ctypes.data), C.byref(st)))
        return (ids, sc, counts, st) if with_stats else (ids, sc, counts)

    def search_multi(self, queries, k, ef=None, kstride=None, with_stats=False):
        """`search` with a k and an ef per query in ONE launch (nmn_hnsw_search_multi).  `k`: one integer per query; `ef`: None
        (ef_search for all) or one per query, 0 = ef_search; `kstride`: row length of the outputs (None: max(k)).
        -> (ids u64 [nq,kstride], scores f32 [nq,kstride], counts u32 [nq]); row i is what search(q_i, k[i], ef[i]) answers."""
        q = self._rows(queries)
        nq = q.shape[0]
        kk, ee, ks = _per_query(k, ef, kstride, nq, "one k (and one ef) per query")
        ids, sc, counts, st = _host_out(nq, ks)
        _capi.check(self._lib.nmn_hnsw_search_multi(self._h, C.c_void_p(q.ctypes.data), nq, C.c_void_p(kk.ctypes.data),
                                                    C.c_void_p(ee.ctypes.data) if ee is not None else None, ks,
                                                    C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data),
                                                    C.c_void_p(counts.ctypes.data), C.byref(st)))
        return (ids, sc, counts, st) if with_stats else (ids, sc, counts)

    @staticmethod
    def sparse_from_dense(queries):
        """SparseVector::from_dense (sparse_vector.rs:212-236) row by row -> CSR (indptr u64 [nq + 1], positions u32, values f32):
        a value is stored iff it `!= 0.0` — both zeros are skipped, NaN is stored — in position order."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        keep = q != 0
        indptr = np.zeros(q.shape[0] + 1, dtype=np.uint64)
        indptr[1:] = np.cumsum(keep.sum(axis=1))
        return indptr, np.nonzero(keep)[1].astype(np.uint32), q[keep]

    def search_sparse(self, indptr, positions, values, k, ef=None, with_stats=False):
        """HNSWIndex::search_sparse_with_ef per query (nmn_hnsw_search_sparse; ef None: ef_search).  Query i is the (position, value)
        pairs [indptr[i], indptr[i + 1]) of `positions` / `values`, in any order; they are made a SparseVector as try_from_parts
        does (zeros dropped, stably sorted by position; a position >= dim is refused).
        -> (ids u64 [nq,k], scores f32 [nq,k], counts u32 [nq])"""
        ip, pos, val = _csr(indptr, positions, values, "nq")
        nq, k = ip.size - 1, int(k)
        ids, sc, counts, st = _host_out(nq, k)
        _capi.check(self._lib.nmn_hnsw_search_sparse(self._h, C.c_void_p(ip.ctypes.data), C.c_void_p(pos.ctypes.data),
                                                     C.c_void_p(val.ctypes.data), nq, k, 0 if ef is None else int(ef),
                                                     C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data),
                                                     C.c_void_p(counts.ctypes.data), C.byref(st)))
        return (ids, sc, counts, st) if with_stats else (ids, sc, counts)

    def search_sparse_multi(self, indptr, positions, values, k, ef=None, kstride=None, with_stats=False):
        """`search_sparse` with a k and an ef per query in ONE launch (nmn_hnsw_search_sparse_multi).  The CSR is `search_sparse`'s;
        `k`: one integer per query; `ef`: None (ef_search for all) or one per query, 0 = ef_search; `kstride`: row length of the
        outputs (None: max(k)).
        -> (ids u64 [nq,kstride], scores f32 [nq,kstride], counts u32 [nq]); row i is what search_sparse(q_i, k[i], ef[i]) answers."""
        ip, pos, val = _csr(indptr, positions, values, "nq")
        nq = ip.size - 1
        kk, ee, ks = _per_query(k, ef, kstride, nq, "one k (and one ef) per query")
        ids, sc, counts, st = _host_out(nq, ks)
        _capi.check(self._lib.nmn_hnsw_search_sparse_multi(self._h, C.c_void_p(ip.ctypes.data), C.c_void_p(pos.ctypes.data),
                                                           C.c_void_p(val.ctypes.data), nq, C.c_void_p(kk.ctypes.data),
                                                           C.c_void_p(ee.ctypes.data) if ee is not None else None, ks,
                                                           C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data),
                                                           C.c_void_p(counts.ctypes.data), C.byref(st)))
        return (ids, sc, counts, st) if with_stats else (ids, sc, counts)

    def coalesce_stats(self):
        """(batches that carried two or more concurrent calls, calls in them) — nmn_hnsw_coalesce_stats"""
        b, c = C.c_uint64(), C.c_uint64()
        _capi.check(self._lib.nmn_hnsw_coalesce_stats(self._h, C.byref(b), C.byref(c)))
        return int(b.value), int(c.value)

    def search_device(self, queries_t, k, ef=None, out=None, stream=None):
        """`search` with torch device tensors, in stream order (nmn_hnsw_search_device): enqueued on `stream` (None: torch's
        current stream), returns without waiting.  Returns (ids int64 [nq,k] holding the u64 bit pattern, -1 = unused slot;
        scores f32 [nq,k]; counts int32 [nq]), allocated on the queries' device unless `out` supplies them."""
        queries_t, nq, k = self._device_queries(queries_t, k)
        ids, sc, counts = _device_out(out, nq, k, queries_t.device)
        _capi.check(self._lib.nmn_hnsw_search_device(
            self._h, C.c_void_p(queries_t.data_ptr()), nq, k, 0 if ef is None else int(ef), C.c_void_p(ids.data_ptr()),
            C.c_void_p(sc.data_ptr()), C.c_void_p(counts.data_ptr()), _stream_ptr(stream)))
        return ids, sc, counts

    def search_sparse_device(self, indptr_t, positions_t, values_t, k, ef=None, max_nnz=None, out=None, status=None, stream=None):
        """`search_sparse` with torch device tensors, in stream order (nmn_hnsw_search_sparse_device; docs/hnsw.md §22): int64
        `indptr_t` [nq + 1] read as u64, int32 `positions_t` read as u32, float32 `values_t`, canonicalised on the GPU; `max_nnz`:
        the bound on one query's raw entries, at most 4096 (None: min(dim, 4096)).  Enqueued on `stream` (None: torch's current
        stream), returns without waiting.  Returns (ids, scores, counts, status): the first three as `search_device` returns them
        (`out` supplies them), status int32 [nq] (`status` supplies it): 0 served, 1 a position >= dim, 2 the range or the count,
        3 a duplicated position on an index with sparse nodes — the row of a query with a status is count 0 with the sentinels."""
        ip, pos, val, nq, nnz = _device_csr(indptr_t, positions_t, values_t)
        k = int(k)
        ids, sc, counts = _device_out(out, nq, k, ip.device)
        status = _device_status(status, nq, ip.device)
        _capi.check(self._lib.nmn_hnsw_search_sparse_device(
            self._h, C.c_void_p(ip.data_ptr()), C.c_void_p(pos.data_ptr()), C.c_void_p(val.data_ptr()), nq, nnz,
            0 if max_nnz is None else int(max_nnz), k, 0 if ef is None else int(ef), C.c_void_p(ids.data_ptr()),
            C.c_void_p(sc.data_ptr()), C.c_void_p(counts.data_ptr()), C.c_void_p(status.data_ptr()), _stream_ptr(stream)))
        return ids, sc, counts, status

    def search_tt(self, tts, k, ef=None, with_stats=False):
        """HNSWIndex::search_tt_with_ef per train (nmn_hnsw_search_tt; ef None: ef_search).  `tts`: one neumann_amd.tt.TTVector or
        several of one shape whose product is the index's dimension.  The trains are reconstructed and their norms taken on the
        GPU; the walk scores under Cosine whatever the index's metric is, the score is 1 - distance (docs/hnsw.md §17).
        -> (ids u64 [nq,k], scores f32 [nq,k], counts u32 [nq])"""
        from . import tt as _tt
        shape, ranks, off, cores = _tt.pack(tts)
        nq, k = ranks.shape[0], int(k)
        ids, sc, counts, st = _host_out(nq, k)
        _capi.check(self._lib.nmn_hnsw_search_tt(self._h, C.c_void_p(shape.ctypes.data), shape.size, C.c_void_p(ranks.ctypes.data),
                                                 C.c_void_p(off.ctypes.data), C.c_void_p(cores.ctypes.data), nq, k,
                                                 0 if ef is None else int(ef), C.c_void_p(ids.ctypes.data),
                                                 C.c_void_p(sc.ctypes.data), C.c_void_p(counts.ctypes.data), C.byref(st)))
        return (ids, sc, counts, st) if with_stats else (ids, sc, counts)

    def search_tt_device(self, shape, ranks, cores_t, k, ef=None, out=None, stream=None):
        """`search_tt` with the core data in a torch device tensor, in stream order (nmn_hnsw_search_tt_device): `cores_t` is
        float32 [nq, storage] — every train's cores back to back — and ONE rank vector `ranks` [len(shape) + 1] serves the whole
        call.  Preparation and walk are enqueued on `stream` (None: torch's current stream); nothing is read back.  Returns
        (ids int64 [nq,k], -1 = unused slot; scores f32 [nq,k]; counts int32 [nq]) like `search_device`."""
        import torch

        if not (isinstance(cores_t, torch.Tensor) and cores_t.is_cuda):
            raise _capi.NeumannGpuError(_capi.ERR_INVALID_ARGUMENT, "cores must be a device tensor")
        if cores_t.dtype != torch.float32 or not cores_t.is_contiguous() or cores_t.dim() != 2:
            raise _capi.NeumannGpuError(_capi.ERR_INVALID_ARGUMENT, "cores must be contiguous float32 [nq, storage]")
        sh = np.ascontiguousarray(shape, dtype=np.uint32).reshape(-1)
        rk = np.ascontiguousarray(ranks, dtype=np.uint32).reshape(-1)
        if rk.size != sh.size + 1:
            raise _capi.NeumannGpuError(_capi.ERR_INVALID_ARGUMENT, "TT: ranks is [n_cores + 1]")
        storage = int(sum(int(rk[i]) * int(sh[i]) * int(rk[i + 1]) for i in range(sh.size)))
        if cores_t.shape[1] != storage:
            raise _capi.NeumannGpuError(_capi.ERR_INVALID_ARGUMENT, f"TT: a train of these ranks holds {storage} floats")
        nq, k = cores_t.shape[0], int(k)
        ids, sc, counts = _device_out(out, nq, k, cores_t.device)
        _capi.check(self._lib.nmn_hnsw_search_tt_device(
            self._h, C.c_void_p(sh.ctypes.data), sh.size, C.c_void_p(rk.ctypes.data), C.c_void_p(cores_t.data_ptr()), nq, k,
            0 if ef is None else int(ef), C.c_void_p(ids.data_ptr()), C.c_void_p(sc.data_ptr()), C.c_void_p(counts.data_ptr()),
            _stream_ptr(stream)))
        return ids, sc, counts

    def insert_tt(self, tts):
        """HNSWIndex::insert_tt_vector for each train in order (nmn_hnsw_insert_tt): reconstructed on the GPU, inserted as Dense
        nodes by `insert`'s path; returns the node ids.  Dense handles only."""
        from . import tt as _tt
        shape, ranks, off, cores = _tt.pack(tts)
        n = ranks.shape[0]
        ids = np.empty(n, dtype=np.uint64)
        _capi.check(self._lib.nmn_hnsw_insert_tt(self._h, C.c_void_p(shape.ctypes.data), shape.size, C.c_void_p(ranks.ctypes.data),
                                                 C.c_void_p(off.ctypes.data), C.c_void_p(cores.ctypes.data), n,
                                                 C.c_void_p(ids.ctypes.data)))
        return ids

    def insert_embedding_tt(self, tts):
        """HNSWIndex::insert_embedding(EmbeddingStorage::from(tt)) for each train in order (nmn_hnsw_insert_embedding_tt):
        TensorTrain nodes, which keep the train and its cached tt_norm and are scored by their own rules (docs/hnsw.md §24) —
        not the Dense nodes `insert_tt` makes.  `tts`: one neumann_amd.tt.TTVector or several of one shape whose product is the
        index's dimension; another call may bring another shape of that product.  Returns the node ids.  Dense handles only."""
        from . import tt as _tt
        shape, ranks, off, cores = _tt.pack(tts)
        n = ranks.shape[0]
        ids = np.empty(n, dtype=np.uint64)
        _capi.check(self._lib.nmn_hnsw_insert_embedding_tt(self._h, C.c_void_p(shape.ctypes.data), shape.size,
                                                           C.c_void_p(ranks.ctypes.data), C.c_void_p(off.ctypes.data),
                                                           C.c_void_p(cores.ctypes.data), n, C.c_void_p(ids.ctypes.data)))
        return ids

    def tt_row(self, node):
        """the train of a TensorTrain node as a neumann_amd.tt.TTVector (nmn_hnsw_tt_row); None for a node of another kind"""
        from . import tt as _tt
        storage, nc = C.c_uint64(), C.c_uint32()
        shape = np.zeros(8, dtype=np.uint32)
        ranks = np.zeros(9, dtype=np.uint32)
        _capi.check(self._lib.nmn_hnsw_tt_row(self._h, int(node), C.c_void_p(shape.ctypes.data), C.byref(nc),
                                              C.c_void_p(ranks.ctypes.data), None, 0, C.byref(storage)))
        if storage.value == 0xFFFFFFFFFFFFFFFF:
            return None
        cores = np.empty(storage.value, dtype=np.float32)
        _capi.check(self._lib.nmn_hnsw_tt_row(self._h, int(node), None, None, None, C.c_void_p(cores.ctypes.data), cores.size,
                                              C.byref(storage)))
        d = nc.value
        sh, rk = [int(x) for x in shape[:d]], [int(x) for x in ranks[:d + 1]]
        parts, at = [], 0
        for c in range(d):
            size = rk[c] * sh[c] * rk[c + 1]
            parts.append(cores[at:at + size].reshape(rk[c], sh[c], rk[c + 1]))
            at += size
        return _tt.TTVector(sh, rk, parts)

    def tt_walk_limits(self, ef=None):
        """-> (max_node_rank, nodes_above_limits, lds_floats): the limits of the device walk of TT queries on an index with
        TensorTrain nodes (nmn_hnsw_tt_walk_limits, docs/hnsw.md §24)"""
        r, n, f = C.c_uint32(), C.c_uint64(), C.c_uint32()
        _capi.check(self._lib.nmn_hnsw_tt_walk_limits(self._h, 0 if ef is None else int(ef), C.byref(r), C.byref(n), C.byref(f)))
        return r.value, n.value, f.value

    def search_tt_dense(self, queries, k, config, with_stats=False):
        """HNSWIndex::search_tt per query (nmn_hnsw_search_tt_dense): the query is decomposed under `config` (a
        neumann_amd.tt.TTConfig); an Ok train is answered as `search_tt` answers it (Cosine, ef_search), an Err of any kind as
        `search` answers the dense query under the index's metric (docs/hnsw.md §21).
        -> (ids u64 [nq,k], scores f32 [nq,k], counts u32 [nq])"""
        q = self._rows(queries)
        nq, k = q.shape[0], int(k)
        sh, r, tol = config._c()
        ids, sc, counts, st = _host_out(nq, k)
        _capi.check(self._lib.nmn_hnsw_search_tt_dense(self._h, C.c_void_p(q.ctypes.data), nq, q.shape[1], C.c_void_p(sh.ctypes.data),
                                                       sh.size, r, tol, k, C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data),
                                                       C.c_void_p(counts.ctypes.data), C.byref(st)))
        return (ids, sc, counts, st) if with_stats else (ids, sc, counts)

    def insert_tt_dense(self, vector, config):
        """HNSWIndex::insert_tt (nmn_hnsw_insert_tt_dense): the vector is decomposed under `config` to validate it and inserted
        as a Dense node by `insert`'s path; returns the node id.  Dense handles only."""
        v = np.ascontiguousarray(vector, dtype=np.float32).reshape(-1)
        sh, r, tol = config._c()
        out = C.c_uint64()
        _capi.check(self._lib.nmn_hnsw_insert_tt_dense(self._h, C.c_void_p(v.ctypes.data), v.size, C.c_void_p(sh.ctypes.data), sh.size,
                                                       r, tol, C.byref(out)))
        return int(out.value)

    def insert_batch_tt(self, vectors, config):
        """HNSWIndex::insert_batch_tt (nmn_hnsw_insert_batch_tt): every vector is decomposed under `config`; if any decomposition
        fails nothing is inserted and the error names the lowest failing index; returns the node ids (none for an empty batch)."""
        v = np.ascontiguousarray(vectors, dtype=np.float32)
        if v.size == 0:
            return np.empty(0, dtype=np.uint64)
        if v.ndim != 2:
            raise _capi.NeumannGpuError(_capi.ERR_INVALID_ARGUMENT, "vectors must be [n, dim]")
        sh, r, tol = config._c()
        ids = np.empty(v.shape[0], dtype=np.uint64)
        _capi.check(self._lib.nmn_hnsw_insert_batch_tt(self._h, C.c_void_p(v.ctypes.data), v.shape[0], v.shape[1],
                                                       C.c_void_p(sh.ctypes.data), sh.size, r, tol, C.c_void_p(ids.ctypes.data)))
        return ids

    def search_metric(self, queries, top_k, metric, with_stats=False):
        """search_with_hnsw_and_metric's steps per query (nmn_hnsw_search_metric): c = max(2 top_k, 10) candidates from the walk,
        re-ranked under `metric` (an ExtendedDistanceMetric), the first top_k of the stable descending order.
        -> (ids u64 [nq,top_k], scores f32 [nq,top_k], counts u32 [nq])"""
        q = self._rows(queries)
        nq, k = q.shape[0], int(top_k)
        ids, sc, counts, st = _host_out(nq, k)
        m = metric._c()
        _capi.check(self._lib.nmn_hnsw_search_metric(self._h, C.c_void_p(q.ctypes.data), nq, k, C.byref(m),
                                                     C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data),
                                                     C.c_void_p(counts.ctypes.data), C.byref(st)))
        return (ids, sc, counts, st) if with_stats else (ids, sc, counts)

    def search_metric_multi(self, queries, top_k, metrics, kstride=None, with_stats=False):
        """`search_metric` with a top_k and a metric per query in ONE call (nmn_hnsw_search_metric_multi).  `top_k`: one integer
        per query; `metrics`: one ExtendedDistanceMetric per query; `kstride`: row length of the outputs (None: max(top_k)).
        -> (ids u64 [nq,kstride], scores f32 [nq,kstride], counts u32 [nq]); row i is what search_metric(q_i, top_k[i],
        metrics[i]) answers."""
        q = self._rows(queries)
        nq = q.shape[0]
        metrics = list(metrics)
        kk, _, ks = _per_query(top_k, None, kstride, nq, "one top_k and one metric per query")
        if len(metrics) != nq:
            raise _capi.NeumannGpuError(_capi.ERR_INVALID_ARGUMENT, "one top_k and one metric per query")
        mm = (_capi.XMetric * max(nq, 1))(*[m._c() for m in metrics])
        ids, sc, counts, st = _host_out(nq, ks)
        _capi.check(self._lib.nmn_hnsw_search_metric_multi(self._h, C.c_void_p(q.ctypes.data), nq, C.c_void_p(kk.ctypes.data),
                                                           C.cast(mm, C.c_void_p), ks, C.c_void_p(ids.ctypes.data),
                                                           C.c_void_p(sc.ctypes.data), C.c_void_p(counts.ctypes.data), C.byref(st)))
        return (ids, sc, counts, st) if with_stats else (ids, sc, counts)

    def search_metric_device(self, queries_t, top_k, metric, out=None, stream=None):
        """`search_metric` with torch device tensors, in stream order (nmn_hnsw_search_metric_device); same conventions as
        `search_device`."""
        queries_t, nq, k = self._device_queries(queries_t, top_k)
        ids, sc, counts = _device_out(out, nq, k, queries_t.device)
        m = metric._c()
        _capi.check(self._lib.nmn_hnsw_search_metric_device(
            self._h, C.c_void_p(queries_t.data_ptr()), nq, k, C.byref(m), C.c_void_p(ids.data_ptr()), C.c_void_p(sc.data_ptr()),
            C.c_void_p(counts.data_ptr()), _stream_ptr(stream)))
        return ids, sc, counts

    def set_node_mask(self, nodes, live):
        """nmn_hnsw_set_node_mask: set (`live` true) or clear the live bits of `nodes`.  A new node is live; only `cache_search*`
        read the mask, and `save` does not store it."""
        nn = np.ascontiguousarray(nodes, dtype=np.uint64).reshape(-1)
        _capi.check(self._lib.nmn_hnsw_set_node_mask(self._h, C.c_void_p(nn.ctypes.data), nn.size, 1 if live else 0))

    def node_live(self, node):
        """the node's live bit (nmn_hnsw_node_live); None for a node the index does not hold"""
        r = int(self._lib.nmn_hnsw_node_live(self._h, int(node)))
        return None if r < 0 else bool(r)

    def cache_search(self, queries, k, threshold, metric, with_stats=False):
        """CacheIndex::search_with_metric's steps per query with node ids in place of keys (nmn_hnsw_cache_search; docs/hnsw.md
        §16): c = max(3k, 10) candidates from the walk, dead nodes dropped, every other re-scored under `metric` on its stored form
        (a Sparse node by its own entries), kept iff similarity >= threshold, the first k of the stable descending order.
        -> (ids u64 [nq,k], similarities f32 [nq,k], counts u32 [nq])"""
        q = self._rows(queries)
        nq, k = q.shape[0], int(k)
        ids, sc, counts, st = _host_out(nq, k)
        m = metric._c()
        _capi.check(self._lib.nmn_hnsw_cache_search(self._h, C.c_void_p(q.ctypes.data), nq, k, float(threshold), C.byref(m),
                                                    C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data),
                                                    C.c_void_p(counts.ctypes.data), C.byref(st)))
        return (ids, sc, counts, st) if with_stats else (ids, sc, counts)

    def cache_search_sparse(self, indptr, positions, values, k, threshold, metric, with_stats=False):
        """CacheIndex::search_sparse_with_metric per query (nmn_hnsw_cache_search_sparse): `cache_search` behind
        `search_sparse`'s walk, the query's own entries scored.  The CSR is `search_sparse`'s.
        -> (ids u64 [nq,k], similarities f32 [nq,k], counts u32 [nq])"""
        ip, pos, val = _csr(indptr, positions, values, "nq")
        nq, k = ip.size - 1, int(k)
        ids, sc, counts, st = _host_out(nq, k)
        m = metric._c()
        _capi.check(self._lib.nmn_hnsw_cache_search_sparse(self._h, C.c_void_p(ip.ctypes.data), C.c_void_p(pos.ctypes.data),
                                                           C.c_void_p(val.ctypes.data), nq, k, float(threshold), C.byref(m),
                                                           C.c_void_p(ids.ctypes.data), C.c_void_p(sc.ctypes.data),
                                                           C.c_void_p(counts.ctypes.data), C.byref(st)))
        return (ids, sc, counts, st) if with_stats else (ids, sc, counts)

    def cache_search_sparse_device(self, indptr_t, positions_t, values_t, k, threshold, metric, max_nnz=None, out=None, status=None,
                                   stream=None):
        """`cache_search_sparse` with torch device tensors as ONE stream-ordered chain (nmn_hnsw_cache_search_sparse_device): the
        CSR, `max_nnz`, the returned (ids, similarities, counts, status) and the statuses are `search_sparse_device`'s."""
        ip, pos, val, nq, nnz = _device_csr(indptr_t, positions_t, values_t)
        k = int(k)
        ids, sc, counts = _device_out(out, nq, k, ip.device)
        status = _device_status(status, nq, ip.device)
        m = metric._c()
        _capi.check(self._lib.nmn_hnsw_cache_search_sparse_device(
            self._h, C.c_void_p(ip.data_ptr()), C.c_void_p(pos.data_ptr()), C.c_void_p(val.data_ptr()), nq, nnz,
            0 if max_nnz is None else int(max_nnz), k, float(threshold), C.byref(m), C.c_void_p(ids.data_ptr()),
            C.c_void_p(sc.data_ptr()), C.c_void_p(counts.data_ptr()), C.c_void_p(status.data_ptr()), _stream_ptr(stream)))
        return ids, sc, counts, status

    def cache_search_device(self, queries_t, k, threshold, metric, out=None, stream=None):
        """`cache_search` with torch device tensors, in stream order (nmn_hnsw_cache_search_device); same conventions as
        `search_device`."""
        queries_t, nq, k = self._device_queries(queries_t, k)
        ids, sc, counts = _device_out(out, nq, k, queries_t.device)
        m = metric._c()
        _capi.check(self._lib.nmn_hnsw_cache_search_device(
            self._h, C.c_void_p(queries_t.data_ptr()), nq, k, float(threshold), C.byref(m), C.c_void_p(ids.data_ptr()),
            C.c_void_p(sc.data_ptr()), C.c_void_p(counts.data_ptr()), _stream_ptr(stream)))
        return ids, sc, counts
