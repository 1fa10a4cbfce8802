"""tensor_cache::CacheIndex on the GPU HNSW index — host wrapper of `nmn_cache_index_*` (include/neumann_cache.h).

The key maps of the semantic cache (tensor_cache/src/index.rs:30-451) on the host, every lookup one `nmn_hnsw_cache_search`: the walk
for max(3k, 10) candidates, nodes whose key is gone dropped, the others re-scored under an ExtendedDistanceMetric on their stored
form, the threshold, the stable order (docs/hnsw.md §16).  Every method may be called from many threads at once."""
import ctypes as C

import numpy as np

from . import _capi
from .hnsw import HNSWConfig
from .xmetric import ExtendedDistanceMetric, GeometricConfig


_vp, _u64p, _u32p = C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
# include/neumann_cache.h
SIGNATURES = {
    "nmn_cache_index_create": (C.c_int32, [C.c_uint32, C.POINTER(_capi.HnswConfig), C.POINTER(_capi.XMetric), C.c_int32, C.POINTER(_vp)]),
    "nmn_cache_index_destroy": (C.c_int32, [_vp]),
    "nmn_cache_index_last_error": (C.c_char_p, []),
    "nmn_cache_index_insert": (C.c_int32, [_vp, C.c_char_p, _vp, C.c_uint32, _u64p]),
    "nmn_cache_index_insert_sparse": (C.c_int32, [_vp, C.c_char_p, _vp, _vp, C.c_uint64, _u64p]),
    "nmn_cache_index_insert_auto": (C.c_int32, [_vp, C.c_char_p, _vp, C.c_uint32, C.c_float, _u64p]),
    "nmn_cache_index_search": (C.c_int32, [_vp, _vp, C.c_uint32, C.c_uint32, C.c_float, _vp, C.c_uint64, _u64p, _vp, _u32p]),
    "nmn_cache_index_search_with_metric": (C.c_int32, [_vp, _vp, C.c_uint32, C.c_uint32, C.c_float, C.POINTER(_capi.XMetric), _vp, C.c_uint64,
                                                       _u64p, _vp, _u32p]),
    "nmn_cache_index_search_sparse": (C.c_int32, [_vp, _vp, _vp, C.c_uint64, C.c_uint32, C.c_float, _vp, C.c_uint64, _u64p, _vp, _u32p]),
    "nmn_cache_index_search_sparse_with_metric": (C.c_int32, [_vp, _vp, _vp, C.c_uint64, C.c_uint32, C.c_float, C.POINTER(_capi.XMetric), _vp,
                                                              C.c_uint64, _u64p, _vp, _u32p]),
    "nmn_cache_index_remove": (C.c_int32, [_vp, C.c_char_p]),
    "nmn_cache_index_contains": (C.c_int32, [_vp, C.c_char_p]),
    "nmn_cache_index_len": (C.c_uint64, [_vp]),
    "nmn_cache_index_dimension": (C.c_uint32, [_vp]),
    "nmn_cache_index_metric": (C.c_int32, [_vp, C.POINTER(_capi.XMetric)]),
    "nmn_cache_index_keys": (C.c_int32, [_vp, _vp, C.c_uint64, _u64p, _u64p]),
    "nmn_cache_index_clear": (C.c_int32, [_vp]),
    "nmn_cache_index_memory_stats": (C.c_int32, [_vp, C.POINTER(_capi.HnswMemStats)]),
    "nmn_cache_index_get_embedding": (C.c_int32, [_vp, C.c_char_p, C.POINTER(C.c_int32), _vp, _vp, _vp, C.c_uint32, _u32p]),
    "nmn_cache_index_hnsw": (_vp, [_vp]),
}
_bound = False


def _load():
    """the shared library with the nmn_cache_index_* entries bound (a missing one is an error: header / library mismatch)"""
    global _bound
    lib = _capi.load()
    if not _bound:
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _bound = True
    return lib


def _check(lib, status):
    if status != _capi.OK:
        raise _capi.NeumannGpuError(status, lib.nmn_cache_index_last_error().decode(errors="replace"))


class CacheIndex:
    def __init__(self, dimension, config=None, metric=None, device=-1):
        """CacheIndex::with_metric: `config` an HNSWConfig (None: default), `metric` an ExtendedDistanceMetric (None: Cosine)"""
        self._lib = _load()
        self._c = None
        self.config = config or HNSWConfig()
        self._metric = metric or ExtendedDistanceMetric.Cosine
        cfg = self.config._c()
        m = self._metric._c()
        c = C.c_void_p()
        _check(self._lib, self._lib.nmn_cache_index_create(int(dimension), C.byref(cfg), C.byref(m), int(device), C.byref(c)))
        self._c = c

    def close(self):
        if getattr(self, "_c", None):
            self._lib.nmn_cache_index_destroy(self._c)
            self._c = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def dimension(self):
        return int(self._lib.nmn_cache_index_dimension(self._c))

    def metric(self):
        m = _capi.XMetric()
        _check(self._lib, self._lib.nmn_cache_index_metric(self._c, C.byref(m)))
        if m.kind == _capi.XMETRIC_COMPOSITE:
            return ExtendedDistanceMetric.Composite(GeometricConfig(m.cosine_weight, m.structural_weight, m.magnitude_weight))
        return ExtendedDistanceMetric(m.kind)

    def __len__(self):
        return int(self._lib.nmn_cache_index_len(self._c))

    def is_empty(self):
        return len(self) == 0

    def contains(self, key):
        return bool(self._lib.nmn_cache_index_contains(self._c, key.encode()))

    __contains__ = contains

    def insert(self, key, embedding):
        """-> the node id.  An existing key keeps its old node answering (index.rs:99-105) and does not grow len()."""
        v = np.ascontiguousarray(embedding, dtype=np.float32).reshape(-1)
        node = C.c_uint64()
        _check(self._lib, self._lib.nmn_cache_index_insert(self._c, key.encode(), C.c_void_p(v.ctypes.data), v.size, C.byref(node)))
        return int(node.value)

    def insert_sparse(self, key, positions, values):
        """(position, value) pairs in any order, made a SparseVector as try_from_parts does -> the node id"""
        pos = np.ascontiguousarray(positions, dtype=np.uint32).reshape(-1)
        val = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
        if pos.size != val.size:
            raise _capi.NeumannGpuError(_capi.ERR_INVALID_ARGUMENT, "positions and values of one length")
        node = C.c_uint64()
        _check(self._lib, self._lib.nmn_cache_index_insert_sparse(self._c, key.encode(), C.c_void_p(pos.ctypes.data),
                                                                  C.c_void_p(val.ctypes.data), pos.size, C.byref(node)))
        return int(node.value)

    def insert_auto(self, key, embedding, sparsity_threshold):
        """Sparse(from_dense(embedding)) iff its sparsity() >= sparsity_threshold (the caller's, in f32), Dense otherwise"""
        v = np.ascontiguousarray(embedding, dtype=np.float32).reshape(-1)
        node = C.c_uint64()
        _check(self._lib, self._lib.nmn_cache_index_insert_auto(self._c, key.encode(), C.c_void_p(v.ctypes.data), v.size,
                                                                float(sparsity_threshold), C.byref(node)))
        return int(node.value)

    def _lookup(self, call, k):
        k = int(k)
        if k > 0:
            k = min(k, max(self._nodes(), 1))   # no answer is longer than the index; the library writes at most k similarities
        sims = np.empty(max(k, 1), dtype=np.float32)
        cap = 4096
        while True:
            buf = C.create_string_buffer(cap)
            need, count = C.c_uint64(), C.c_uint32()
            st = call(k, buf, cap, C.byref(need), C.c_void_p(sims.ctypes.data), C.byref(count))
            if st == _capi.ERR_BUFFER_TOO_SMALL and need.value > cap:
                cap = int(need.value)
                continue
            _check(self._lib, st)
            keys = buf.raw[:need.value].split(b"\0")[:count.value]
            return [(key.decode(), np.float32(s)) for key, s in zip(keys, sims[:count.value])]

    def _nodes(self):
        return int(self._lib.nmn_hnsw_len(self._lib.nmn_cache_index_hnsw(self._c)))

    def search(self, query, k, threshold):
        """-> [(key, similarity f32)] best first, under the metric given at construction"""
        return self.search_with_metric(query, k, threshold, None)

    def search_with_metric(self, query, k, threshold, metric):
        q = np.ascontiguousarray(query, dtype=np.float32).reshape(-1)
        m = (metric or self._metric)._c()
        return self._lookup(lambda kk, buf, cap, need, sims, count: self._lib.nmn_cache_index_search_with_metric(
            self._c, C.c_void_p(q.ctypes.data), q.size, kk, float(threshold), C.byref(m), buf, cap, need, sims, count), k)

    def search_sparse(self, positions, values, k, threshold):
        return self.search_sparse_with_metric(positions, values, k, threshold, None)

    def search_sparse_with_metric(self, positions, values, k, threshold, metric):
        pos = np.ascontiguousarray(positions, dtype=np.uint32).reshape(-1)
        val = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
        if pos.size != val.size:
            raise _capi.NeumannGpuError(_capi.ERR_INVALID_ARGUMENT, "positions and values of one length")
        m = (metric or self._metric)._c()
        return self._lookup(lambda kk, buf, cap, need, sims, count: self._lib.nmn_cache_index_search_sparse_with_metric(
            self._c, C.c_void_p(pos.ctypes.data), C.c_void_p(val.ctypes.data), pos.size, kk, float(threshold), C.byref(m), buf, cap,
            need, sims, count), k)

    def remove(self, key):
        r = int(self._lib.nmn_cache_index_remove(self._c, key.encode()))
        if r < 0:   # the live mask could not follow: nothing was removed
            _check(self._lib, r)
        return bool(r)

    def clear(self):
        _check(self._lib, self._lib.nmn_cache_index_clear(self._c))

    def keys(self):
        cap = 1 << 16
        while True:
            buf = C.create_string_buffer(cap)
            need, n = C.c_uint64(), C.c_uint64()
            st = self._lib.nmn_cache_index_keys(self._c, buf, cap, C.byref(need), C.byref(n))
            if st == _capi.ERR_BUFFER_TOO_SMALL and need.value > cap:
                cap = int(need.value)
                continue
            _check(self._lib, st)
            return [k.decode() for k in buf.raw[:need.value].split(b"\0")[:n.value]]

    def memory_stats(self):
        st = _capi.HnswMemStats()
        _check(self._lib, self._lib.nmn_cache_index_memory_stats(self._c, C.byref(st)))
        return {n: int(getattr(st, n)) for n, _ in st._fields_}

    def get_embedding(self, key):
        """-> ("dense", row f32 [dim]) / ("sparse", (positions u32, values f32)) of the key's current node; None for an unknown key"""
        kind, nnz = C.c_int32(), C.c_uint32()
        dense = np.empty(self.dimension, dtype=np.float32)
        st = self._lib.nmn_cache_index_get_embedding(self._c, key.encode(), C.byref(kind), C.c_void_p(dense.ctypes.data), None, None, 0,
                                                     C.byref(nnz))
        if st == _capi.ERR_NOT_FOUND:
            return None
        _check(self._lib, st)
        if kind.value == 0:
            return "dense", dense
        pos = np.empty(nnz.value, dtype=np.uint32)
        val = np.empty(nnz.value, dtype=np.float32)
        _check(self._lib, self._lib.nmn_cache_index_get_embedding(self._c, key.encode(), None, None, C.c_void_p(pos.ctypes.data),
                                                                  C.c_void_p(val.ctypes.data), nnz.value, C.byref(nnz)))
        return "sparse", (pos, val)

    def coalesce_stats(self):
        """nmn_hnsw_coalesce_stats of the HNSW handle in use now"""
        b, c = C.c_uint64(), C.c_uint64()
        _capi.check(self._lib.nmn_hnsw_coalesce_stats(self._lib.nmn_cache_index_hnsw(self._c), C.byref(b), C.byref(c)))
        return int(b.value), int(c.value)
