"""IVF probe on the GPU — host wrapper of `nmn_ivf_*` (include/neumann_gpu.h).

Mirrors `tensor_store::ivf::IVFIndex` (tensor_store/src/ivf.rs:160-406) for the parts on the SIMILAR path: `add`
(nearest-centroid assignment) and `search` / `search_with_nprobe`, with `IVFStorage::Flat` (`GpuIvfFlat`),
`IVFStorage::PQ` (`GpuIvfPQ`) and `IVFStorage::Binary` (`GpuIvfBinary`).  `build` trains on the GPU exactly as the
reference's k-means does (`nmn_ivf_build` / `nmn_ivf_build_ex`); the plain constructors take centroids (and a PQ
codebook) trained elsewhere."""
import ctypes as C

import numpy as np

from . import _capi
from .flat_index import _stream_ptr


class GpuIvfFlat:
    def __init__(self, centroids, capacity_rows, nprobe=None, device=-1):
        self._lib = _capi.load()
        c = np.ascontiguousarray(centroids, dtype=np.float32)
        assert c.ndim == 2 and c.shape[0] >= 1
        self.n_clusters, self.dim = int(c.shape[0]), int(c.shape[1])
        # default_nprobe (ivf.rs:46-56): ceil(sqrt(num_clusters)) computed in f32
        self.nprobe = int(np.ceil(np.sqrt(np.float32(self.n_clusters)))) if nprobe is None else int(nprobe)
        desc = _capi.IndexDesc(dim=self.dim, flags=0, capacity_rows=int(capacity_rows), row_base=0, device=int(device),
                               cand_cap=0)
        h = C.c_void_p()
        _capi.check(self._lib.nmn_ivf_create(C.byref(desc), C.c_void_p(c.ctypes.data), self.n_clusters, C.byref(h)))
        self._h = h

    @classmethod
    def build(cls, rows, num_clusters, nprobe=None, max_iterations=100, convergence_threshold=1e-4, seed=42,
              init_method="kmeans++", capacity_rows=None, device=-1):
        """IVFIndex::train(rows) + add(every row) on the GPU (`nmn_ivf_build`): k-means exactly as the reference runs it."""
        self = cls.__new__(cls)
        self._lib = _capi.load()
        r = np.ascontiguousarray(rows, dtype=np.float32)
        n, self.dim = int(r.shape[0]), int(r.shape[1])
        desc = _capi.IndexDesc(dim=self.dim, flags=0, capacity_rows=int(capacity_rows or n), row_base=0, device=int(device),
                               cand_cap=0)
        opt = _capi.KMeansOptions(max_iterations=int(max_iterations), convergence_threshold=float(convergence_threshold),
                                  seed=int(seed), init_method=0 if init_method == "random" else 1)
        h = C.c_void_p()
        _capi.check(self._lib.nmn_ivf_build(C.byref(desc), C.c_void_p(r.ctypes.data), n, int(num_clusters), C.byref(opt),
                                            C.byref(h)))
        self._h = h
        self.n_clusters = int(self._lib.nmn_ivf_clusters(h))
        self.nprobe = int(np.ceil(np.sqrt(np.float32(num_clusters)))) if nprobe is None else int(nprobe)
        return self

    def save(self, path):
        """Centroids, the list of every vector and the vectors in id order -> `path` (nmn_ivf_save)."""
        _capi.check(self._lib.nmn_ivf_save(self._h, str(path).encode()))

    @classmethod
    def load(cls, path, nprobe=None, capacity_rows=0, device=-1, max_file_bytes=0, max_entries=0):
        """nmn_ivf_load: no k-means, no re-assignment — lists and centroids come back exactly as saved."""
        self = cls.__new__(cls)
        self._lib = _capi.load()
        desc = _capi.IndexDesc(dim=0, flags=0, capacity_rows=int(capacity_rows), row_base=0, device=int(device), cand_cap=0)
        h = C.c_void_p()
        _capi.check(self._lib.nmn_ivf_load(str(path).encode(), C.byref(desc), int(max_file_bytes), int(max_entries), C.byref(h)))
        self._h = h
        self.n_clusters = int(self._lib.nmn_ivf_clusters(h))
        self.dim = int(self._lib.nmn_index_dim(self._lib.nmn_ivf_vectors(h)))
        self.nprobe = int(np.ceil(np.sqrt(np.float32(self.n_clusters)))) if nprobe is None else int(nprobe)
        return self

    def centroids(self):
        out = np.empty((self.n_clusters, self.dim), dtype=np.float32)
        _capi.check(self._lib.nmn_ivf_centroids(self._h, C.c_void_p(out.ctypes.data), out.size))
        return out

    def close(self):
        if self._h:
            self._lib.nmn_ivf_destroy(self._h)
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

    @property
    def list_major_rows(self):
        """vectors covered by the list-major copy (0: every probe goes through the bitmap over the id-ordered rows)"""
        return int(self._lib.nmn_ivf_list_major_rows(self._h))

    def __len__(self):
        return int(self._lib.nmn_ivf_len(self._h))

    def add(self, rows):
        """IVFIndex::add for each row; returns the clusters chosen (ids are len-before .. len-after - 1)."""
        r = np.ascontiguousarray(rows, dtype=np.float32)
        if r.ndim == 1:
            r = r[None, :]
        assert r.shape[1] == self.dim
        out = np.empty(r.shape[0], dtype=np.uint32)
        _capi.check(self._lib.nmn_ivf_add(self._h, C.c_void_p(r.ctypes.data), r.shape[0], C.c_void_p(out.ctypes.data)))
        return out

    def cluster_sizes(self):
        out = np.zeros(self.n_clusters, dtype=np.uint64)
        _capi.check(self._lib.nmn_ivf_cluster_sizes(self._h, C.c_void_p(out.ctypes.data)))
        return out

    def search(self, queries, k, nprobe=None):
        """-> (ids u64 [nq,k], distances f32 [nq,k], counts u32 [nq]); IVFIndex::search_with_nprobe."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        assert q.shape[1] == self.dim
        nq, k = q.shape[0], int(k)
        ids = np.empty((nq, max(k, 1)), dtype=np.uint64)
        dist = np.empty((nq, max(k, 1)), dtype=np.float32)
        counts = np.empty(nq, dtype=np.uint32)
        _capi.check(self._lib.nmn_ivf_search(self._h, C.c_void_p(q.ctypes.data), nq, k,
                                             self.nprobe if nprobe is None else int(nprobe),
                                             C.c_void_p(ids.ctypes.data), C.c_void_p(dist.ctypes.data),
                                             C.c_void_p(counts.ctypes.data), None))
        return ids, dist, counts

    def search_device(self, queries_t, k, nprobe=None, out=None, stream=None):
        """`search` with torch device tensors, in stream order (nmn_ivf_search_device): enqueued on `stream` (None: torch's
        current stream), returns without waiting.  queries_t: [nq, dim] f32 on the index's device.  Returns (ids int64 [nq,k]
        holding the u64 bit pattern, -1 = unused slot; distances f32 [nq,k]; counts int32 [nq]), allocated on the queries'
        device unless `out` supplies them — the same answer `search` gives for the index as it is when the call returns."""
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
        if out is None:
            kk = max(k, 1)
            ids = torch.empty((nq, kk), dtype=torch.int64, device=queries_t.device)
            dist = torch.empty((nq, kk), dtype=torch.float32, device=queries_t.device)
            counts = torch.empty((nq,), dtype=torch.int32, device=queries_t.device)
        else:
            ids, dist, counts = out
        _capi.check(self._lib.nmn_ivf_search_device(
            self._h, C.c_void_p(queries_t.data_ptr()), nq, k, self.nprobe if nprobe is None else int(nprobe),
            C.c_void_p(ids.data_ptr()), C.c_void_p(dist.data_ptr()), C.c_void_p(counts.data_ptr()), _stream_ptr(stream)))
        return ids, dist, counts

    @property
    def hbm_bytes(self):
        """device memory the index holds right now (vectors or codes, centroids, codebook, search scratch)"""
        return int(self._lib.nmn_ivf_hbm_bytes(self._h))


def _kmeans_options(max_iterations=100, convergence_threshold=1e-4, seed=42, init_method="kmeans++"):
    return _capi.KMeansOptions(max_iterations=int(max_iterations), convergence_threshold=float(convergence_threshold),
                               seed=int(seed), init_method=0 if init_method == "random" else 1)


class _GpuIvfCoded(GpuIvfFlat):
    """An IVF index whose lists hold codes (nmn_ivf_create_ex / nmn_ivf_build_ex): no f32 vector on the device."""
    _KIND = None

    def _storage(self):
        raise NotImplementedError

    def _create(self, centroids, capacity_rows, nprobe, device, codebook=None, K=0):
        self._lib = _capi.load()
        c = np.ascontiguousarray(centroids, dtype=np.float32)
        assert c.ndim == 2 and c.shape[0] >= 1
        self.n_clusters, self.dim = int(c.shape[0]), int(c.shape[1])
        self.nprobe = int(np.ceil(np.sqrt(np.float32(self.n_clusters)))) if nprobe is None else int(nprobe)
        desc = _capi.IndexDesc(dim=self.dim, flags=0, capacity_rows=int(capacity_rows), row_base=0, device=int(device),
                               cand_cap=0)
        st = self._storage()
        cb = None if codebook is None else np.ascontiguousarray(codebook, dtype=np.float32)
        h = C.c_void_p()
        self._h = None
        _capi.check(self._lib.nmn_ivf_create_ex(C.byref(desc), C.c_void_p(c.ctypes.data), self.n_clusters, C.byref(st),
                                                None if cb is None or cb.size == 0 else C.c_void_p(cb.ctypes.data), int(K),
                                                C.byref(h)))
        self._h = h

    def _build(self, rows, num_clusters, nprobe, max_iterations, convergence_threshold, seed, init_method, capacity_rows,
               device):
        self._lib = _capi.load()
        self._h = None
        r = np.ascontiguousarray(rows, dtype=np.float32)
        n, self.dim = int(r.shape[0]), int(r.shape[1])
        desc = _capi.IndexDesc(dim=self.dim, flags=0, capacity_rows=int(capacity_rows or n), row_base=0, device=int(device),
                               cand_cap=0)
        opt = _kmeans_options(max_iterations, convergence_threshold, seed, init_method)
        st = self._storage()
        h = C.c_void_p()
        _capi.check(self._lib.nmn_ivf_build_ex(C.byref(desc), C.c_void_p(r.ctypes.data), n, int(num_clusters), C.byref(opt),
                                               C.byref(st), C.byref(h)))
        self._h = h
        self.n_clusters = int(self._lib.nmn_ivf_clusters(h))
        self.nprobe = int(np.ceil(np.sqrt(np.float32(num_clusters)))) if nprobe is None else int(nprobe)

    @classmethod
    def load(cls, *a, **kw):
        raise NotImplementedError("IVF-PQ / IVF-Binary indexes are not persisted (IVF-Flat only)")

    @property
    def storage_kind(self):
        return int(self._lib.nmn_ivf_storage_kind(self._h))

class GpuIvfPQ(_GpuIvfCoded):
    """IVFIndex with IVFStorage::PQ (ivf.rs:222-406, pq.rs:114-430): M bytes of codes per vector, residuals against the
    vector's list centroid, ADC distances sqrt(sum_m table[m][code_m])."""

    def __init__(self, centroids, codebook, capacity_rows, num_subspaces=8, nprobe=None, device=-1):
        """centroids C x dim and a codebook [M][K][dim / M] trained elsewhere (K = codebook.shape[1], may be 0)."""
        self.num_subspaces = int(num_subspaces)
        cb = np.asarray(codebook, dtype=np.float32)
        K = int(cb.shape[1]) if cb.ndim == 3 else 0
        self._create(centroids, capacity_rows, nprobe, device, codebook=cb, K=K)

    def _storage(self):
        s = _capi.IvfStorage()
        self._lib.nmn_ivf_storage_default(C.byref(s))
        s.kind = _capi.IVF_PQ
        s.pq_num_subspaces = self.num_subspaces
        s.pq_num_centroids = getattr(self, "_num_centroids", 256)
        if getattr(self, "_pq_kmeans", None) is not None:
            s.pq_kmeans = self._pq_kmeans
        return s

    @classmethod
    def build(cls, rows, num_clusters, num_subspaces=8, num_centroids=256, pq_kmeans=None, nprobe=None, max_iterations=100,
              convergence_threshold=1e-4, seed=42, init_method="kmeans++", capacity_rows=None, device=-1):
        """IVFIndex::train + add for IVFStorage::PQ on the GPU; pq_kmeans: dict of KMeansConfig fields for the codebook
        (default KMeansConfig::default), separate from the IVF k-means arguments."""
        self = cls.__new__(cls)
        self._lib = _capi.load()
        self.num_subspaces, self._num_centroids = int(num_subspaces), int(num_centroids)
        self._pq_kmeans = _kmeans_options(**(pq_kmeans or {}))
        self._build(rows, num_clusters, nprobe, max_iterations, convergence_threshold, seed, init_method, capacity_rows, device)
        return self

    @property
    def num_codewords(self):
        """K' = min(num_centroids, training rows) codewords per subspace"""
        return int(self._lib.nmn_ivf_pq_codewords(self._h))

    def codebook(self):
        """[M][K'][dim / M] f32"""
        K = self.num_codewords
        out = np.empty((self.num_subspaces, K, self.dim // self.num_subspaces), dtype=np.float32)
        _capi.check(self._lib.nmn_ivf_pq_codebook(self._h, C.c_void_p(out.ctypes.data), out.size))
        return out

    def codes(self):
        """u8 [len][M] in id order"""
        out = np.empty((len(self), self.num_subspaces), dtype=np.uint8)
        _capi.check(self._lib.nmn_ivf_codes(self._h, C.c_void_p(out.ctypes.data), out.nbytes))
        return out


class GpuIvfBinary(_GpuIvfCoded):
    """IVFIndex with IVFStorage::Binary (ivf.rs:305-309, 356-401; binary_quantization.rs:27-155): ceil(dim / 64) u64
    words per vector, distance hamming / dim."""

    def __init__(self, centroids, capacity_rows, threshold="sign", nprobe=None, device=-1):
        from .engine import BinaryThreshold
        self.threshold = threshold
        self._tcode = BinaryThreshold.code(threshold)
        self._create(centroids, capacity_rows, nprobe, device)

    def _storage(self):
        s = _capi.IvfStorage()
        self._lib.nmn_ivf_storage_default(C.byref(s))
        s.kind = _capi.IVF_BINARY
        s.binary_threshold = self._tcode
        return s

    @classmethod
    def build(cls, rows, num_clusters, threshold="sign", nprobe=None, max_iterations=100, convergence_threshold=1e-4, seed=42,
              init_method="kmeans++", capacity_rows=None, device=-1):
        from .engine import BinaryThreshold
        self = cls.__new__(cls)
        self._lib = _capi.load()
        self.threshold, self._tcode = threshold, BinaryThreshold.code(threshold)
        self._build(rows, num_clusters, nprobe, max_iterations, convergence_threshold, seed, init_method, capacity_rows, device)
        return self

    def codes(self):
        """u64 [len][ceil(dim / 64)] in id order"""
        out = np.empty((len(self), (self.dim + 63) // 64), dtype=np.uint64)
        _capi.check(self._lib.nmn_ivf_codes(self._h, C.c_void_p(out.ctypes.data), out.nbytes))
        return out
