//! Safe wrappers over `ffi` (integration/rust/ffi.rs) for the reference's crate `vector_engine`:
//! `GpuFlatIndex` = one row-range shard on one GPU, `GpuShardedIndex` = one logical index over several GPUs of a node.
//! Written against the reference's own types (`DistanceMetric`, `VectorError`, `Result`, lib.rs:148-260); this image has
//! no Rust toolchain, so the file is not compiled here — the C ABI it calls is exercised by tests/ through ctypes and by
//! nmn_engine.cpp and the nmn_engine_*.cpp files beside it.
#![allow(unsafe_code)]
use std::ffi::{CStr, CString};
use std::path::Path;

use crate::ffi;
use crate::{DistanceMetric, Result, VectorError};

fn last_error() -> String {
    // thread-local in the library: the message of this thread's most recent failing call
    unsafe { CStr::from_ptr(ffi::nmn_last_error()) }.to_string_lossy().into_owned()
}

/// Status codes are the `VectorError` variants (include/neumann_gpu.h:32-50; lib.rs:148-200).
fn check(st: ffi::nmn_status, expected_dim: usize, got_dim: usize) -> Result<()> {
    match st {
        ffi::NMN_OK => Ok(()),
        ffi::NMN_ERR_DIMENSION_MISMATCH => Err(VectorError::DimensionMismatch { expected: expected_dim, got: got_dim }),
        ffi::NMN_ERR_EMPTY_VECTOR => Err(VectorError::EmptyVector),
        ffi::NMN_ERR_INVALID_TOP_K => Err(VectorError::InvalidTopK),
        ffi::NMN_ERR_CONFIGURATION => Err(VectorError::ConfigurationError(last_error())),
        ffi::NMN_ERR_IO => Err(VectorError::IoError(last_error())),
        ffi::NMN_ERR_SERIALIZATION => Err(VectorError::SerializationError(last_error())),
        _ => Err(VectorError::StorageError(last_error())),
    }
}

impl From<DistanceMetric> for ffi::nmn_metric {
    fn from(m: DistanceMetric) -> Self {
        match m {
            DistanceMetric::Cosine => ffi::nmn_metric::NMN_METRIC_COSINE,
            DistanceMetric::Euclidean => ffi::nmn_metric::NMN_METRIC_EUCLIDEAN,
            DistanceMetric::DotProduct => ffi::nmn_metric::NMN_METRIC_DOT_PRODUCT,
        }
    }
}

/// `tensor_store::DistanceMetric` (the crate's `ExtendedDistanceMetric`, tensor_store/src/distance.rs:13-52) as the library takes it.
impl From<&crate::ExtendedDistanceMetric> for ffi::nmn_xmetric {
    fn from(m: &crate::ExtendedDistanceMetric) -> Self {
        use crate::ExtendedDistanceMetric as M;
        let unit = |kind| ffi::nmn_xmetric { kind, cosine_weight: 0.0, structural_weight: 0.0, magnitude_weight: 0.0 };
        match m {
            M::Cosine => unit(ffi::NMN_XMETRIC_COSINE),
            M::Angular => unit(ffi::NMN_XMETRIC_ANGULAR),
            M::Geodesic => unit(ffi::NMN_XMETRIC_GEODESIC),
            M::Jaccard => unit(ffi::NMN_XMETRIC_JACCARD),
            M::Overlap => unit(ffi::NMN_XMETRIC_OVERLAP),
            M::WeightedJaccard => unit(ffi::NMN_XMETRIC_WEIGHTED_JACCARD),
            M::Euclidean => unit(ffi::NMN_XMETRIC_EUCLIDEAN),
            M::Manhattan => unit(ffi::NMN_XMETRIC_MANHATTAN),
            M::Composite(c) => ffi::nmn_xmetric {
                kind: ffi::NMN_XMETRIC_COMPOSITE,
                cosine_weight: c.cosine_weight,
                structural_weight: c.structural_weight,
                magnitude_weight: c.magnitude_weight,
            },
        }
    }
}

fn c_path(p: &Path) -> Result<CString> {
    CString::new(p.to_string_lossy().as_bytes()).map_err(|e| VectorError::IoError(e.to_string()))
}

pub struct GpuFlatIndex {
    raw: *mut ffi::nmn_index,
    dim: usize,
}
// One handle may be searched from any number of threads: callers that arrive while the shard is busy are queued and run
// together as ONE query batch (nmn_index_coalesce_stats); each gets exactly what it gets alone.  Writers drain the queue.
unsafe impl Send for GpuFlatIndex {}
unsafe impl Sync for GpuFlatIndex {}

impl GpuFlatIndex {
    /// `rows`: row-major n x dim, the vectors of the keys in `HnswCacheEntry` order (lib.rs:98).
    pub fn build(dim: usize, rows: &[f32], device: i32) -> Result<Self> {
        if dim == 0 {
            return Err(VectorError::EmptyVector);
        }
        let n = (rows.len() / dim) as u64;
        let desc = ffi::nmn_index_desc {
            dim: u32::try_from(dim).map_err(|_| VectorError::ConfigurationError("dimension exceeds u32".into()))?,
            flags: 0,
            capacity_rows: n + n / 4 + 1024, // spare rows for appends (Mirror in nmn_engine_internal.h; get_mirror in nmn_engine_mirror.cpp)
            row_base: 0,
            device,
            cand_cap: 0,
        };
        let mut raw = std::ptr::null_mut();
        check(unsafe { ffi::nmn_index_create(&desc, &mut raw) }, dim, dim)?;
        let idx = Self { raw, dim };
        check(unsafe { ffi::nmn_index_upload(idx.raw, rows.as_ptr(), 0, n) }, dim, dim)?;
        Ok(idx)
    }

    pub fn len(&self) -> usize {
        unsafe { ffi::nmn_index_rows(self.raw) as usize }
    }

    /// Device memory the shard holds: (f32 rows, mirrors that exist right now, per-row factors), in bytes.  A shard keeps the
    /// f32 rows plus ONE approximate copy by default (int8 codes where the row stride is a multiple of 128 elements: 5 bytes per
    /// element in all); what `VectorEngine::gpu_memory_usage()` would sum over its `gpu_cache`.
    pub fn hbm_bytes(&self) -> (u64, u64, u64) {
        let (mut a, mut b, mut c) = (0u64, 0u64, 0u64);
        unsafe { ffi::nmn_index_hbm_bytes(self.raw, &mut a, &mut b, &mut c) };
        (a, b, c)
    }

    /// Same shape as `HNSWIndex::search` (tensor_store/src/hnsw.rs:2055): (row, score), best first; ties by row id.
    /// `mask`: bit i of word i/64 = row i takes part (pre-filter bitmap, the `live` bitmap of lazy deletes, or both ANDed).
    pub fn search(&self, q: &[f32], k: usize, metric: DistanceMetric, mask: Option<&[u64]>) -> Result<Vec<(usize, f32)>> {
        if q.len() != self.dim {
            return Err(VectorError::DimensionMismatch { expected: self.dim, got: q.len() });
        }
        let mut rows = vec![u64::MAX; k];
        let mut scores = vec![f32::NEG_INFINITY; k];
        let mut n = 0u32;
        let st = unsafe {
            ffi::nmn_index_search(
                self.raw, q.as_ptr(), 1, k as u32, metric.into(), mask.map_or(std::ptr::null(), |m| m.as_ptr()),
                rows.as_mut_ptr(), scores.as_mut_ptr(), &mut n, std::ptr::null_mut(),
            )
        };
        check(st, self.dim, q.len())?;
        Ok(rows.into_iter().zip(scores).take(n as usize).map(|(r, s)| (r as usize, s)).collect())
    }

    /// `nq` queries in one sweep of the shard (row-major nq x dim); result lists in query order.
    pub fn search_batch(&self, queries: &[f32], k: usize, metric: DistanceMetric) -> Result<Vec<Vec<(usize, f32)>>> {
        let nq = queries.len() / self.dim;
        let mut rows = vec![u64::MAX; nq * k];
        let mut scores = vec![f32::NEG_INFINITY; nq * k];
        let mut counts = vec![0u32; nq];
        let st = unsafe {
            ffi::nmn_index_search(
                self.raw, queries.as_ptr(), nq as u32, k as u32, metric.into(), std::ptr::null(), rows.as_mut_ptr(),
                scores.as_mut_ptr(), counts.as_mut_ptr(), std::ptr::null_mut(),
            )
        };
        check(st, self.dim, self.dim)?;
        Ok((0..nq)
            .map(|i| (0..counts[i] as usize).map(|j| (rows[i * k + j] as usize, scores[i * k + j])).collect())
            .collect())
    }

    /// The re-rank of `search_with_hnsw_and_metric` (lib.rs:2588-2601) for candidates that are rows of this shard:
    /// `metric.to_similarity(metric.compute(from_dense(q), from_dense(row)))` per row, on the GPU (nmn_index_score_rows_xmetric).
    /// The caller sorts (stable, descending) and truncates, as lib.rs:2611-2617 does.
    pub fn score_rows_extended(&self, q: &[f32], rows: &[u64], metric: &crate::ExtendedDistanceMetric) -> Result<Vec<f32>> {
        if q.len() != self.dim {
            return Err(VectorError::DimensionMismatch { expected: self.dim, got: q.len() });
        }
        let m: ffi::nmn_xmetric = metric.into();
        let mut sim = vec![0f32; rows.len()];
        let st = unsafe {
            ffi::nmn_index_score_rows_xmetric(
                self.raw, q.as_ptr(), 1, &m, rows.as_ptr(), rows.len() as u32, std::ptr::null_mut(), sim.as_mut_ptr(),
            )
        };
        check(st, self.dim, q.len())?;
        Ok(sim)
    }

    /// Overwrite (or append at `len()`) one row: `store_embedding` keeps the mirror current instead of dropping it.
    pub fn set_row(&self, row: usize, v: &[f32]) -> Result<()> {
        if v.len() != self.dim {
            return Err(VectorError::DimensionMismatch { expected: self.dim, got: v.len() });
        }
        check(unsafe { ffi::nmn_index_set_row(self.raw, row as u64, v.as_ptr()) }, self.dim, v.len())
    }

    /// Device-layout snapshot (nmn_index_save): rows + magnitudes, checksummed; loads without re-deriving anything.
    pub fn save(&self, path: &Path) -> Result<()> {
        let p = c_path(path)?;
        check(unsafe { ffi::nmn_index_save(self.raw, p.as_ptr()) }, self.dim, self.dim)
    }

    /// `max_file_bytes` / `max_entries`: VectorEngineConfig::max_index_file_bytes / max_index_entries (lib.rs:644-646);
    /// 0 = no limit.  Exceeding either is a ConfigurationError with the reference's message.
    pub fn load(path: &Path, device: i32, max_file_bytes: u64, max_entries: u64) -> Result<Self> {
        let p = c_path(path)?;
        let ov = ffi::nmn_index_desc { dim: 0, flags: 0, capacity_rows: 0, row_base: 0, device, cand_cap: 0 };
        let mut raw = std::ptr::null_mut();
        check(unsafe { ffi::nmn_index_load(p.as_ptr(), &ov, max_file_bytes, max_entries, &mut raw) }, 0, 0)?;
        let dim = unsafe { ffi::nmn_index_dim(raw) } as usize;
        Ok(Self { raw, dim })
    }
}

impl Drop for GpuFlatIndex {
    fn drop(&mut self) {
        unsafe { ffi::nmn_index_destroy(self.raw) };
    }
}

/// One logical index over the GPUs of a node (nmn_sharded_*): rows are split into equal contiguous ranges, every search
/// runs on all shards at once, the per-shard top-k blocks are gathered (RCCL all-gather over xGMI, or peer copies) and
/// merged on one device with ResultMerger's rule (query_router/src/distributed.rs:413-433: score desc, ties by row id).
pub struct GpuShardedIndex {
    raw: *mut ffi::nmn_sharded,
    dim: usize,
}
unsafe impl Send for GpuShardedIndex {}
unsafe impl Sync for GpuShardedIndex {}

impl GpuShardedIndex {
    pub fn build(dim: usize, rows: &[f32], devices: &[i32]) -> Result<Self> {
        let n = (rows.len() / dim.max(1)) as u64;
        let desc = ffi::nmn_sharded_desc {
            dim: dim as u32,
            flags: 0,
            capacity_rows: n,
            row_base: 0,
            n_shards: devices.len() as u32,
            gather: ffi::NMN_GATHER_AUTO,
            devices: devices.as_ptr(),
            cand_cap: 0,
            layout: ffi::NMN_SHARDED_LAYOUT_RANGES,
        };
        let mut raw = std::ptr::null_mut();
        check(unsafe { ffi::nmn_sharded_create(&desc, &mut raw) }, dim, dim)?;
        let s = Self { raw, dim };
        check(unsafe { ffi::nmn_sharded_upload(s.raw, rows.as_ptr(), 0, n) }, dim, dim)?;
        Ok(s)
    }

    pub fn search(&self, q: &[f32], k: usize, metric: DistanceMetric, mask: Option<&[u64]>) -> Result<Vec<(usize, f32)>> {
        if q.len() != self.dim {
            return Err(VectorError::DimensionMismatch { expected: self.dim, got: q.len() });
        }
        let mut rows = vec![u64::MAX; k];
        let mut scores = vec![f32::NEG_INFINITY; k];
        let mut n = 0u32;
        let st = unsafe {
            ffi::nmn_sharded_search(
                self.raw, q.as_ptr(), 1, k as u32, metric.into(), mask.map_or(std::ptr::null(), |m| m.as_ptr()),
                rows.as_mut_ptr(), scores.as_mut_ptr(), &mut n, std::ptr::null_mut(),
            )
        };
        check(st, self.dim, q.len())?;
        Ok(rows.into_iter().zip(scores).take(n as usize).map(|(r, s)| (r as usize, s)).collect())
    }
}

impl Drop for GpuShardedIndex {
    fn drop(&mut self) {
        unsafe { ffi::nmn_sharded_destroy(self.raw) };
    }
}

/// `tensor_store::HNSWIndex` built on the host in the reference's order and searched on the GPU (nmn_hnsw_*), with the one thing
/// the reference's index lacks: it can be saved and loaded (docs/hnsw.md §10), so the sequential build is paid once.
pub struct GpuHnswIndex {
    raw: *mut ffi::nmn_hnsw,
    dim: usize,
}
unsafe impl Send for GpuHnswIndex {}
unsafe impl Sync for GpuHnswIndex {}

impl GpuHnswIndex {
    pub fn with_config(dim: usize, cfg: &ffi::nmn_hnsw_config, storage: i32, capacity_hint: usize, device: i32) -> Result<Self> {
        let mut raw = std::ptr::null_mut();
        let st = unsafe { ffi::nmn_hnsw_create_with_storage(cfg, storage, dim as u32, capacity_hint as u64, device, &mut raw) };
        check(st, dim, dim)?;
        Ok(Self { raw, dim })
    }

    /// An index whose every node is EmbeddingStorage::Binary(BinaryVector::from_dense(row, threshold)) (nmn_hnsw_create_binary,
    /// docs/hnsw.md §18): `threshold` is ffi::NMN_BINARY_SIGN / _MEAN / _MEDIAN.  `insert` and `search` work as on every handle;
    /// sparse, TT, metric and cache searches, the node mask and `save` are refused with a configuration error.
    pub fn new_binary(dim: usize, cfg: &ffi::nmn_hnsw_config, threshold: i32, capacity_hint: usize, device: i32) -> Result<Self> {
        let mut raw = std::ptr::null_mut();
        let st = unsafe { ffi::nmn_hnsw_create_binary(cfg, threshold, dim as u32, capacity_hint as u64, device, &mut raw) };
        check(st, dim, dim)?;
        Ok(Self { raw, dim })
    }

    /// The BinaryVector words of a node of a binary index (nmn_hnsw_binary_row): ceil(dim / 64) of them, padding bits zero.
    pub fn binary_row(&self, node: usize) -> Result<Vec<u64>> {
        let mut words = vec![0u64; self.dim.div_ceil(64)];
        let st = unsafe { ffi::nmn_hnsw_binary_row(self.raw, node as u64, words.as_mut_ptr(), words.len() as u32) };
        check(st, self.dim, self.dim)?;
        Ok(words)
    }

    pub fn len(&self) -> usize {
        unsafe { ffi::nmn_hnsw_len(self.raw) as usize }
    }

    /// HNSWIndex::insert for every row in order; the node ids are len() .. len() + n.
    pub fn insert(&self, rows: &[f32]) -> Result<()> {
        let n = (rows.len() / self.dim.max(1)) as u64;
        check(unsafe { ffi::nmn_hnsw_insert(self.raw, rows.as_ptr(), n, std::ptr::null_mut()) }, self.dim, self.dim)
    }

    /// HNSWIndex::insert_sparse for every vector in order (nmn_hnsw_insert_sparse): vector i is the (position, value) pairs
    /// `rows[i]`, in any order, made a SparseVector as try_from_parts makes it.  The node is stored Sparse and scored by
    /// SparseVector's own arithmetic (docs/hnsw.md §15).  Dense handles only.
    pub fn insert_sparse(&self, rows: &[Vec<(u32, f32)>]) -> Result<()> {
        let mut indptr = Vec::with_capacity(rows.len() + 1);
        let mut positions = Vec::new();
        let mut values = Vec::new();
        indptr.push(0u64);
        for r in rows {
            for &(p, v) in r {
                positions.push(p);
                values.push(v);
            }
            indptr.push(positions.len() as u64);
        }
        let st = unsafe {
            ffi::nmn_hnsw_insert_sparse(self.raw, indptr.as_ptr(), positions.as_ptr(), values.as_ptr(), rows.len() as u64, std::ptr::null_mut())
        };
        check(st, self.dim, self.dim)
    }

    /// HNSWIndex::insert_auto for every row in order (nmn_hnsw_insert_auto): Sparse(from_dense(row)) where the share of zeros
    /// reaches the config's sparsity_threshold, Dense otherwise.
    pub fn insert_auto(&self, rows: &[f32]) -> Result<()> {
        let n = (rows.len() / self.dim.max(1)) as u64;
        check(unsafe { ffi::nmn_hnsw_insert_auto(self.raw, rows.as_ptr(), n, std::ptr::null_mut()) }, self.dim, self.dim)
    }

    /// The stored (position, value) entries of a Sparse node, None for a Dense one (nmn_hnsw_sparse_row).
    pub fn sparse_row(&self, node: usize) -> Result<Option<Vec<(u32, f32)>>> {
        let mut nnz = 0u32;
        let st = unsafe { ffi::nmn_hnsw_sparse_row(self.raw, node as u64, std::ptr::null_mut(), std::ptr::null_mut(), 0, &mut nnz) };
        check(st, self.dim, self.dim)?;
        if nnz == u32::MAX {
            return Ok(None);
        }
        let mut positions = vec![0u32; nnz as usize];
        let mut values = vec![0f32; nnz as usize];
        let st = unsafe { ffi::nmn_hnsw_sparse_row(self.raw, node as u64, positions.as_mut_ptr(), values.as_mut_ptr(), nnz, &mut nnz) };
        check(st, self.dim, self.dim)?;
        Ok(Some(positions.into_iter().zip(values).collect()))
    }

    /// HNSWIndex::search: (node id, to_similarity(distance)), best first.
    pub fn search(&self, q: &[f32], k: usize) -> Result<Vec<(usize, f32)>> {
        if q.len() != self.dim {
            return Err(VectorError::DimensionMismatch { expected: self.dim, got: q.len() });
        }
        let mut ids = vec![u64::MAX; k];
        let mut scores = vec![f32::NEG_INFINITY; k];
        let mut n = 0u32;
        let st = unsafe {
            ffi::nmn_hnsw_search(self.raw, q.as_ptr(), 1, k as u32, 0, ids.as_mut_ptr(), scores.as_mut_ptr(), &mut n, std::ptr::null_mut())
        };
        check(st, self.dim, q.len())?;
        Ok(ids.into_iter().zip(scores).take(n as usize).map(|(r, s)| (r as usize, s)).collect())
    }

    /// One TTVector as the C entries take it: (shape, ranks, every core's data back to back) of `tensor_compress::TTVector`.
    fn tt_parts(tt: &tensor_compress::TTVector) -> (Vec<u32>, Vec<u32>, Vec<f32>) {
        let shape: Vec<u32> = tt.shape.iter().map(|&n| n as u32).collect();
        let mut ranks = vec![1u32];
        let mut cores = Vec::new();
        for c in &tt.cores {
            ranks.push(c.shape.2 as u32);
            cores.extend_from_slice(&c.data);
        }
        (shape, ranks, cores)
    }

    /// HNSWIndex::search_tt_with_ef (nmn_hnsw_search_tt; ef 0 = ef_search): the train is reconstructed and its norm taken on the
    /// GPU, the walk scores under Cosine whatever the index's metric is (docs/hnsw.md §17).  (node id, 1 - distance), best first.
    pub fn search_tt(&self, tt: &tensor_compress::TTVector, k: usize, ef: usize) -> Result<Vec<(usize, f32)>> {
        let (shape, ranks, cores) = Self::tt_parts(tt);
        let off = [0u64, cores.len() as u64];
        let mut ids = vec![u64::MAX; k];
        let mut scores = vec![f32::NEG_INFINITY; k];
        let mut n = 0u32;
        let st = unsafe {
            ffi::nmn_hnsw_search_tt(self.raw, shape.as_ptr(), shape.len() as u32, ranks.as_ptr(), off.as_ptr(), cores.as_ptr(), 1, k as u32,
                                    ef as u32, ids.as_mut_ptr(), scores.as_mut_ptr(), &mut n, std::ptr::null_mut())
        };
        check(st, self.dim, shape.iter().map(|&x| x as usize).product())?;
        Ok(ids.into_iter().zip(scores).take(n as usize).map(|(r, s)| (r as usize, s)).collect())
    }

    /// HNSWIndex::insert_tt_vector (nmn_hnsw_insert_tt): reconstructed on the GPU, inserted as a Dense node.
    pub fn insert_tt(&self, tt: &tensor_compress::TTVector) -> Result<()> {
        let (shape, ranks, cores) = Self::tt_parts(tt);
        let off = [0u64, cores.len() as u64];
        let st = unsafe {
            ffi::nmn_hnsw_insert_tt(self.raw, shape.as_ptr(), shape.len() as u32, ranks.as_ptr(), off.as_ptr(), cores.as_ptr(), 1, std::ptr::null_mut())
        };
        check(st, self.dim, shape.iter().map(|&x| x as usize).product())
    }

    /// HNSWIndex::insert_embedding(EmbeddingStorage::from(tt)) (nmn_hnsw_insert_embedding_tt): a TensorTrain node, which keeps the
    /// train and its cached tt_norm and is scored by its own rules (docs/hnsw.md §24) — not the Dense node `insert_tt` makes.
    /// Returns the node id.
    pub fn insert_embedding_tt(&self, tt: &tensor_compress::TTVector) -> Result<usize> {
        let (shape, ranks, cores) = Self::tt_parts(tt);
        let off = [0u64, cores.len() as u64];
        let mut id = u64::MAX;
        let st = unsafe {
            ffi::nmn_hnsw_insert_embedding_tt(self.raw, shape.as_ptr(), shape.len() as u32, ranks.as_ptr(), off.as_ptr(), cores.as_ptr(), 1, &mut id)
        };
        check(st, self.dim, shape.iter().map(|&x| x as usize).product())?;
        Ok(id as usize)
    }

    /// `search` for several queries in ONE launch, each with its own k and ef (nmn_hnsw_search_multi; ef 0 = ef_search).  Answer i is
    /// bit for bit what `search_with_ef(q_i, k_i, ef_i)` returns alone.  Concurrent callers of `search` / `search_multi` are
    /// coalesced into such launches by the library (docs/hnsw.md §11).
    pub fn search_multi(&self, queries: &[&[f32]], k: &[u32], ef: &[u32]) -> Result<Vec<Vec<(usize, f32)>>> {
        let nq = queries.len();
        if k.len() != nq || ef.len() != nq {
            return Err(VectorError::ConfigurationError("one k and one ef per query".to_string()));
        }
        let mut flat = Vec::with_capacity(nq * self.dim);
        for q in queries {
            if q.len() != self.dim {
                return Err(VectorError::DimensionMismatch { expected: self.dim, got: q.len() });
            }
            flat.extend_from_slice(q);
        }
        let kstride = k.iter().copied().max().unwrap_or(1).max(1) as usize;
        let mut ids = vec![u64::MAX; nq * kstride];
        let mut scores = vec![f32::NEG_INFINITY; nq * kstride];
        let mut counts = vec![0u32; nq];
        let st = unsafe {
            ffi::nmn_hnsw_search_multi(self.raw, flat.as_ptr(), nq as u32, k.as_ptr(), ef.as_ptr(), kstride as u32, ids.as_mut_ptr(),
                                       scores.as_mut_ptr(), counts.as_mut_ptr(), std::ptr::null_mut())
        };
        check(st, self.dim, self.dim)?;
        Ok((0..nq)
            .map(|i| (0..counts[i] as usize).map(|j| (ids[i * kstride + j] as usize, scores[i * kstride + j])).collect())
            .collect())
    }

    /// `HNSWIndex::search_sparse_with_ef` for several sparse queries in ONE launch, each with its own k and ef
    /// (nmn_hnsw_search_sparse_multi; ef 0 = ef_search).  Query i is the (position, value) pairs `queries[i]`, in any order, made a
    /// SparseVector of the index's dimension as `try_from_parts` does; a position out of bounds is refused before anything runs.
    /// Answer i is bit for bit what `search_sparse_with_ef(q_i, k_i, ef_i)` returns alone.  Concurrent sparse callers ride the
    /// coalescer's launches with every other host caller (docs/hnsw.md §14).
    pub fn search_sparse_multi(&self, queries: &[&[(u32, f32)]], k: &[u32], ef: &[u32]) -> Result<Vec<Vec<(usize, f32)>>> {
        let nq = queries.len();
        if k.len() != nq || ef.len() != nq {
            return Err(VectorError::ConfigurationError("one k and one ef per query".to_string()));
        }
        let mut indptr = Vec::with_capacity(nq + 1);
        let (mut positions, mut values) = (Vec::new(), Vec::new());
        indptr.push(0u64);
        for q in queries {
            for &(p, v) in q.iter() {
                positions.push(p);
                values.push(v);
            }
            indptr.push(positions.len() as u64);
        }
        let kstride = k.iter().copied().max().unwrap_or(1).max(1) as usize;
        let mut ids = vec![u64::MAX; nq * kstride];
        let mut scores = vec![f32::NEG_INFINITY; nq * kstride];
        let mut counts = vec![0u32; nq];
        let st = unsafe {
            ffi::nmn_hnsw_search_sparse_multi(self.raw, indptr.as_ptr(), positions.as_ptr(), values.as_ptr(), nq as u32, k.as_ptr(),
                                              ef.as_ptr(), kstride as u32, ids.as_mut_ptr(), scores.as_mut_ptr(), counts.as_mut_ptr(),
                                              std::ptr::null_mut())
        };
        check(st, self.dim, self.dim)?;
        Ok((0..nq)
            .map(|i| (0..counts[i] as usize).map(|j| (ids[i * kstride + j] as usize, scores[i * kstride + j])).collect())
            .collect())
    }

    /// Sets (`live`) or clears the live bits of `nodes` (nmn_hnsw_set_node_mask).  Only `cache_search*` read the mask.
    pub fn set_node_mask(&self, nodes: &[u64], live: bool) -> Result<()> {
        let st = unsafe { ffi::nmn_hnsw_set_node_mask(self.raw, nodes.as_ptr(), nodes.len() as u64, live as i32) };
        check(st, self.dim, self.dim)
    }

    /// The node's live bit; None for a node the index does not hold (nmn_hnsw_node_live).
    pub fn node_live(&self, node: usize) -> Option<bool> {
        match unsafe { ffi::nmn_hnsw_node_live(self.raw, node as u64) } {
            0 => Some(false),
            1 => Some(true),
            _ => None,
        }
    }

    /// `CacheIndex::search_with_metric` with node ids in place of keys (nmn_hnsw_cache_search): max(3k, 10) candidates from the walk,
    /// dead nodes dropped, every other re-scored under `metric` on its stored form, kept iff similarity >= threshold, best first,
    /// at most k.  Concurrent callers ride the coalescer's launches (docs/hnsw.md §16).  k == 0 answers empty here, as the
    /// reference's key layer does.
    pub fn cache_search(&self, q: &[f32], k: usize, threshold: f32, metric: &crate::ExtendedDistanceMetric) -> Result<Vec<(usize, f32)>> {
        if q.len() != self.dim {
            return Err(VectorError::DimensionMismatch { expected: self.dim, got: q.len() });
        }
        if k == 0 {
            return Ok(Vec::new());
        }
        let m = ffi::nmn_xmetric::from(metric);
        let mut ids = vec![u64::MAX; k];
        let mut scores = vec![f32::NEG_INFINITY; k];
        let mut n = 0u32;
        let st = unsafe {
            ffi::nmn_hnsw_cache_search(self.raw, q.as_ptr(), 1, k as u32, threshold, &m, ids.as_mut_ptr(), scores.as_mut_ptr(), &mut n,
                                       std::ptr::null_mut())
        };
        check(st, self.dim, q.len())?;
        Ok(ids.into_iter().zip(scores).take(n as usize).map(|(r, s)| (r as usize, s)).collect())
    }

    /// `CacheIndex::search_sparse_with_metric` with node ids in place of keys (nmn_hnsw_cache_search_sparse).  `q`: (position,
    /// value) pairs in any order, made a SparseVector as `try_from_parts` does.
    pub fn cache_search_sparse(&self, q: &[(u32, f32)], k: usize, threshold: f32, metric: &crate::ExtendedDistanceMetric) -> Result<Vec<(usize, f32)>> {
        if k == 0 {
            return Ok(Vec::new());
        }
        let indptr = [0u64, q.len() as u64];
        let positions: Vec<u32> = q.iter().map(|e| e.0).collect();
        let values: Vec<f32> = q.iter().map(|e| e.1).collect();
        let m = ffi::nmn_xmetric::from(metric);
        let mut ids = vec![u64::MAX; k];
        let mut scores = vec![f32::NEG_INFINITY; k];
        let mut n = 0u32;
        let st = unsafe {
            ffi::nmn_hnsw_cache_search_sparse(self.raw, indptr.as_ptr(), positions.as_ptr(), values.as_ptr(), 1, k as u32, threshold, &m,
                                              ids.as_mut_ptr(), scores.as_mut_ptr(), &mut n, std::ptr::null_mut())
        };
        check(st, self.dim, self.dim)?;
        Ok(ids.into_iter().zip(scores).take(n as usize).map(|(r, s)| (r as usize, s)).collect())
    }

    /// (batches that carried two or more concurrent calls, the calls in them) — nmn_hnsw_coalesce_stats.
    pub fn coalesce_stats(&self) -> (u64, u64) {
        let (mut b, mut c) = (0u64, 0u64);
        unsafe { ffi::nmn_hnsw_coalesce_stats(self.raw, &mut b, &mut c) };
        (b, c)
    }

    /// The handle's HNSWConfig; after `load`, the file's.
    pub fn config(&self) -> Result<ffi::nmn_hnsw_config> {
        let mut c = std::mem::MaybeUninit::<ffi::nmn_hnsw_config>::zeroed();
        check(unsafe { ffi::nmn_hnsw_get_config(self.raw, c.as_mut_ptr()) }, self.dim, self.dim)?;
        Ok(unsafe { c.assume_init() })
    }

    /// Graph, level generator state and rows (nmn_hnsw_save).  Searches may run meanwhile, inserts wait.
    pub fn save(&self, path: &Path) -> Result<()> {
        let p = c_path(path)?;
        check(unsafe { ffi::nmn_hnsw_save(self.raw, p.as_ptr()) }, self.dim, self.dim)
    }

    /// No build: the index comes back as saved (same answers, and `insert` continues where the saved index would have).  Every
    /// index of the file is checked on the host first; a damaged file is a SerializationError.  `max_file_bytes` /
    /// `max_entries` as for `GpuFlatIndex::load`.
    pub fn load(path: &Path, device: i32, capacity_hint: usize, max_file_bytes: u64, max_entries: u64) -> Result<Self> {
        let p = c_path(path)?;
        let mut raw = std::ptr::null_mut();
        check(unsafe { ffi::nmn_hnsw_load(p.as_ptr(), device, capacity_hint as u64, max_file_bytes, max_entries, &mut raw) }, 0, 0)?;
        let dim = unsafe { ffi::nmn_hnsw_dim(raw) } as usize;
        Ok(Self { raw, dim })
    }
}

impl Drop for GpuHnswIndex {
    fn drop(&mut self) {
        unsafe { ffi::nmn_hnsw_destroy(self.raw) };
    }
}

/// `tensor_store::ArchetypeRegistry` (delta_vector.rs:421-643) behind nmn_archetypes (docs/delta.md): archetypes and their
/// magnitude_sq in HBM, find_best_archetype and encode_batch for whole batches, bit for bit.
pub struct GpuArchetypeRegistry {
    raw: *mut ffi::nmn_archetypes,
    dim: usize,
}
unsafe impl Send for GpuArchetypeRegistry {}
unsafe impl Sync for GpuArchetypeRegistry {}

impl GpuArchetypeRegistry {
    pub fn new(dim: usize, max_archetypes: usize, device: i32) -> Result<Self> {
        let mut raw = std::ptr::null_mut();
        check(unsafe { ffi::nmn_archetypes_create(dim as u32, max_archetypes as u64, device, &mut raw) }, dim, dim)?;
        Ok(Self { raw, dim })
    }

    /// Calls of fewer rows than this run on the library's host restatement, same bits (nmn_delta_options).
    pub fn set_min_device_rows(&self, rows: u64) -> Result<()> {
        let opt = ffi::nmn_delta_options { min_device_rows: rows };
        check(unsafe { ffi::nmn_archetypes_set_options(self.raw, &opt) }, self.dim, self.dim)
    }

    pub fn len(&self) -> usize {
        unsafe { ffi::nmn_archetypes_len(self.raw) as usize }
    }

    /// ArchetypeRegistry::register for one archetype: None at max_archetypes.
    pub fn register(&self, archetype: &[f32]) -> Result<Option<usize>> {
        let mut id = -1i64;
        check(unsafe { ffi::nmn_archetypes_register(self.raw, archetype.as_ptr(), 1, &mut id) }, self.dim, archetype.len())?;
        Ok(if id < 0 { None } else { Some(id as usize) })
    }

    /// ArchetypeRegistry::discover_archetypes: the centroids of the exact GPU k-means, appended in order.
    pub fn discover_archetypes(&self, rows: &[f32], k: usize, opt: &ffi::nmn_kmeans_options) -> Result<usize> {
        let n = (rows.len() / self.dim.max(1)) as u64;
        let mut added = 0u64;
        check(unsafe { ffi::nmn_archetypes_discover(self.raw, rows.as_ptr(), n, k as u64, opt, &mut added) }, self.dim, self.dim)?;
        Ok(added as usize)
    }

    /// ArchetypeRegistry::find_best_archetype of every row: None on an empty registry.
    pub fn find_best(&self, rows: &[f32]) -> Result<Vec<Option<(usize, f32)>>> {
        let n = rows.len() / self.dim.max(1);
        let (mut ids, mut sims) = (vec![-1i64; n], vec![0f32; n]);
        check(unsafe { ffi::nmn_archetypes_find_best(self.raw, rows.as_ptr(), n as u64, ids.as_mut_ptr(), sims.as_mut_ptr()) }, self.dim, self.dim)?;
        Ok(ids.iter().zip(&sims).map(|(&i, &s)| if i < 0 { None } else { Some((i as usize, s)) }).collect())
    }

    /// ArchetypeRegistry::encode_batch: the delta rows stay together in one set; DimensionExceeded arrives as a StorageError with
    /// DeltaVectorError's Display.
    pub fn encode_batch(&self, rows: &[f32], threshold: f32, with_magnitude: bool) -> Result<GpuDeltaSet<'_>> {
        let n = (rows.len() / self.dim.max(1)) as u64;
        let mut raw = std::ptr::null_mut();
        check(unsafe { ffi::nmn_archetypes_encode_batch(self.raw, rows.as_ptr(), n, threshold, with_magnitude as i32, &mut raw) }, self.dim, self.dim)?;
        Ok(GpuDeltaSet { raw, registry: self })
    }

    /// encode_batch of `n` rows that are already on the device (docs/delta.md §9): a resident set without host arrays.  `rows_dev`
    /// is a DEVICE pointer to n x dim floats, `stream` a hipStream_t; the registry must be resident (nmn_archetypes_to_device).
    ///
    /// # Safety
    /// `rows_dev` must point to n x dim floats on the registry's device and stay unchanged until `stream` has run the call.
    pub unsafe fn encode_batch_device(&self, rows_dev: *const f32, n: usize, threshold: f32, with_magnitude: bool, stream: *mut std::ffi::c_void)
                                      -> Result<GpuDeltaSet<'_>> {
        let mut raw = std::ptr::null_mut();
        check(
            ffi::nmn_deltaset_encode_device(self.raw, rows_dev, n as u64, threshold, with_magnitude as i32, std::ptr::null_mut(), std::ptr::null_mut(),
                                            stream, &mut raw),
            self.dim,
            self.dim,
        )?;
        Ok(GpuDeltaSet { raw, registry: self })
    }
}

impl Drop for GpuArchetypeRegistry {
    fn drop(&mut self) {
        unsafe { ffi::nmn_archetypes_destroy(self.raw) };
    }
}

/// N `DeltaVector`s against one registry (nmn_delta_set); the borrow keeps the registry alive for as long as the set.
pub struct GpuDeltaSet<'a> {
    raw: *mut ffi::nmn_delta_set,
    registry: &'a GpuArchetypeRegistry,
}
unsafe impl Send for GpuDeltaSet<'_> {}
unsafe impl Sync for GpuDeltaSet<'_> {}

impl GpuDeltaSet<'_> {
    pub fn len(&self) -> usize {
        unsafe { ffi::nmn_delta_set_len(self.raw) as usize }
    }

    pub fn nnz(&self) -> usize {
        unsafe { ffi::nmn_delta_set_nnz(self.raw) as usize }
    }

    /// DeltaVector::compression_ratio of every row, the second half of encode_batch's pairs.
    pub fn compression_ratios(&self) -> Result<Vec<f32>> {
        let mut out = vec![0f32; self.len()];
        check(unsafe { ffi::nmn_delta_set_compression_ratio(self.raw, out.as_mut_ptr()) }, self.registry.dim, self.registry.dim)?;
        Ok(out)
    }

    /// ArchetypeRegistry::dot_delta_dense of every row with every query: out[q * len + row].
    pub fn dot_dense(&self, queries: &[f32]) -> Result<Vec<f32>> {
        let dim = self.registry.dim;
        let nq = queries.len() / dim.max(1);
        let mut out = vec![0f32; nq * self.len()];
        check(unsafe { ffi::nmn_delta_set_dot_dense(self.raw, queries.as_ptr(), nq as u32, out.as_mut_ptr()) }, dim, dim)?;
        Ok(out)
    }

    /// Top-k over the set (docs/delta.md §8): per query the first min(k, len) rows by (score descending, row ascending), the score
    /// being dot_dense's (`cosine` false) or cosine_similarity_dense's; each pair carries the row's own score bits.
    pub fn search(&self, queries: &[f32], k: usize, cosine: bool) -> Result<Vec<Vec<(usize, f32)>>> {
        let dim = self.registry.dim;
        let nq = queries.len() / dim.max(1);
        let (mut rows, mut scores, mut counts) = (vec![u64::MAX; nq * k], vec![f32::NEG_INFINITY; nq * k], vec![0u32; nq]);
        check(
            unsafe {
                ffi::nmn_deltaset_search(self.raw, queries.as_ptr(), nq as u32, k as u32, cosine as i32, rows.as_mut_ptr(), scores.as_mut_ptr(),
                                         counts.as_mut_ptr())
            },
            dim,
            dim,
        )?;
        Ok((0..nq).map(|q| (0..counts[q] as usize).map(|i| (rows[q * k + i] as usize, scores[q * k + i])).collect()).collect())
    }

    /// ArchetypeRegistry::decode of every row: out[row * dim ..].
    pub fn decode(&self) -> Result<Vec<f32>> {
        let dim = self.registry.dim;
        let mut out = vec![0f32; self.len() * dim];
        check(unsafe { ffi::nmn_delta_set_decode(self.raw, out.as_mut_ptr()) }, dim, dim)?;
        Ok(out)
    }
}

impl Drop for GpuDeltaSet<'_> {
    fn drop(&mut self) {
        unsafe { ffi::nmn_delta_set_destroy(self.raw) };
    }
}
