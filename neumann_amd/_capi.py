"""ctypes binding of libneumann_gpu.so (include/neumann_gpu.h).

This is the same C ABI the Rust `vector_engine::ffi` module binds; Python only
plays the role of the host language here because the image has no Rust toolchain.  Loading fails
loudly when the library has not been built: there is no Python/CPU fallback for the hot path.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# NEUMANN_GPU_LIB: an alternative build of the same library (A/B runs of kernel variants, tools/build_variant.sh)
LIB_PATH = os.environ.get("NEUMANN_GPU_LIB") or os.path.join(_HERE, "lib", "libneumann_gpu.so")

OK = 0
ERR_NOT_FOUND = -1
ERR_DIMENSION_MISMATCH = -2
ERR_EMPTY_VECTOR = -3
ERR_INVALID_TOP_K = -4
ERR_STORAGE = -5
ERR_CONFIGURATION = -6
ERR_COLLECTION_EXISTS = -7
ERR_COLLECTION_NOT_FOUND = -8
ERR_SEARCH_TIMEOUT = -9
ERR_IO = -10
ERR_SERIALIZATION = -11
ERR_INVALID_ARGUMENT = -20
ERR_NO_DEVICE = -21
ERR_OUT_OF_MEMORY = -22
ERR_TOP_K_TOO_LARGE = -23
ERR_CAPACITY = -24
ERR_BUFFER_TOO_SMALL = -25

MAX_TOP_K = 4096
MAX_QUERIES = 1024

METRIC_COSINE, METRIC_EUCLIDEAN, METRIC_DOT_PRODUCT = 0, 1, 2

f32p = C.POINTER(C.c_float)
u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)
i32p = C.POINTER(C.c_int32)
vp = C.c_void_p


class IndexDesc(C.Structure):
    _fields_ = [("dim", C.c_uint32), ("flags", C.c_uint32), ("capacity_rows", C.c_uint64),
                ("row_base", C.c_uint64), ("device", C.c_int32), ("cand_cap", C.c_uint32)]


class ShardedDesc(C.Structure):
    """nmn_sharded_desc: one corpus row-range sharded over several devices of ONE process."""
    _fields_ = [("dim", C.c_uint32), ("flags", C.c_uint32), ("capacity_rows", C.c_uint64), ("row_base", C.c_uint64),
                ("n_shards", C.c_uint32), ("gather", C.c_uint32), ("devices", C.POINTER(C.c_int32)),
                ("cand_cap", C.c_uint32), ("layout", C.c_uint32)]


GATHER_AUTO, GATHER_RCCL, GATHER_PEER = 0, 1, 2


class SearchStats(C.Structure):
    _fields_ = [("rows_scanned", C.c_uint64), ("bytes_scanned", C.c_uint64),
                ("candidates_rescored", C.c_uint32), ("fallback_queries", C.c_uint32),
                ("scan_ms", C.c_float), ("total_ms", C.c_float),
                ("sweep_kind", C.c_uint32), ("sweep_launches", C.c_uint32)]

    @property
    def sweep(self):
        """Name of `sweep_kind` as the library spells it (nmn_sweep_kind_str): ring_f32, valu_f32, valu_bf16, valu_i8, mfma_f32, ..."""
        return load().nmn_sweep_kind_str(self.sweep_kind).decode()


SWEEP_NONE, SWEEP_RING_F32, SWEEP_VALU_F32, SWEEP_VALU_BF16, SWEEP_VALU_I8, SWEEP_MFMA_F32, SWEEP_MFMA_BF16, SWEEP_MFMA_I8, SWEEP_EXACT, SWEEP_GRAPH = range(10)


class KMeansOptions(C.Structure):
    """nmn_kmeans_options (KMeansConfig, tensor_store/src/delta_vector.rs:691-711)."""
    _fields_ = [("max_iterations", C.c_uint64), ("convergence_threshold", C.c_float), ("seed", C.c_uint64),
                ("init_method", C.c_int32)]


class DeltaOptions(C.Structure):
    """nmn_delta_options: which calls of the delta-vector family take the device path (docs/delta.md)."""
    _fields_ = [("min_device_rows", C.c_uint64)]


class CoverageStats(C.Structure):
    """nmn_coverage_stats (CoverageStats, tensor_store/src/delta_vector.rs:677-687, without archetype_usage)."""
    _fields_ = [("avg_similarity", C.c_float), ("avg_compression_ratio", C.c_float), ("avg_delta_nnz", C.c_float),
                ("reserved", C.c_uint32)]


class IvfStorage(C.Structure):
    """nmn_ivf_storage (IVFStorage, tensor_store/src/ivf.rs:150-157; PQConfig, pq.rs:40-85; BinaryThreshold)."""
    _fields_ = [("kind", C.c_int32), ("pq_num_subspaces", C.c_uint32), ("pq_num_centroids", C.c_uint32),
                ("pq_kmeans", KMeansOptions), ("binary_threshold", C.c_int32)]


IVF_FLAT, IVF_PQ, IVF_BINARY = range(3)
BINARY_SIGN, BINARY_MEAN, BINARY_MEDIAN = range(3)


class HnswConfig(C.Structure):
    """nmn_hnsw_config (HNSWConfig, tensor_store/src/hnsw.rs:1434-1463)."""
    _fields_ = [("m", C.c_uint32), ("m0", C.c_uint32), ("ef_construction", C.c_uint32), ("ef_search", C.c_uint32),
                ("ml", C.c_double), ("max_nodes", C.c_uint64), ("sparsity_threshold", C.c_float),
                ("distance_metric", C.c_int32), ("storage", C.c_int32), ("reserved", C.c_uint32)]


HNSW_STORAGE_DENSE, HNSW_STORAGE_AUTO, HNSW_STORAGE_QUANTIZED, HNSW_STORAGE_BINARY = range(4)


class HnswBuildOptions(C.Structure):
    """nmn_hnsw_build_options (HNSWBuildOptions, vector_engine/src/lib.rs:848-858; include/neumann_engine.h)."""
    _fields_ = [("storage", C.c_int32), ("reserved", C.c_uint32), ("hnsw_config", HnswConfig)]


class HnswMemStats(C.Structure):
    """nmn_hnsw_memstats (HNSWMemoryStats, tensor_store/src/hnsw.rs:2733-2768)."""
    _fields_ = [(n, C.c_uint64) for n in ("total_nodes", "dense_count", "sparse_count", "delta_count", "tt_count",
                                          "quantized_count", "pq_count", "binary_count", "embedding_bytes")]


class HnswBulkStats(C.Structure):
    """nmn_hnsw_bulk_stats: the counters of nmn_hnsw_insert_bulk, cumulative per handle."""
    _fields_ = [(n, C.c_uint64) for n in ("batches", "walks", "accepted", "conflicts", "overflowed", "host_nodes",
                                          "patched_lists")]


class XMetric(C.Structure):
    """nmn_xmetric (tensor_store::DistanceMetric, tensor_store/src/distance.rs:13-52; the weights are GeometricConfig, 115-125)."""
    _fields_ = [("kind", C.c_int32), ("cosine_weight", C.c_float), ("structural_weight", C.c_float),
                ("magnitude_weight", C.c_float)]


(XMETRIC_COSINE, XMETRIC_ANGULAR, XMETRIC_GEODESIC, XMETRIC_JACCARD, XMETRIC_OVERLAP, XMETRIC_WEIGHTED_JACCARD,
 XMETRIC_EUCLIDEAN, XMETRIC_MANHATTAN, XMETRIC_COMPOSITE) = range(9)


class PredOp(C.Structure):
    """nmn_pred_op: one step of a WHERE-predicate program (include/neumann_gpu.h, NMN_PRED_*)."""
    _fields_ = [("op", C.c_uint32), ("cmp", C.c_uint32), ("vkind", C.c_uint32), ("column", C.c_uint32),
                ("a", C.c_uint64), ("b", C.c_uint64)]


CELL_ABSENT, CELL_NULL, CELL_BOOL, CELL_INT, CELL_FLOAT, CELL_STRING = range(6)
PRED_TRUE, PRED_FALSE, PRED_AND, PRED_OR, PRED_EXISTS, PRED_CMP, PRED_IN, PRED_STRSET = range(8)
CMP_EQ, CMP_NE, CMP_LT, CMP_LE, CMP_GT, CMP_GE = range(6)

# name -> (restype, argtypes); one entry per declaration in include/neumann_gpu.h
SIGNATURES = {
    "nmn_device_count": (C.c_int32, [i32p]),
    "nmn_status_str": (C.c_char_p, [C.c_int32]),
    "nmn_last_error": (C.c_char_p, []),
    "nmn_version": (C.c_char_p, []),
    "nmn_sweep_kind_str": (C.c_char_p, [C.c_uint32]),
    "nmn_select_form_counts": (C.c_int32, [u64p]),
    "nmn_index_create": (C.c_int32, [C.POINTER(IndexDesc), C.POINTER(vp)]),
    "nmn_index_destroy": (C.c_int32, [vp]),
    "nmn_index_upload": (C.c_int32, [vp, vp, C.c_uint64, C.c_uint64]),
    "nmn_index_upload_device": (C.c_int32, [vp, vp, C.c_uint64, C.c_uint64, vp]),
    "nmn_index_set_rows": (C.c_int32, [vp, C.c_uint64]),
    "nmn_index_rows": (C.c_uint64, [vp]),
    "nmn_index_dim": (C.c_uint32, [vp]),
    "nmn_index_row_stride": (C.c_uint32, [vp]),
    "nmn_index_row_base": (C.c_uint64, [vp]),
    "nmn_index_corpus_device": (vp, [vp, u32p]),
    "nmn_index_norms_device": (vp, [vp]),
    "nmn_index_search": (C.c_int32, [vp, vp, C.c_uint32, C.c_uint32, C.c_int32, vp, vp, vp, vp,
                                     C.POINTER(SearchStats)]),
    "nmn_index_search_device": (C.c_int32, [vp, vp, C.c_uint32, C.c_uint32, C.c_int32, vp, vp, vp, vp, vp]),
    "nmn_index_last_stats": (C.c_int32, [vp, vp, C.POINTER(SearchStats)]),
    "nmn_index_set_timing": (C.c_int32, [vp, C.c_int32]),
    "nmn_index_set_mirror": (C.c_int32, [vp, C.c_int32]),
    "nmn_index_scan_history": (C.c_int32, [vp, vp, C.POINTER(C.c_float), C.c_uint32, C.POINTER(C.c_uint32)]),
    "nmn_index_hbm_bytes": (C.c_int32, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "nmn_index_retry_declined": (C.c_int32, [vp]),
    "nmn_index_score_rows": (C.c_int32, [vp, vp, C.c_uint32, C.c_int32, vp, C.c_uint32, vp]),
    "nmn_index_count_exact": (C.c_int32, [vp, vp, C.c_int32, vp, C.c_float, u64p, u64p]),
    "nmn_index_read_probe": (C.c_int32, [vp, C.c_uint32, C.POINTER(C.c_double)]),
    "nmn_index_coalesce_stats": (C.c_int32, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "nmn_index_callers_probe": (C.c_int32, [vp, vp, C.c_uint32, C.c_uint32, C.c_int32, C.c_double, C.POINTER(C.c_double),
                                            C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "nmn_merge_topk_host": (C.c_int32, [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp]),
    "nmn_merge_topk_device": (C.c_int32, [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp]),
    "nmn_merge_topk_device_strided": (C.c_int32, [vp, vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                                  vp, vp, vp, vp]),
    "nmn_synth_value": (C.c_float, [C.c_uint64, C.c_uint64, C.c_uint32]),
    "nmn_synth_fill_host": (C.c_int32, [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32]),
    "nmn_index_fill_synthetic": (C.c_int32, [vp, C.c_uint64, C.c_uint64, C.c_uint64]),
    "nmn_index_set_row": (C.c_int32, [vp, C.c_uint64, vp]),
    "nmn_columns_create": (C.c_int32, [C.c_int32, C.c_uint64, C.POINTER(vp)]),
    "nmn_columns_destroy": (C.c_int32, [vp]),
    "nmn_columns_add": (C.c_int32, [vp, u32p]),
    "nmn_columns_count": (C.c_uint32, [vp]),
    "nmn_columns_write": (C.c_int32, [vp, C.c_uint32, C.c_uint64, C.c_uint64, vp, vp]),
    "nmn_columns_clear_row": (C.c_int32, [vp, C.c_uint64]),
    "nmn_columns_write_valid": (C.c_int32, [vp, C.c_uint64, C.c_uint64, vp]),
    "nmn_columns_eval": (C.c_int32, [vp, C.POINTER(PredOp), C.c_uint32, vp, C.c_uint64, C.c_uint64, u64p]),
    "nmn_columns_eval_acquire": (C.c_int32, [vp, C.POINTER(PredOp), C.c_uint32, vp, C.c_uint64, C.c_uint64, u64p,
                                             C.POINTER(C.c_uint32), C.POINTER(C.c_void_p)]),
    "nmn_columns_eval_release": (C.c_int32, [vp, C.c_uint32]),
    "nmn_index_search_pred": (C.c_int32, [vp, vp, C.POINTER(PredOp), C.c_uint32, vp, C.c_uint64, vp, C.c_uint32, C.c_uint32,
                                          C.c_int32, vp, vp, vp, u64p, C.POINTER(SearchStats)]),
    "nmn_columns_mask_device": (vp, [vp]),
    "nmn_columns_valid_device": (vp, [vp]),
    "nmn_columns_read_mask": (C.c_int32, [vp, vp, C.c_uint64]),
    "nmn_ivf_create": (C.c_int32, [C.POINTER(IndexDesc), vp, C.c_uint32, C.POINTER(vp)]),
    "nmn_ivf_destroy": (C.c_int32, [vp]),
    "nmn_ivf_build": (C.c_int32, [C.POINTER(IndexDesc), vp, C.c_uint64, C.c_uint32, C.POINTER(KMeansOptions), C.POINTER(vp)]),
    "nmn_ivf_centroids": (C.c_int32, [vp, vp, C.c_uint64]),
    "nmn_ivf_add": (C.c_int32, [vp, vp, C.c_uint64, vp]),
    "nmn_ivf_len": (C.c_uint64, [vp]),
    "nmn_ivf_list_major_rows": (C.c_uint64, [vp]),
    "nmn_ivf_clusters": (C.c_uint32, [vp]),
    "nmn_ivf_cluster_sizes": (C.c_int32, [vp, vp]),
    "nmn_ivf_search": (C.c_int32, [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.POINTER(SearchStats)]),
    "nmn_ivf_search_device": (C.c_int32, [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp]),
    "nmn_ivf_vectors": (vp, [vp]),
    "nmn_ivf_storage_default": (None, [C.POINTER(IvfStorage)]),
    "nmn_ivf_build_ex": (C.c_int32, [C.POINTER(IndexDesc), vp, C.c_uint64, C.c_uint32, C.POINTER(KMeansOptions),
                                     C.POINTER(IvfStorage), C.POINTER(vp)]),
    "nmn_ivf_create_ex": (C.c_int32, [C.POINTER(IndexDesc), vp, C.c_uint32, C.POINTER(IvfStorage), vp, C.c_uint32,
                                      C.POINTER(vp)]),
    "nmn_ivf_storage_kind": (C.c_int32, [vp]),
    "nmn_ivf_pq_codewords": (C.c_uint32, [vp]),
    "nmn_ivf_pq_codebook": (C.c_int32, [vp, vp, C.c_uint64]),
    "nmn_ivf_codes": (C.c_int32, [vp, vp, C.c_uint64]),
    "nmn_ivf_hbm_bytes": (C.c_uint64, [vp]),
    "nmn_hnsw_config_default": (None, [C.POINTER(HnswConfig)]),
    "nmn_hnsw_config_high_recall": (None, [C.POINTER(HnswConfig)]),
    "nmn_hnsw_config_high_speed": (None, [C.POINTER(HnswConfig)]),
    "nmn_hnsw_create": (C.c_int32, [C.POINTER(HnswConfig), C.c_uint32, C.c_uint64, C.c_int32, C.POINTER(vp)]),
    "nmn_hnsw_destroy": (C.c_int32, [vp]),
    "nmn_hnsw_insert": (C.c_int32, [vp, vp, C.c_uint64, vp]),
    "nmn_hnsw_insert_bulk": (C.c_int32, [vp, vp, C.c_uint64, vp]),
    "nmn_hnsw_set_bulk_policy": (C.c_int32, [vp, C.c_uint32, C.c_uint32]),
    "nmn_hnsw_get_bulk_stats": (C.c_int32, [vp, C.POINTER(HnswBulkStats)]),
    "nmn_hnsw_get_bulk_trace": (C.c_int32, [vp, vp, C.c_uint64, u64p]),
    "nmn_hnsw_insert_sparse": (C.c_int32, [vp, vp, vp, vp, C.c_uint64, vp]),
    "nmn_hnsw_insert_auto": (C.c_int32, [vp, vp, C.c_uint64, vp]),
    "nmn_hnsw_sparse_row": (C.c_int32, [vp, C.c_uint64, vp, vp, C.c_uint32, C.POINTER(C.c_uint32)]),
    "nmn_hnsw_len": (C.c_uint64, [vp]),
    "nmn_hnsw_dim": (C.c_uint32, [vp]),
    "nmn_hnsw_entry_point": (C.c_uint64, [vp]),
    "nmn_hnsw_max_layer": (C.c_uint32, [vp]),
    "nmn_hnsw_levels": (C.c_int32, [vp, vp, C.c_uint64]),
    "nmn_hnsw_neighbors": (C.c_int32, [vp, C.c_uint64, C.c_uint32, vp, C.c_uint32, u32p]),
    "nmn_hnsw_search": (C.c_int32, [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.POINTER(SearchStats)]),
    "nmn_hnsw_search_device": (C.c_int32, [vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp]),
    "nmn_sparse_canonicalise_device": (C.c_int32, [C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint64, C.c_uint32, vp, vp, vp, vp, vp, vp,
                                                   C.c_int32, vp]),
    "nmn_hnsw_search_sparse_device": (C.c_int32, [vp, vp, vp, vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp,
                                                  vp, vp]),
    "nmn_hnsw_search_multi": (C.c_int32, [vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp, vp, vp, C.POINTER(SearchStats)]),
    "nmn_hnsw_search_sparse": (C.c_int32, [vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, C.POINTER(SearchStats)]),
    "nmn_hnsw_search_sparse_multi": (C.c_int32, [vp, vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp, vp, vp, C.POINTER(SearchStats)]),
    "nmn_hnsw_coalesce_stats": (C.c_int32, [vp, vp, vp]),
    "nmn_hnsw_set_heap_capacity": (C.c_int32, [vp, C.c_uint32, C.c_uint32]),
    "nmn_hnsw_vectors": (vp, [vp]),
    "nmn_hnsw_hbm_bytes": (C.c_uint64, [vp]),
    "nmn_hnsw_create_with_storage": (C.c_int32, [C.POINTER(HnswConfig), C.c_int32, C.c_uint32, C.c_uint64, C.c_int32,
                                                 C.POINTER(vp)]),
    "nmn_hnsw_storage": (C.c_int32, [vp]),
    "nmn_hnsw_quantized_row": (C.c_int32, [vp, C.c_uint64, vp, f32p, f32p]),
    "nmn_hnsw_create_binary": (C.c_int32, [C.POINTER(HnswConfig), C.c_int32, C.c_uint32, C.c_uint64, C.c_int32, C.POINTER(vp)]),
    "nmn_hnsw_binary_threshold": (C.c_int32, [vp]),
    "nmn_hnsw_binary_row": (C.c_int32, [vp, C.c_uint64, vp, C.c_uint32]),
    "nmn_hnsw_get_vector": (C.c_int32, [vp, C.c_uint64, vp]),
    "nmn_hnsw_memory_stats": (C.c_int32, [vp, C.POINTER(HnswMemStats)]),
    "nmn_hnsw_get_config": (C.c_int32, [vp, C.POINTER(HnswConfig)]),
    "nmn_tt_reconstruct": (C.c_int32, [vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp]),
    "nmn_tt_norm": (C.c_int32, [vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp]),
    "nmn_tt_limits": (C.c_int32, [u32p, u32p, u32p, u32p]),
    "nmn_hnsw_search_tt": (C.c_int32, [vp, vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp,
                                       C.POINTER(SearchStats)]),
    "nmn_hnsw_search_tt_device": (C.c_int32, [vp, vp, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp]),
    "nmn_hnsw_insert_tt": (C.c_int32, [vp, vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp]),
    "nmn_hnsw_insert_embedding_tt": (C.c_int32, [vp, vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp]),
    "nmn_hnsw_tt_row": (C.c_int32, [vp, C.c_uint64, vp, vp, vp, vp, C.c_uint64, vp]),
    "nmn_hnsw_tt_walk_limits": (C.c_int32, [vp, C.c_uint32, vp, vp, vp]),
    "nmn_tt_config_for_dim": (C.c_int32, [C.c_uint64, C.c_uint32, u32p, u32p, u32p, C.POINTER(C.c_float)]),
    "nmn_tt_max_storage": (C.c_uint64, [vp, C.c_uint32, C.c_uint32]),
    "nmn_tt_decompose": (C.c_int32, [vp, C.c_uint64, C.c_uint64, vp, C.c_uint32, C.c_uint32, C.c_float, vp, vp, vp, vp, C.c_uint64]),
    "nmn_tt_decompose_device": (C.c_int32, [vp, C.c_uint64, C.c_uint64, vp, C.c_uint32, C.c_uint32, C.c_float, vp, vp, vp, vp,
                                            C.c_uint64, vp]),
    "nmn_tt_decompose_limits": (C.c_int32, [u32p, u32p, u32p, u32p]),
    "nmn_tt_decompose_lds_floats": (C.c_uint64, [vp, C.c_uint32, C.c_uint32]),
    "nmn_tt_similarity": (C.c_int32, [C.c_uint32, vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp]),
    "nmn_tt_self_dot": (C.c_int32, [vp, C.c_uint32, vp, vp, vp, C.c_uint32, vp]),
    "nmn_tt_self_dot_device": (C.c_int32, [vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp, C.c_uint32, vp, vp]),
    "nmn_tt_similarity_device": (C.c_int32, [C.c_uint32, vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp, C.c_uint32, vp, vp, vp, C.c_uint64,
                                             vp, C.c_uint32, vp, vp, vp, vp]),
    "nmn_hnsw_search_tt_dense": (C.c_int32, [vp, vp, C.c_uint32, C.c_uint64, vp, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, vp,
                                             vp, vp, C.POINTER(SearchStats)]),
    "nmn_hnsw_insert_tt_dense": (C.c_int32, [vp, vp, C.c_uint64, vp, C.c_uint32, C.c_uint32, C.c_float, vp]),
    "nmn_hnsw_insert_batch_tt": (C.c_int32, [vp, vp, C.c_uint64, C.c_uint64, vp, C.c_uint32, C.c_uint32, C.c_float, vp]),
    "nmn_xmetric_geometric_default": (None, [C.POINTER(XMetric)]),
    "nmn_xmetric_geometric_angular_heavy": (None, [C.POINTER(XMetric)]),
    "nmn_xmetric_geometric_structural_heavy": (None, [C.POINTER(XMetric)]),
    "nmn_xmetric_geometric_conflict_detection": (None, [C.POINTER(XMetric)]),
    "nmn_xmetric_to_similarity": (C.c_float, [C.POINTER(XMetric), C.c_float]),
    "nmn_xmetric_higher_is_better": (C.c_int32, [C.POINTER(XMetric)]),
    "nmn_index_score_rows_xmetric": (C.c_int32, [vp, vp, C.c_uint32, C.POINTER(XMetric), vp, C.c_uint32, vp, vp]),
    "nmn_xmetric_score_host_rows": (C.c_int32, [C.c_int32, vp, C.c_uint32, C.c_uint32, vp, C.POINTER(XMetric), vp, vp]),
    "nmn_hnsw_search_metric": (C.c_int32, [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(XMetric), vp, vp, vp,
                                           C.POINTER(SearchStats)]),
    "nmn_hnsw_search_metric_multi": (C.c_int32, [vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp, vp, vp, C.POINTER(SearchStats)]),
    "nmn_hnsw_search_metric_device": (C.c_int32, [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(XMetric), vp, vp, vp, vp]),
    "nmn_hnsw_set_node_mask": (C.c_int32, [vp, vp, C.c_uint64, C.c_int32]),
    "nmn_hnsw_node_live": (C.c_int32, [vp, C.c_uint64]),
    "nmn_hnsw_cache_search": (C.c_int32, [vp, vp, C.c_uint32, C.c_uint32, C.c_float, C.POINTER(XMetric), vp, vp, vp,
                                          C.POINTER(SearchStats)]),
    "nmn_hnsw_cache_search_sparse": (C.c_int32, [vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_float, C.POINTER(XMetric), vp, vp, vp,
                                                 C.POINTER(SearchStats)]),
    "nmn_hnsw_cache_search_device": (C.c_int32, [vp, vp, C.c_uint32, C.c_uint32, C.c_float, C.POINTER(XMetric), vp, vp, vp, vp]),
    "nmn_hnsw_cache_search_sparse_device": (C.c_int32, [vp, vp, vp, vp, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_float,
                                                        C.POINTER(XMetric), vp, vp, vp, vp, vp]),
    "nmn_delta_options_default": (None, [C.POINTER(DeltaOptions)]),
    "nmn_delta_limits": (C.c_int32, [u32p, u32p, u32p, u32p]),
    "nmn_archetypes_create": (C.c_int32, [C.c_uint32, C.c_uint64, C.c_int32, C.POINTER(vp)]),
    "nmn_archetypes_destroy": (C.c_int32, [vp]),
    "nmn_archetypes_set_options": (C.c_int32, [vp, C.POINTER(DeltaOptions)]),
    "nmn_archetypes_register": (C.c_int32, [vp, vp, C.c_uint64, vp]),
    "nmn_archetypes_discover": (C.c_int32, [vp, vp, C.c_uint64, C.c_uint64, C.POINTER(KMeansOptions), u64p]),
    "nmn_archetypes_len": (C.c_uint64, [vp]),
    "nmn_archetypes_dim": (C.c_uint32, [vp]),
    "nmn_archetypes_max": (C.c_uint64, [vp]),
    "nmn_archetypes_get": (C.c_int32, [vp, C.c_uint64, vp]),
    "nmn_archetypes_magnitude_sq": (C.c_int32, [vp, C.c_uint64, f32p]),
    "nmn_archetypes_find_best": (C.c_int32, [vp, vp, C.c_uint64, vp, vp]),
    "nmn_archetypes_analyze_coverage": (C.c_int32, [vp, vp, C.c_uint64, C.c_float, C.POINTER(CoverageStats), vp]),
    "nmn_archetypes_encode_batch": (C.c_int32, [vp, vp, C.c_uint64, C.c_float, C.c_int32, C.POINTER(vp)]),
    "nmn_delta_set_from_parts": (C.c_int32, [vp, C.c_uint64, vp, vp, vp, vp, vp, vp, C.POINTER(vp)]),
    "nmn_delta_set_destroy": (C.c_int32, [vp]),
    "nmn_delta_set_len": (C.c_uint64, [vp]),
    "nmn_delta_set_nnz": (C.c_uint64, [vp]),
    "nmn_delta_set_arrays": (C.c_int32, [vp, vp, vp, vp, vp, vp, vp, vp]),
    "nmn_delta_set_compression_ratio": (C.c_int32, [vp, vp]),
    "nmn_delta_set_memory_bytes": (C.c_int32, [vp, vp]),
    "nmn_delta_set_decode": (C.c_int32, [vp, vp]),
    "nmn_delta_set_magnitudes": (C.c_int32, [vp, vp]),
    "nmn_delta_set_dot_dense": (C.c_int32, [vp, vp, C.c_uint32, vp]),
    "nmn_delta_set_cosine_dense": (C.c_int32, [vp, vp, C.c_uint32, vp]),
    "nmn_delta_set_dot_same_archetype": (C.c_int32, [vp, vp, vp, C.c_uint64, vp, vp]),
    "nmn_archetypes_to_device": (C.c_int32, [vp]),
    "nmn_delta_set_to_device": (C.c_int32, [vp]),
    "nmn_archetypes_find_best_device": (C.c_int32, [vp, vp, C.c_uint64, vp, vp, vp]),
    "nmn_delta_set_dot_dense_device": (C.c_int32, [vp, vp, C.c_uint32, vp, vp, vp]),
    "nmn_delta_set_cosine_dense_device": (C.c_int32, [vp, vp, C.c_uint32, vp, vp, vp]),
    "nmn_deltaset_encode_device": (C.c_int32, [vp, vp, C.c_uint64, C.c_float, C.c_int32, vp, vp, vp, C.POINTER(vp)]),
    "nmn_deltaset_host_arrays_present": (C.c_int32, [vp]),
    "nmn_deltaset_limits": (C.c_int32, [u32p, u32p, u64p, u64p]),
    "nmn_deltaset_search": (C.c_int32, [vp, vp, C.c_uint32, C.c_uint32, C.c_int32, vp, vp, vp]),
    "nmn_deltaset_search_scratch_bytes": (C.c_uint64, [vp, C.c_uint32, C.c_uint32]),
    "nmn_deltaset_search_device": (C.c_int32, [vp, vp, C.c_uint32, C.c_uint32, C.c_int32, vp, C.c_uint64, vp, vp, vp, vp]),
    "nmn_index_save": (C.c_int32, [vp, C.c_char_p]),
    "nmn_index_load": (C.c_int32, [C.c_char_p, C.POINTER(IndexDesc), C.c_uint64, C.c_uint64, C.POINTER(vp)]),
    "nmn_ivf_save": (C.c_int32, [vp, C.c_char_p]),
    "nmn_ivf_load": (C.c_int32, [C.c_char_p, C.POINTER(IndexDesc), C.c_uint64, C.c_uint64, C.POINTER(vp)]),
    "nmn_hnsw_save": (C.c_int32, [vp, C.c_char_p]),
    "nmn_hnsw_load": (C.c_int32, [C.c_char_p, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(vp)]),
    "nmn_sharded_create": (C.c_int32, [C.POINTER(ShardedDesc), C.POINTER(vp)]),
    "nmn_sharded_destroy": (C.c_int32, [vp]),
    "nmn_sharded_upload": (C.c_int32, [vp, vp, C.c_uint64, C.c_uint64]),
    "nmn_sharded_fill_synthetic": (C.c_int32, [vp, C.c_uint64, C.c_uint64, C.c_uint64]),
    "nmn_sharded_search": (C.c_int32, [vp, vp, C.c_uint32, C.c_uint32, C.c_int32, vp, vp, vp, vp, C.POINTER(SearchStats)]),
    "nmn_sharded_shards": (C.c_uint32, [vp]),
    "nmn_sharded_rows": (C.c_uint64, [vp]),
    "nmn_sharded_shard": (vp, [vp, C.c_uint32]),
    "nmn_sharded_device": (C.c_int32, [vp, C.c_uint32]),
    "nmn_sharded_gather_mode": (C.c_uint32, [vp]),
    "nmn_sharded_layout": (C.c_uint32, [vp]),
    "nmn_sharded_global_row": (C.c_uint64, [vp, C.c_uint32, C.c_uint64]),
    "nmn_sharded_rccl_ranks": (C.c_uint32, [vp]),
    "nmn_sharded_set_timing": (C.c_int32, [vp, C.c_int32]),
    "nmn_sharded_set_mirror": (C.c_int32, [vp, C.c_int32]),
    "nmn_sharded_last_gather_ms": (C.c_int32, [vp, C.POINTER(C.c_float)]),
    "nmn_sharded_coalesce_stats": (C.c_int32, [vp, vp, vp]),
    "nmn_index_search_dmask": (C.c_int32, [vp, vp, C.c_uint32, C.c_uint32, C.c_int32, vp, vp, vp, vp,
                                           C.POINTER(SearchStats)]),
    "nmn_index_search_dmask_hint": (C.c_int32, [vp, vp, C.c_uint32, C.c_uint32, C.c_int32, vp, C.c_uint64, vp, vp, vp,
                                                C.POINTER(SearchStats)]),
}

_lib = None


class NeumannGpuError(RuntimeError):
    """A non-zero nmn_status.  `.status` is the code, the message mirrors VectorError's Display."""

    def __init__(self, status, detail=""):
        self.status = status
        msg = load().nmn_status_str(status).decode()
        if detail:
            msg = f"{msg}: {detail}"
        super().__init__(msg)


def _preload_torch_hip_runtime():
    """One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64.so (SONAME
    libamdhip64.so.7, the SONAME libneumann_gpu.so needs).  If ours resolved to /opt/rocm first, a later
    `import torch` would bring up a second runtime in the same process (torch then sees no GPU, and torch
    streams / tensors would belong to a different runtime than our kernels).  Loading torch's copy first
    makes the dynamic loader satisfy our NEEDED entry with it.  Without torch installed this is a no-op
    and the system ROCm runtime is used."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    """Load the shared library (once).  Raises if it was not built — no fallback."""
    global _lib
    if _lib is None:
        _preload_torch_hip_runtime()
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -m neumann_amd.build` "
                "(neumann_amd has no CPU fallback for the SIMILAR TOP-K path)")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError = header/library mismatch: fail loudly
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(status):
    if status != OK:
        detail = load().nmn_last_error().decode(errors="replace")
        raise NeumannGpuError(status, detail)


def select_form_counts():
    """(flat, split, walk): launches of select_kernel by form since the library was loaded (nmn_select_form_counts)."""
    out = (C.c_uint64 * 3)()
    check(load().nmn_select_form_counts(out))
    return tuple(int(x) for x in out)
