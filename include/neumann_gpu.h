/*
 * neumann_gpu.h — C ABI of libneumann_gpu.so, the MI355X (gfx950) flat-scan index behind
 * Neumann's `vector_engine` SIMILAR TOP-K hot path.
 *
 * The reference (Shadylukin/Neumann, Rust, `unsafe_code = "forbid"`) has no FFI of its own; the
 * boundary it offers is the public API of crate `vector_engine`.  Every entry point below therefore
 * cites the reference code it REPLACES (paths relative to the reference root) and is exactly what
 * the `ffi` module of a GPU-enabled `vector_engine` crate binds (see INTEGRATION.md for the
 * `extern "C"` block and the safe `GpuFlatIndex` wrapper).
 *
 * Conventions: plain C, caller-owned buffers, opaque handles, `nmn_status` return (0 = ok,
 * negative = error; values mirror `VectorError`, vector_engine/src/lib.rs:101-149), no exceptions
 * or torch types across the boundary.  Streams are passed as `void*` (a `hipStream_t`; NULL = the
 * legacy default stream).  All `*_device` entry points are asynchronous on that stream.
 *
 * There is NO CPU fallback anywhere in this library: without a usable gfx950 device every compute
 * entry point returns NMN_ERR_NO_DEVICE.
 */
#ifndef NEUMANN_GPU_H
#define NEUMANN_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t nmn_status;

/* Status codes.  The first block mirrors VectorError (vector_engine/src/lib.rs:101-149). */
#define NMN_OK 0
#define NMN_ERR_NOT_FOUND (-1)            /* VectorError::NotFound            */
#define NMN_ERR_DIMENSION_MISMATCH (-2)   /* VectorError::DimensionMismatch   */
#define NMN_ERR_EMPTY_VECTOR (-3)         /* VectorError::EmptyVector         */
#define NMN_ERR_INVALID_TOP_K (-4)        /* VectorError::InvalidTopK         */
#define NMN_ERR_STORAGE (-5)              /* VectorError::StorageError (HIP runtime failure) */
#define NMN_ERR_CONFIGURATION (-6)        /* VectorError::ConfigurationError  */
#define NMN_ERR_COLLECTION_EXISTS (-7)    /* VectorError::CollectionExists    */
#define NMN_ERR_COLLECTION_NOT_FOUND (-8) /* VectorError::CollectionNotFound  */
#define NMN_ERR_SEARCH_TIMEOUT (-9)       /* VectorError::SearchTimeout       */
#define NMN_ERR_IO (-10)                  /* VectorError::IoError             (index files: open / read / write) */
#define NMN_ERR_SERIALIZATION (-11)       /* VectorError::SerializationError  (index files: not decodable / corrupt) */
/* Shim-only codes (no VectorError counterpart). */
#define NMN_ERR_INVALID_ARGUMENT (-20)
#define NMN_ERR_NO_DEVICE (-21)
#define NMN_ERR_OUT_OF_MEMORY (-22)
#define NMN_ERR_TOP_K_TOO_LARGE (-23)     /* reserved (k > NMN_MAX_TOP_K is served by the large-k path) */
#define NMN_ERR_CAPACITY (-24)            /* upload beyond capacity_rows */
#define NMN_ERR_BUFFER_TOO_SMALL (-25)

/* Largest k the candidate pipeline serves (single-workgroup final sort in LDS).  Larger k is legal — the
 * reference sorts everything and truncates (lib.rs:2026-2034) — and takes the large-k path: exact score
 * of every row, full device sort, first k (neumann_amd/csrc/nmn_sortk.hip). */
#define NMN_MAX_TOP_K 4096u
/* Largest number of queries one search call accepts. */
#define NMN_MAX_QUERIES 1024u

/* DistanceMetric, same order as vector_engine/src/lib.rs:268-289. */
typedef enum nmn_metric {
    NMN_METRIC_COSINE = 0,
    NMN_METRIC_EUCLIDEAN = 1,
    NMN_METRIC_DOT_PRODUCT = 2,
    /* Not a vector_engine metric: tensor_blob's artifact similarity (tensor_blob/src/lib.rs:591-625), i.e.
     * SparseVector::from_dense(a).cosine_similarity(&SparseVector::from_dense(b)) — f64 dot and magnitudes over
     * the non-zero positions, NaN/Inf -> 0, clamped to [-1, 1], rounded once to f32 (sparse_vector.rs:583-599). */
    NMN_METRIC_SPARSE_COSINE_F64 = 3
} nmn_metric;

typedef struct nmn_index nmn_index; /* opaque: one row-range shard resident on one GPU */

/* nmn_index_desc.flags.  By default a row length is padded up to the next multiple of 128 elements only when that costs at
 * most 1/8 more bytes per sweep (1000 -> 1024); with NMN_INDEX_WIDE_ROWS also when it costs up to 1/2 more (300 -> 384,
 * 200 -> 256, 100 -> 128): batches of queries and concurrent callers then take the matrix-core sweep (up to 128 queries per
 * corpus read instead of 4) at the price of that much more HBM and single-query sweep time.  Results are the same. */
#define NMN_INDEX_WIDE_ROWS 1u
/* Shards of <= 65 536 rows (<= 64 MiB, dim <= 768) answer a single-query nmn_index_search (k <= 1024) with ONE kernel launch:
 * exact reference-order scores of every row, selection and sort in that launch, the query in the kernel arguments and the
 * result written straight into pinned host memory (neumann_amd/csrc/nmn_exact.hip: tiny_search_kernel).  With this flag
 * such searches take the general pipeline (sweep, select, rescore, final) instead: same answers; for tests and A/B runs. */
#define NMN_INDEX_NO_SINGLE_LAUNCH 2u

typedef struct nmn_index_desc {
    uint32_t dim;            /* vector dimension d (>0) */
    uint32_t flags;          /* NMN_INDEX_* bits, 0 = defaults */
    uint64_t capacity_rows;  /* rows this shard can hold (HBM is allocated up front) */
    uint64_t row_base;       /* global id of local row 0 (shard offset; §8e row-range sharding) */
    int32_t device;          /* HIP device ordinal, -1 = current device */
    uint32_t cand_cap;       /* per-query candidate capacity before the exact-fallback path; 0 = default 4096 */
} nmn_index_desc;

/* Timing / accounting of the most recent search on a workspace (nullable everywhere). */
typedef struct nmn_search_stats {
    uint64_t rows_scanned;        /* rows whose vectors were read (mask-excluded rows are not) */
    uint64_t bytes_scanned;       /* algorithmic bytes of the scan: rows_scanned * dim * (4: f32 corpus, 2: bf16 mirror, 1: 8-bit mirror) */
    uint32_t candidates_rescored; /* max over queries of rows re-scored in reference order */
    uint32_t fallback_queries;    /* queries that took the exact-fallback path */
    float scan_ms;                /* hipEvent span of the scan kernel(s); -1 if not timed */
    float total_ms;               /* hipEvent span scan+select+rescore+sort; -1 if not timed */
    uint32_t sweep_kind;          /* NMN_SWEEP_*: which kernel streamed the rows for this search (the library's own dispatch decision) */
    uint32_t sweep_launches;      /* kernel launches of that sweep per query pass (sampling pass and bound kernels included) */
} nmn_search_stats;

/* nmn_search_stats.sweep_kind: the kernel that read the corpus (or its mirror) for the last search. */
#define NMN_SWEEP_NONE 0u       /* no rows (empty shard) */
#define NMN_SWEEP_RING_F32 1u   /* nmn::scan_ring_kernel: one unmasked query, f32 rows through the LDS-DMA ring (SURVEY §8(d) headline) */
#define NMN_SWEEP_VALU_F32 2u   /* nmn::scan_kernel over the f32 rows (bitmaps, 2-4 queries, small shards) */
#define NMN_SWEEP_VALU_BF16 3u  /* nmn::scan_kernel over the bf16 mirror */
#define NMN_SWEEP_VALU_I8 4u    /* nmn::scan_i8_kernel over the 8-bit mirror */
#define NMN_SWEEP_MFMA_F32 5u   /* nmn::scan_mfma_kernel over the f32 rows (rounded to bf16 in registers) */
#define NMN_SWEEP_MFMA_BF16 6u  /* nmn::scan_mfma_kernel over the bf16 mirror */
#define NMN_SWEEP_MFMA_I8 7u    /* nmn::scan_mfma_kernel over the 8-bit mirror */
#define NMN_SWEEP_EXACT 8u      /* exact reference-order scores of every row, no approximate sweep (tiny_search_kernel, large-k path) */
#define NMN_SWEEP_GRAPH 9u      /* not a sweep: nmn::hnsw_search_kernel walked an HNSW graph; rows_scanned = distance evaluations made */
/* Name of a NMN_SWEEP_* value ("ring_f32", "valu_f32", "valu_bf16", "valu_i8", "mfma_f32", "mfma_bf16", "mfma_i8", "exact", "graph", "none"). */
const char* nmn_sweep_kind_str(uint32_t sweep_kind);

/* ---- device / lifecycle ------------------------------------------------------------------- */

/* Number of usable HIP devices (0 and NMN_OK when none). */
nmn_status nmn_device_count(int32_t* n);

/* Human-readable text of a status code.  Mirrors `impl Display for VectorError`
 * (vector_engine/src/lib.rs:151-183) for the mirrored codes. */
const char* nmn_status_str(nmn_status s);

/* Text of the last HIP/runtime failure on the calling thread ("" if none). */
const char* nmn_last_error(void);

/* Library version "major.minor.patch". */
const char* nmn_version(void);

/* Which form of the candidate selection the searches of this process took: launches of nmn::select_kernel since the library was
 * loaded, out[0] the flat path (shards of <= 16 384 tiles), out[1] the split selection (lone callers, k <= 256, 16 385 .. 262 144
 * tiles), out[2] the three-level walk (everything else; NMN_NO_FLAT_SELECT=1 / NMN_NO_SPLIT_SELECT=1 send the other two there).
 * Process-wide, all shards and devices together; one launch serves all queries of a pass.  For tests and A/B runs. */
nmn_status nmn_select_form_counts(uint64_t* out);

/* Allocate one shard: corpus[capacity_rows][ld] f32 row-major (ld = dim rounded up to 8, or to the next multiple of 128 if that is at most 1/8 more; zero
 * padded), norms[capacity_rows] f32.  Replaces the per-row `TensorStore` reads of the hot loop
 * (vector_engine/src/lib.rs:2121-2138; tensor_store/src/lib.rs:948-963) by one resident matrix. */
nmn_status nmn_index_create(const nmn_index_desc* desc, nmn_index** out);
nmn_status nmn_index_destroy(nmn_index* idx);

/* Copy n rows (row-major n x dim f32, HOST memory) into local rows [row0, row0+n) and compute
 * their magnitudes in reference order (`simd::magnitude`, tensor_store/src/hnsw.rs:198-229), so
 * the scan never recomputes |v| (the reference does, per row per query: lib.rs:2257-2266).
 * Rows above the current row count extend it; gaps are not allowed (row0 <= rows). */
nmn_status nmn_index_upload(nmn_index* idx, const float* rows_host, uint64_t row0, uint64_t n);
/* Same, rows already in DEVICE memory (row-major n x dim, tightly packed). Asynchronous. */
nmn_status nmn_index_upload_device(nmn_index* idx, const float* rows_dev, uint64_t row0, uint64_t n,
                                   void* stream);
/* Truncate/extend the logical row count without touching data (rows <= capacity). */
nmn_status nmn_index_set_rows(nmn_index* idx, uint64_t rows);

uint64_t nmn_index_rows(const nmn_index* idx);
uint32_t nmn_index_dim(const nmn_index* idx);
/* Elements per stored row including the zero padding (>= dim; a multiple of 128 when batches take the matrix-core sweep). */
uint32_t nmn_index_row_stride(const nmn_index* idx);
uint64_t nmn_index_row_base(const nmn_index* idx);
/* Device pointers of the resident data (for zero-copy producers and for tests). */
const float* nmn_index_corpus_device(const nmn_index* idx, uint32_t* ld_out);
const float* nmn_index_norms_device(const nmn_index* idx);

/* ---- the hot path ------------------------------------------------------------------------- */

/* SIMILAR TOP-K over the shard.  Replaces `search_similar` / `search_similar_with_metric` /
 * `search_in_collection` scoring + full sort + truncate (vector_engine/src/lib.rs:1950-2101,
 * 1585-1689) and, with `mask`, the survivor scan of `search_with_pre_filter` (lib.rs:3514-3557).
 *
 *   queries  nq x dim f32, HOST.          k  >= 1 (k > NMN_MAX_TOP_K: large-k path, exact scores + select/sort per query)
 *   mask     nullable HOST bitmap, ceil(rows/64) u64 words, bit i of word i/64 (LSB first) = row i
 *            takes part (layout of relational_engine's selection bitmaps, simd.rs:6-311).
 *   out_rows   nq x k  global row ids (row_base + local row), best first; unused slots = UINT64_MAX
 *   out_scores nq x k  scores exactly as the reference computes them (compute_score,
 *            lib.rs:2231-2266; lane order hnsw.rs:168-229); unused slots = -inf
 *   out_counts nq      min(k, rows taking part)
 * Ranking: score descending, equal scores by ascending row id (the reference's own tie order is
 * unspecified: slab_router.rs:287-305).  Zero-magnitude handling is the caller's (lib.rs:1970-1974):
 * at this level a zero query under COSINE scores every row 0.0, as cosine_similarity does.
 * Synchronous: returns after the results are in the host buffers. */
nmn_status nmn_index_search(nmn_index* idx, const float* queries, uint32_t nq, uint32_t k,
                            nmn_metric metric, const uint64_t* mask, uint64_t* out_rows,
                            float* out_scores, uint32_t* out_counts, nmn_search_stats* stats);

/* Same with every buffer in DEVICE memory; enqueues on `stream` and returns immediately.
 * Calls on one stream may be pipelined back to back (they share that stream's workspace). */
nmn_status nmn_index_search_device(nmn_index* idx, const float* queries_dev, uint32_t nq, uint32_t k,
                                   nmn_metric metric, const uint64_t* mask_dev, uint64_t* out_rows_dev,
                                   float* out_scores_dev, uint32_t* out_counts_dev, void* stream);

/* Stats of the last search enqueued on `stream` (synchronises that stream). */
nmn_status nmn_index_last_stats(nmn_index* idx, void* stream, nmn_search_stats* stats);
/* With timing on (nmn_index_set_timing): the sweep durations (HIP events on the launch stream, around the dominant kernel) of
 * the searches enqueued on `stream` since the last call — at most the 64 most recent, oldest first; synchronises the stream.
 * What bench.py averages over its timed loop for `roofline.achieved`. */
nmn_status nmn_index_scan_history(nmn_index* idx, void* stream, float* scan_ms, uint32_t cap, uint32_t* n_out);
/* Which matrix the approximate sweep streams.  enabled == 1 (default): the smallest mirror that serves the call —
 *   the shard's 8-BIT mirror (int8 codes with a scale per row, 1 byte per corpus element) for sweeps of 1-2 queries over rows
 *     whose stride is a multiple of 128 elements up to 4096 (128, 256, 384, ... — nmn_index_create pads row lengths just short
 *     of one up to it), and for query batches (matrix cores) where the stride is a multiple of 256 up to 1536, or 2048, or 3072
 *     (3072 under NMN_METRIC_EUCLIDEAN stays on the bf16 mirror);
 *   else its bf16 mirror (2 bytes per element; every row stride, VALU sweeps and — strides of 128 .. 768, 1024, 1280, 1536,
 *     2048, 3072, 4096 — the matrix cores);
 *   else the f32 rows.
 * A shard keeps ONE mirror by default: the one built while its rows arrive (the 8-bit one where the stride allows it: 5 bytes
 * per element resident with the f32 rows; nmn_index_hbm_bytes reports it), and builds the other only when a call needs it.  A
 * mirror that does not fit the device's free memory (with room to spare for workspaces) is not built: the call is served from
 * the next one down — never an error.  Mirrors carry their MEASURED rounding error into the candidate margin, and a shard whose
 * 8-bit margin keeps overflowing the candidate lists returns to the bf16 mirror by itself.
 * enabled == 2: the bf16 mirror only.  enabled == 0: the row-major f32 corpus itself — the sweep SURVEY.md §8(d) prices at
 * rows * dim * 4 bytes per query (bench.py's headline: `value`, `roofline`); query batches then take the matrix-core sweep over
 * the f32 rows themselves (rounded to bf16 in registers: the rows' bytes once per 64-128 queries, nmn_scan_mfma_f32.hip).  Any other
 * value: NMN_ERR_INVALID_ARGUMENT.  Results are identical in every mode (every candidate is re-scored from the f32 corpus in
 * the reference's order). */
nmn_status nmn_index_set_mirror(nmn_index* idx, int32_t enabled);
/* Device memory the shard holds for its rows: corpus_bytes = the f32 rows (capacity x stride x 4), mirror_bytes = the 8-bit and
 * bf16 mirrors that exist right now, with their per-row factors; per_row_bytes = magnitudes and their reciprocals.  Workspaces
 * (per stream, sized by the largest search seen) are not counted.  Any pointer may be null.  No side effects. */
nmn_status nmn_index_hbm_bytes(nmn_index* idx, uint64_t* corpus_bytes, uint64_t* mirror_bytes, uint64_t* per_row_bytes);
/* A mirror that was declined (or a query pass that was shrunk) because the device was short of memory stays declined until the
 * verdict expires (every 4096 searches) — or until this call: the next search that wants the mirror / the larger pass asks the device
 * again.  For a host that has just freed memory on the device (dropped a sibling shard, a collection). */
nmn_status nmn_index_retry_declined(nmn_index* idx);
/* hipEvent timing of searches (default 0 = off).  1: events at the start and end of the pipeline and around its sweep (scan_ms,
 * total_ms of nmn_index_last_stats).  2: the two events around the sweep only (scan_ms, nmn_index_scan_history) — what a timed
 * loop can afford on a small shard: every event is a packet of its own in the queue (1M x 768: four more cost ~9 % of a step). */
nmn_status nmn_index_set_timing(nmn_index* idx, int32_t enabled);

/* Reference-order scores of arbitrary rows (the exact-rescore kernel exposed on its own):
 * out[q*n_rows + i] = compute_score(query q, row rows[i]).  HOST buffers.  Used by the parity
 * tests and by `compute_similarity`-style callers (lib.rs:2268-2290). */
nmn_status nmn_index_score_rows(nmn_index* idx, const float* queries, uint32_t nq, nmn_metric metric,
                                const uint64_t* local_rows, uint32_t n_rows, float* out_scores);

/* Count local rows whose reference-order score is > / == the given score (full exact pass; a
 * size-independent certificate for top-k results at scales the CPU oracle cannot reach). */
nmn_status nmn_index_count_exact(nmn_index* idx, const float* query, nmn_metric metric,
                                 const uint64_t* mask, float score, uint64_t* n_greater,
                                 uint64_t* n_equal);

/* Measurement aid: a pure read sweep over the shard, best of `reps` runs, in GB/s: the data movement of the sweep a single f32 query
 * takes on this shard with the arithmetic and every store removed — the LDS-DMA ring of nmn::scan_ring_kernel where that kernel
 * serves (>= 4096 tiles, stride a multiple of 128 up to 4096), nmn::scan_kernel's register loads elsewhere.  What a read-only
 * kernel can reach on this device; bench.py reports the sweep against it (`ring_only_read_ceiling`). */
nmn_status nmn_index_read_probe(nmn_index* idx, uint32_t reps, double* gbps_out);

/* Measurement aid: `threads` host threads call nmn_index_search(nq = 1, k, metric) in a loop for `seconds`, thread t
 * with query t of `queries` (HOST, threads x dim).  Reports calls per second, how many sweeps carried >= 2 calls and
 * how many calls rode in them, and how many of the checked answers differed bit-wise from the same query searched
 * alone before the threads started (must be 0).  bench.py reports it as `concurrent_callers`. */
nmn_status nmn_index_callers_probe(nmn_index* idx, const float* queries, uint32_t threads, uint32_t k, nmn_metric metric,
                                   double seconds, double* calls_per_s, uint64_t* merged_batches,
                                   uint64_t* merged_calls, uint64_t* mismatches);

/* ---- shard merge (multi-GPU) -------------------------------------------------------------- */

/* Merge `n_lists` per-shard top-k lists (each nq x k, padded as nmn_index_search pads) into one:
 * concatenate, order by (score desc, row asc), keep k — `ResultMerger::merge_top_k`
 * (query_router/src/distributed.rs:413-433).  Layout of the inputs: [list][query][k], i.e. what an
 * all-gather of per-rank outputs produces.  HOST version (router-side merge): */
nmn_status nmn_merge_topk_host(const uint64_t* rows, const float* scores, const uint32_t* counts,
                               uint32_t n_lists, uint32_t nq, uint32_t k, uint64_t* out_rows,
                               float* out_scores, uint32_t* out_counts);
/* DEVICE version, asynchronous on `stream` (merges the RCCL all-gather output in place on GPU). */
nmn_status nmn_merge_topk_device(const uint64_t* rows_dev, const float* scores_dev,
                                 const uint32_t* counts_dev, uint32_t n_lists, uint32_t nq, uint32_t k,
                                 uint64_t* out_rows_dev, float* out_scores_dev, uint32_t* out_counts_dev,
                                 void* stream);

/* Same merge over an all-gather of PACKED per-rank blocks: rank l's rows / scores / counts start at
 * (char*)rows_dev + l*list_stride_bytes etc., so one collective can move all three fields.  With
 * list_stride_bytes == 0 the layout is the contiguous one of nmn_merge_topk_device. */
nmn_status nmn_merge_topk_device_strided(const uint64_t* rows_dev, const float* scores_dev,
                                         const uint32_t* counts_dev, uint64_t list_stride_bytes, uint32_t n_lists,
                                         uint32_t nq, uint32_t k, uint64_t* out_rows_dev, float* out_scores_dev,
                                         uint32_t* out_counts_dev, void* stream);

/* ---- multi-GPU in ONE process: row-range shards over the GPUs of a node --------------------- */

/* The reference host is one process sharing an Arc<VectorEngine> (query_router/src/lib.rs:710); what it offers for
 * spreading a SIMILAR over several holders of the data is the distributed planner's scatter-gather — every shard runs
 * the query, ResultMerger::merge_top_k concatenates, sorts by score descending and truncates
 * (query_router/src/distributed.rs:173-180, 413-433).  nmn_sharded is that with GPUs as shards, behind one handle a
 * single host process drives (SURVEY.md §8b `nmn_index_desc{.., n_gpus, gpu_ids[]}`, §8e): shard g holds the global
 * rows [g*ceil(N/G), (g+1)*ceil(N/G)) on devices[g]; a search replicates the queries, runs the single-shard pipeline
 * on every device's own stream, gathers the per-shard top-k blocks with ONE collective — an RCCL all-gather over xGMI
 * (ncclCommInitAll communicators, grouped calls) when every shard has a device of its own, peer copies when several
 * LOGICAL shards share a device — and merges them on the device of shard 0 (nmn_merge_topk_device_strided's kernel).
 * The answer is the unsharded one: rows, scores, tie order (global top-k is a subset of the union of the local ones).
 * Calls on one handle are serialised; use one handle per concurrent client group, or the per-shard handles
 * (nmn_sharded_shard) with nmn_merge_topk_* directly. */
typedef struct nmn_sharded nmn_sharded;

#define NMN_MAX_SHARDS 64u
#define NMN_GATHER_AUTO 0u /* RCCL when the shards' devices are distinct (and there are >= 2), else peer copies */
#define NMN_GATHER_RCCL 1u /* ncclAllGather, one communicator rank per shard; needs distinct devices (1 shard is legal) */
#define NMN_GATHER_PEER 2u /* hipMemcpyPeerAsync of every block into the merging device's gather buffer */
/* How the global rows map to the shards.  RANGES (default): shard g holds [g*ceil(N/G), (g+1)*ceil(N/G)) of
 * the CAPACITY — the layout of a corpus loaded once (bench.py, config 4).  CYCLIC: 64-row blocks (one scan tile, one bitmap
 * word) are dealt round-robin, block b -> shard b % G, so the rows HELD are spread evenly however few of the capacity's rows
 * exist and wherever appends land — what a store that grows and shrinks needs (the engine's mirrors: with RANGES the n live
 * rows of a mirror with 50 % spare capacity filled shard 0, then shard 1, ... and left the last GPUs idle).  Same API, same
 * answers: row ids in and out are the global ones. */
#define NMN_SHARDED_LAYOUT_RANGES 0u
#define NMN_SHARDED_LAYOUT_CYCLIC 1u

typedef struct nmn_sharded_desc {
    uint32_t dim;            /* vector dimension d (>0) */
    uint32_t flags;          /* NMN_INDEX_* bits, applied to every shard */
    uint64_t capacity_rows;  /* rows of the WHOLE corpus; shard g gets the rows [g*ceil(N/G), ...) */
    uint64_t row_base;       /* global id of row 0 of the whole corpus */
    uint32_t n_shards;       /* G, 1..NMN_MAX_SHARDS */
    uint32_t gather;         /* NMN_GATHER_* */
    const int32_t* devices;  /* [n_shards] HIP device ordinal of each shard (repeats = logical shards on one GPU);
                                NULL = round-robin over the node's devices */
    uint32_t cand_cap;       /* as nmn_index_desc.cand_cap */
    uint32_t layout;         /* NMN_SHARDED_LAYOUT_*; 0 = contiguous row ranges */
} nmn_sharded_desc;

nmn_status nmn_sharded_create(const nmn_sharded_desc* desc, nmn_sharded** out);
nmn_status nmn_sharded_destroy(nmn_sharded* s);
/* nmn_index_upload over the GLOBAL row numbering: rows [row0, row0+n) (HOST, row-major n x dim) go to the shards whose
 * ranges they fall into.  Rows must arrive in global order (row0 <= nmn_sharded_rows: a gap is refused before any shard is
 * touched).  With shards on several devices the parts are copied side by side, one host thread per shard (the same threads
 * enqueue every shard's search pipeline at once; environment NMN_SHARDED_CREW=1|0 forces them on / off). */
nmn_status nmn_sharded_upload(nmn_sharded* s, const float* rows_host, uint64_t row0, uint64_t n);
/* nmn_index_fill_synthetic over the global numbering: the shards together hold exactly the unsharded corpus. */
nmn_status nmn_sharded_fill_synthetic(nmn_sharded* s, uint64_t seed, uint64_t row0, uint64_t n);
/* nmn_index_search over all shards: same arguments (HOST buffers; `mask` is ONE bitmap over the global rows, bit i =
 * row row_base + i, sliced per shard here), same outputs, same ranking.  stats: rows / bytes summed over the shards,
 * times = the slowest shard's (they run side by side).  Synchronous. */
nmn_status nmn_sharded_search(nmn_sharded* s, const float* queries, uint32_t nq, uint32_t k, nmn_metric metric,
                              const uint64_t* mask, uint64_t* out_rows, float* out_scores, uint32_t* out_counts,
                              nmn_search_stats* stats);
uint32_t nmn_sharded_shards(const nmn_sharded* s);
uint64_t nmn_sharded_rows(const nmn_sharded* s);               /* rows held, all shards */
nmn_index* nmn_sharded_shard(nmn_sharded* s, uint32_t g);      /* the shard's own handle (owned by s) */
int32_t nmn_sharded_device(const nmn_sharded* s, uint32_t g);  /* HIP device of shard g */
uint32_t nmn_sharded_gather_mode(const nmn_sharded* s);        /* NMN_GATHER_RCCL or NMN_GATHER_PEER: what create chose */
uint32_t nmn_sharded_layout(const nmn_sharded* s);             /* NMN_SHARDED_LAYOUT_* in effect (1 shard: RANGES) */
/* global id (row_base included) of local row `local_row` of shard g under the handle's layout; UINT64_MAX for a bad shard */
uint64_t nmn_sharded_global_row(const nmn_sharded* s, uint32_t g, uint64_t local_row);
/* nmn_sharded_create on >= 2 shards ends with a SELF-TEST of the collective a search will use: every shard puts its rank
 * into its result block, the blocks travel through the very gather code path (grouped ncclAllGather on the communicators of
 * ncclCommInitAll, or the peer copies), and the merging device — with RCCL every device — must hold ranks 0..G-1 in order.
 * A failure is NMN_ERR_STORAGE with the reason in nmn_last_error(), at create time instead of inside the first search.
 * nmn_sharded_rccl_ranks: communicator ranks that took part in that all-gather (ncclCommCount of the handle's communicators,
 * cross-checked against the gathered ranks); 0 when the gather is peer copies. */
uint32_t nmn_sharded_rccl_ranks(const nmn_sharded* s);
nmn_status nmn_sharded_set_timing(nmn_sharded* s, int32_t enabled);  /* hipEvent timing of the shards' sweeps and of gather+merge */
nmn_status nmn_sharded_set_mirror(nmn_sharded* s, int32_t enabled);  /* nmn_index_set_mirror on every shard */
/* hipEvent span of the last search's collective + merge on the merging device (ms; -1 when not timed).  It starts when
 * shard 0's pipeline is done, so it includes waiting for slower shards. */
nmn_status nmn_sharded_last_gather_ms(const nmn_sharded* s, float* ms);
/* Concurrent callers: the handle may be searched from any number of threads (the reference shares one Arc<VectorEngine>,
 * query_router/src/lib.rs:710).  A search that arrives while another runs waits; when the running one ends the oldest
 * waiter leads the next sweep and takes every waiting search of the same metric (no bitmap, k <= NMN_MAX_TOP_K) along as ONE query batch
 * — up to 128 queries, k = the largest asked for; each caller receives the first k entries of its own queries' lists,
 * i.e. exactly what it gets alone.  Uploads run alone, in arrival order.  batches / calls: sweeps that carried two or
 * more calls, and the calls in them. */
nmn_status nmn_sharded_coalesce_stats(nmn_sharded* s, uint64_t* batches, uint64_t* calls);

/* ---- columnar metadata + WHERE-predicate programs ----------------------- */

/* Filtered SIMILAR in the reference evaluates the predicate per key on the host: one `store.get`
 * (BTreeMap lookup + TensorData clone) and one `evaluate_filter` walk per stored row
 * (vector_engine/src/lib.rs:3526-3530, 3582-3630).  Here the metadata fields of the mirrored rows
 * live as typed COLUMNS in HBM, aligned with the rows of an nmn_index, and the predicate is a
 * postfix program one kernel evaluates for every row, writing the selection bitmap the masked scan
 * consumes (same layout as relational_engine's bitmaps: bit i of word i/64, LSB first).
 *
 * A cell is (kind u8, payload u64).  Strings are dictionary-encoded per column by the caller; every
 * string predicate reaches the device as a bitset over dictionary ids (NMN_PRED_STRSET), so the
 * string comparison itself runs once per DISTINCT value on the host, never per row. */
typedef struct nmn_columns nmn_columns;

#define NMN_CELL_ABSENT 0u /* the row has no such field (TensorData::get -> None)        */
#define NMN_CELL_NULL 1u   /* ScalarValue::Null                                            */
#define NMN_CELL_BOOL 2u   /* ScalarValue::Bool,   payload 0/1                             */
#define NMN_CELL_INT 3u    /* ScalarValue::Int,    payload = the i64's bits                */
#define NMN_CELL_FLOAT 4u  /* ScalarValue::Float,  payload = the f64's bits                */
#define NMN_CELL_STRING 5u /* ScalarValue::String, payload = dictionary id in this column  */

/* Program opcodes: postfix over a 64-deep boolean stack; the program must leave exactly one value. */
#define NMN_PRED_TRUE 0u   /* push true                       (FilterCondition::True)                   */
#define NMN_PRED_FALSE 1u  /* push false                      (a field no row has)                      */
#define NMN_PRED_AND 2u    /* pop b, pop a, push a && b       (FilterCondition::And)                    */
#define NMN_PRED_OR 3u     /* pop b, pop a, push a || b       (FilterCondition::Or)                     */
#define NMN_PRED_EXISTS 4u /* push kind != ABSENT             (Exists, lib.rs:3602)                     */
#define NMN_PRED_CMP 5u    /* push cmp(cell, value)           (Eq/Ne/Lt/Le/Gt/Ge, lib.rs:3603-3620; the
                              typed comparison of compare_tensor_value_to_filter, lib.rs:3648-3670:
                              Int/Int, Float/Float, Float/Int, Int/Float (int side widened `as f64`),
                              Bool/Bool, Null/Null; anything else, or a NaN operand, is false) */
#define NMN_PRED_IN 6u     /* push any_j cell == value_j      (In, lib.rs:3627-3629); values are the
                              (kind,payload) pairs consts[a .. a+2*b) */
#define NMN_PRED_STRSET 7u /* push kind == STRING && bit payload of the bitset consts[a ..] (b = number
                              of ids covered)              (string Eq/Ne/Lt/Le/Gt/Ge, Contains,
                              StartsWith, string members of In; lib.rs:3621-3626, 3673-3692) */

/* cmp field of NMN_PRED_CMP, FilterCondition order (lib.rs:296-309). */
#define NMN_CMP_EQ 0u
#define NMN_CMP_NE 1u
#define NMN_CMP_LT 2u
#define NMN_CMP_LE 3u
#define NMN_CMP_GT 4u
#define NMN_CMP_GE 5u

typedef struct nmn_pred_op {
    uint32_t op;     /* NMN_PRED_*                                            */
    uint32_t cmp;    /* NMN_CMP_* (CMP only)                                  */
    uint32_t vkind;  /* NMN_CELL_* kind of the filter value (CMP only)        */
    uint32_t column; /* column id (EXISTS, CMP, IN, STRSET)                   */
    uint64_t a;      /* CMP: value payload; IN / STRSET: offset into consts   */
    uint64_t b;      /* IN: number of values; STRSET: number of ids covered   */
} nmn_pred_op;

/* A column set for `capacity_rows` rows on `device` (-1 = current).  All cells start ABSENT and the
 * row-validity bitmap starts all-zero. */
nmn_status nmn_columns_create(int32_t device, uint64_t capacity_rows, nmn_columns** out);
nmn_status nmn_columns_destroy(nmn_columns* cols);
/* Add one column (every cell ABSENT); its id is returned in *column_out. */
nmn_status nmn_columns_add(nmn_columns* cols, uint32_t* column_out);
uint32_t nmn_columns_count(const nmn_columns* cols);
/* Write cells [row0, row0+n) of one column from HOST arrays. */
nmn_status nmn_columns_write(nmn_columns* cols, uint32_t column, uint64_t row0, uint64_t n,
                             const uint8_t* kinds, const uint64_t* payloads);
/* Make every column's cell of `row` ABSENT (a key overwritten in place drops its old metadata:
 * `put` replaces the whole TensorData, tensor_store/src/lib.rs:927-938, vector_engine/src/lib.rs:3291-3307). */
nmn_status nmn_columns_clear_row(nmn_columns* cols, uint64_t row);
/* Write words [word0, word0+n) of the row-validity bitmap (rows that exist and are not deleted); every
 * evaluation is ANDed with it. */
nmn_status nmn_columns_write_valid(nmn_columns* cols, uint64_t word0, uint64_t n_words, const uint64_t* words);
/* Evaluate the program over rows [0, n_rows): the resulting bitmap stays in device memory
 * (nmn_columns_mask_device), *count_out = number of selected rows.  `prog` and `consts` are HOST
 * arrays.  Synchronous.  Replaces the `list_keys().filter(evaluate_filter_for_key)` stage of
 * search_with_pre_filter (lib.rs:3526-3530) and of search_filtered_in_collection (lib.rs:1776-1784). */
nmn_status nmn_columns_eval(nmn_columns* cols, const nmn_pred_op* prog, uint32_t n_ops, const uint64_t* consts,
                            uint64_t n_consts, uint64_t n_rows, uint64_t* count_out);
/* The same evaluation for concurrent callers (filtered searches of many threads under a shared lock): the result goes
 * to a bitmap of its own, *mask_out (device, ceil(capacity_rows/64) words), which the caller holds — together with the
 * stream and staging the evaluation ran on — as slot *slot_out until nmn_columns_eval_release.  Evaluations of
 * different slots overlap on the device; searches that pass different slot bitmaps to nmn_index_search_dmask share one
 * corpus sweep (request coalescing, one bitmap per query).  Must not run concurrently with the nmn_columns_write*
 * family (the engine's writers hold its exclusive lock). */
nmn_status nmn_columns_eval_acquire(nmn_columns* cols, const nmn_pred_op* prog, uint32_t n_ops, const uint64_t* consts,
                                    uint64_t n_consts, uint64_t n_rows, uint64_t* count_out, uint32_t* slot_out,
                                    const uint64_t** mask_out);
nmn_status nmn_columns_eval_release(nmn_columns* cols, uint32_t slot);
/* Filtered search in ONE call: evaluate `prog` over `cols` (rows [0, nmn_index_rows(idx)), same row numbering as the
 * shard) and search the rows it selects — `search_with_pre_filter` (lib.rs:3514-3557) end to end.  For concurrent
 * callers this is the fast form: the request coalescer hands the predicates of all the calls riding one query batch
 * to a single launch on the batch's stream, right before the ONE sweep that serves them (one bitmap per query), so
 * a filtered search waits for one batch, not for an evaluation and then a batch.  *selected_out (nullable) = rows the
 * predicate selected; results as nmn_index_search_dmask over that bitmap (k <= NMN_MAX_TOP_K).  queries HOST nq x dim. */
nmn_status nmn_index_search_pred(nmn_index* idx, nmn_columns* cols, const nmn_pred_op* prog, uint32_t n_ops,
                                 const uint64_t* consts, uint64_t n_consts, const float* queries, uint32_t nq, uint32_t k,
                                 nmn_metric metric, uint64_t* out_rows, float* out_scores, uint32_t* out_counts,
                                 uint64_t* selected_out, nmn_search_stats* stats);
/* Device bitmap of the last nmn_columns_eval, ceil(capacity_rows/64) words. */
const uint64_t* nmn_columns_mask_device(const nmn_columns* cols);
/* Device row-validity bitmap (a ready-made mask of the live rows). */
const uint64_t* nmn_columns_valid_device(const nmn_columns* cols);
/* Copy words of the last evaluation's bitmap to the host (tests). */
nmn_status nmn_columns_read_mask(nmn_columns* cols, uint64_t* out_words, uint64_t n_words);

/* nmn_index_search with the selection bitmap already in DEVICE memory (e.g. nmn_columns_mask_device);
 * queries and outputs are HOST buffers as in nmn_index_search.  Synchronous. */
nmn_status nmn_index_search_dmask(nmn_index* idx, const float* queries, uint32_t nq, uint32_t k,
                                  nmn_metric metric, const uint64_t* mask_dev, uint64_t* out_rows,
                                  float* out_scores, uint32_t* out_counts, nmn_search_stats* stats);
/* The same, with the number of rows the bitmap selects (the predicate kernel's count) as a hint for the request
 * coalescer: concurrent searches with DIFFERENT device bitmaps share one sweep (one bitmap per query, every row read)
 * once their selectivities add up to a whole sweep; below that each is swept alone and skips what it excludes. */
nmn_status nmn_index_search_dmask_hint(nmn_index* idx, const float* queries, uint32_t nq, uint32_t k, nmn_metric metric,
                                       const uint64_t* mask_dev, uint64_t mask_rows, uint64_t* out_rows,
                                       float* out_scores, uint32_t* out_counts, nmn_search_stats* stats);

/* Request coalescing of the host-buffer searches (nmn_index_search / _dmask): callers that arrive while a search is
 * running on the shard wait and leave together as ONE query batch (same metric and mask, <= 64 queries, k <= 4096),
 * i.e. one corpus sweep instead of one each.  The reference serves concurrent `search_similar` calls of an
 * `Arc<VectorEngine>` (query_router/src/lib.rs:710, 5615-5666) one scan per call; results here are the same per
 * call whatever the batch.  Counters: batches that merged >= 2 calls, and the calls merged.  NMN_NO_COALESCE=1
 * turns it off. */
nmn_status nmn_index_coalesce_stats(nmn_index* idx, uint64_t* batches, uint64_t* requests);

/* ---- IVF-Flat probe ------------------------------------------------------ */

/* `tensor_store::ivf::IVFIndex` with `IVFStorage::Flat` (tensor_store/src/ivf.rs:160-406), searched on the
 * GPU.  nmn_ivf_create takes centroids trained elsewhere; nmn_ivf_build trains them (ivf.rs:222-233) on the GPU.
 * Vectors live in id (insertion) order; ids are the row numbers `add` assigns (ivf.rs:287-289). */
typedef struct nmn_ivf nmn_ivf;
/* desc: dim, capacity_rows (vectors that can be added), device; centroids: HOST, n_clusters x dim. */
nmn_status nmn_ivf_create(const nmn_index_desc* desc, const float* centroids, uint32_t n_clusters, nmn_ivf** out);
nmn_status nmn_ivf_destroy(nmn_ivf* ivf);
/* IVFIndex::train(vectors) followed by add(v) for every vector (ivf.rs:222-316), the k-means
 * (tensor_store/src/delta_vector.rs:737-901, KMeans::fit) run on the GPU bit for bit: assignment = the exact
 * centroid sweep, centroid update = one thread per (cluster, dimension) adding the members in vector order,
 * k-means++ distances on the device with the f32 running sums on the host.  rows_host: n x dim; the index gets
 * min(num_clusters, n) lists; desc->capacity_rows >= n. */
typedef struct nmn_kmeans_options {
    uint64_t max_iterations;      /* KMeansConfig::max_iterations (100)        */
    float convergence_threshold;  /* KMeansConfig::convergence_threshold (1e-4) */
    uint64_t seed;                /* KMeansConfig::seed (42)                   */
    int32_t init_method;          /* 0 = KMeansInit::Random, 1 = KMeansPlusPlus */
} nmn_kmeans_options;
nmn_status nmn_ivf_build(const nmn_index_desc* desc, const float* rows_host, uint64_t n, uint32_t num_clusters,
                         const nmn_kmeans_options* opt, nmn_ivf** out);
/* The centroids, row-major n_clusters x dim, into HOST memory. */
nmn_status nmn_ivf_centroids(nmn_ivf* ivf, float* out, uint64_t cap_floats);
/* IVFIndex::add for n vectors (HOST, n x dim): each goes to the list of its nearest centroid
 * (squared Euclidean, first minimum: find_nearest_centroid, ivf.rs:490-497) and gets the next id.
 * clusters_out (nullable, HOST [n]) receives the chosen clusters. */
nmn_status nmn_ivf_add(nmn_ivf* ivf, const float* rows_host, uint64_t n, uint32_t* clusters_out);
uint64_t nmn_ivf_len(const nmn_ivf* ivf);       /* IVFIndex::len, ivf.rs:409-415 */
uint32_t nmn_ivf_clusters(const nmn_ivf* ivf);
nmn_status nmn_ivf_cluster_sizes(nmn_ivf* ivf, uint64_t* out_sizes /* [n_clusters] */); /* ivf.rs:448-454 */
/* IVFIndex::search_with_nprobe (ivf.rs:325-406): the nprobe nearest centroids (squared distance,
 * ascending, ties by index), every vector of their lists scored by Euclidean distance
 * `squared_euclidean(q, v).sqrt()`, ascending; equal distances in probe order of the cluster, then id.
 *   queries HOST nq x dim;  out_ids nq x k (unused = UINT64_MAX);  out_distances nq x k (unused = +inf);
 *   out_counts nq = min(k, vectors in the probed lists).  Synchronous.
 * Every query is answered as if it had been searched alone (the reference's method takes one query); what nq > 1 buys is
 * throughput: up to 64 queries at a time share the centroid sweep and its host round trip, and their list scans run as one
 * batched sweep that reads a bitmap per query whenever that is cheaper than nq launch-bound scans (2M x 768, nprobe 8:
 * 0.21 ms per call at nq = 1, 0.033 ms per query at nq = 32). */
nmn_status nmn_ivf_search(nmn_ivf* ivf, const float* queries, uint32_t nq, uint32_t k, uint32_t nprobe,
                          uint64_t* out_ids, float* out_distances, uint32_t* out_counts, nmn_search_stats* stats);
/* nmn_ivf_search with every buffer in DEVICE memory, for every storage (Flat, PQ, Binary): queries_dev nq x dim (tightly
 * packed), out_ids_dev / out_distances_dev nq x k, out_counts_dev nq.  Returns what nmn_ivf_search returns for the same index
 * state, bit for bit.  Enqueues on `stream` (NULL: the default stream) and returns without waiting: the centroid ranking, the
 * candidate plan, the scan of the probed lists, the top-k selection and the id map all run on the device, nothing is read
 * back, and a call of a shape (nq, k, nprobe, index size) the stream has served before allocates nothing and waits for
 * nothing (growing a stream's workspace waits for that stream).  Calls on one stream may be pipelined (they share that
 * stream's workspace); none of the host call's scratch is used, so host and device searches of one index run side by side.
 * A call answers for the index as it was when it returned: nmn_ivf_add and nmn_ivf_destroy wait for the device searches in
 * flight before they change or free what those read.  The first call builds a device copy of the list offsets and the
 * candidate-order id map (4 bytes per vector; rebuilt after an add), counted by nmn_ivf_hbm_bytes from then on. */
nmn_status nmn_ivf_search_device(nmn_ivf* ivf, const float* queries_dev, uint32_t nq, uint32_t k, uint32_t nprobe,
                                 uint64_t* out_ids_dev, float* out_distances_dev, uint32_t* out_counts_dev, void* stream);
/* Vectors (ids [0, n)) the LIST-MAJOR copy covers: the reference keeps a Vec of entries per list (ivf.rs:160-175), and so
 * does the device — a second copy of the vectors ordered by list, over which a probe reads contiguous row ranges and no
 * per-row array; laid out after nmn_ivf_build / nmn_ivf_load and again whenever the vectors added since make up an eighth of
 * it (those are scanned through a bitmap over the id-ordered rows meanwhile).  0: no copy (fewer than 4096 vectors, or no
 * HBM for it) — every probe goes through the bitmap.  Results are the same either way. */
uint64_t nmn_ivf_list_major_rows(const nmn_ivf* ivf);
/* The flat index holding the vectors (exhaustive search over the same rows, stats, ...).  NULL for a PQ / Binary index. */
nmn_index* nmn_ivf_vectors(nmn_ivf* ivf);

/* ---- IVF-PQ / IVF-Binary storage (tensor_store/src/ivf.rs:61-157, pq.rs, binary_quantization.rs) ---------------- */

/* IVFStorage: how the vectors of the lists are kept.  PQ and Binary keep only codes in HBM — no f32 row stays on the device
 * once nmn_ivf_build_ex returns.  Centroids and list assignment are Flat's (the same exact k-means and nearest-centroid
 * sweep); a PQ index also trains a codebook on the residuals v - centroid[list(v)] (ivf.rs:235-249, pq.rs:114-169). */
#define NMN_IVF_FLAT 0
#define NMN_IVF_PQ 1
#define NMN_IVF_BINARY 2
#define NMN_BINARY_SIGN 0   /* BinaryThreshold::Sign:   bit i = v[i] > 0.0 */
#define NMN_BINARY_MEAN 1   /* BinaryThreshold::Mean:   bit i = v[i] > sequential f32 sum / len */
#define NMN_BINARY_MEDIAN 2 /* BinaryThreshold::Median: bit i = v[i] > the middle element (f64 midpoint of the two middle ones) */
typedef struct nmn_ivf_storage {
    int32_t kind;                   /* NMN_IVF_FLAT / NMN_IVF_PQ / NMN_IVF_BINARY */
    uint32_t pq_num_subspaces;      /* PQConfig::num_subspaces (8); dim % it must be 0, else NMN_ERR_CONFIGURATION */
    uint32_t pq_num_centroids;      /* PQConfig::num_centroids (256); K' = min(it, n) codewords per subspace */
    nmn_kmeans_options pq_kmeans;   /* PQConfig::kmeans_config (KMeansConfig::default), separate from the IVF k-means */
    int32_t binary_threshold;       /* NMN_BINARY_SIGN / _MEAN / _MEDIAN */
} nmn_ivf_storage;
/* IVFStorage::Flat, PQConfig::default and BinaryThreshold::Sign */
void nmn_ivf_storage_default(nmn_ivf_storage* s);
/* nmn_ivf_build for any storage (nmn_ivf_build == this with NMN_IVF_FLAT).  PQ: K' = min(pq_num_centroids, n) codewords per
 * subspace, each subspace one exact k-means over the residuals' sub-vectors with storage->pq_kmeans.  A PQ / Binary index
 * holds desc->capacity_rows codes, not rows. */
nmn_status nmn_ivf_build_ex(const nmn_index_desc* desc, const float* rows_host, uint64_t n, uint32_t num_clusters,
                            const nmn_kmeans_options* kmeans, const nmn_ivf_storage* storage, nmn_ivf** out);
/* nmn_ivf_create for any storage: centroids (HOST, n_clusters x dim) and, for PQ, the codebook trained elsewhere (HOST,
 * [M][K][dim / M] f32; nullable when K == 0) with K codewords per subspace.  K is ignored for Flat / Binary. */
nmn_status nmn_ivf_create_ex(const nmn_index_desc* desc, const float* centroids, uint32_t n_clusters, const nmn_ivf_storage* storage,
                             const float* pq_codebook, uint32_t K, nmn_ivf** out);
int32_t nmn_ivf_storage_kind(const nmn_ivf* ivf);
/* codewords per subspace of a PQ index (K'), 0 otherwise */
uint32_t nmn_ivf_pq_codewords(const nmn_ivf* ivf);
/* The PQ codebook, [M][K'][dim / M] f32, into HOST memory (NMN_ERR_CONFIGURATION for another kind). */
nmn_status nmn_ivf_pq_codebook(nmn_ivf* ivf, float* out, uint64_t cap_floats);
/* The codes in ID order into HOST memory: PQ M bytes per vector, Binary ceil(dim / 64) little-endian u64 words per vector
 * (bit i of word i / 64 = component i above the threshold).  cap_bytes >= len x that; NMN_ERR_CONFIGURATION for Flat. */
nmn_status nmn_ivf_codes(nmn_ivf* ivf, void* out, uint64_t cap_bytes);
/* Device memory the index holds right now (vectors or codes, centroids, codebook, lists, search scratch). */
uint64_t nmn_ivf_hbm_bytes(nmn_ivf* ivf);

/* ---- HNSW graph index (tensor_store/src/hnsw.rs:1554-2335), searched on the GPU ------------------------------- */

/* `tensor_store::HNSWIndex` with dense or 8-bit quantized storage.  The graph is built on the host in the reference's order (the build is
 * sequential by definition of its result; the reference's is too) and is resident in HBM: layer 0 as n x m0 u32 slots and a
 * count per node, the upper layers as a compact n_upper x max_layer x m table with a row index per node.  Node id == row of
 * the flat index the handle owns (nmn_hnsw_vectors).  Answers are the reference's bit for bit, ties included: both priority
 * queues of search_layer are kept as the array algorithm of std::collections::BinaryHeap (docs/hnsw.md).  nmn_hnsw_save /
 * nmn_hnsw_load (index persistence, below) keep a built graph across restarts. */
typedef struct nmn_hnsw nmn_hnsw;

/* HNSWStorageStrategy (vector_engine/src/lib.rs:833-846).  Dense and Quantized are served, Auto as a STRATEGY is refused
 * with NMN_ERR_CONFIGURATION (what HNSWIndex itself offers for sparse storage — insert_sparse, insert_auto — is served on a dense
 * handle: nmn_hnsw_insert_sparse / nmn_hnsw_insert_auto below).  The strategy's home is the build options, as in the reference: it is the `storage` argument of
 * nmn_hnsw_create_with_storage (and nmn_hnsw_build_options.storage of neumann_engine.h).  nmn_hnsw_config.storage is the older
 * field: nmn_hnsw_create reads it and serves NMN_HNSW_STORAGE_DENSE only. */
#define NMN_HNSW_STORAGE_DENSE 0
#define NMN_HNSW_STORAGE_AUTO 1
#define NMN_HNSW_STORAGE_QUANTIZED 2
#define NMN_HNSW_STORAGE_BINARY 3 /* EmbeddingStorage::Binary nodes (no HNSWStorageStrategy makes them): nmn_hnsw_create_binary */

/* HNSWConfig (hnsw.rs:1434-1463). */
typedef struct nmn_hnsw_config {
    uint32_t m;                /* connections per node per layer (16) */
    uint32_t m0;               /* connections at layer 0 (2 m) */
    uint32_t ef_construction;  /* 200 */
    uint32_t ef_search;        /* 50 */
    double ml;                 /* level multiplier, 1 / ln(m) */
    uint64_t max_nodes;        /* 0 = unlimited; default 10 000 000 */
    float sparsity_threshold;  /* read by nmn_hnsw_insert_auto; every other entry carries it without acting on it */
    int32_t distance_metric;   /* HNSWDistanceMetric (hnsw.rs:135-159) = NMN_METRIC_COSINE / _EUCLIDEAN / _DOT_PRODUCT */
    int32_t storage;           /* NMN_HNSW_STORAGE_* */
    uint32_t reserved;         /* 0 */
} nmn_hnsw_config;
/* HNSWConfig::default (hnsw.rs:1465-1480), ::high_recall (1508-1519), ::high_speed (1523-1534). */
void nmn_hnsw_config_default(nmn_hnsw_config* cfg);
void nmn_hnsw_config_high_recall(nmn_hnsw_config* cfg);
void nmn_hnsw_config_high_speed(nmn_hnsw_config* cfg);

/* HNSWIndex::with_config (hnsw.rs:1578-1587) for vectors of `dim` elements (<= 8192) on `device` (-1 = current).
 * capacity_hint: rows the flat index is allocated for at first (0 = 1); it is re-created at twice the size when an insert
 * outgrows it, so the pointer nmn_hnsw_vectors returns is valid until the next nmn_hnsw_insert. */
nmn_status nmn_hnsw_create(const nmn_hnsw_config* cfg, uint32_t dim, uint64_t capacity_hint, int32_t device, nmn_hnsw** out);
nmn_status nmn_hnsw_destroy(nmn_hnsw* h);
/* HNSWIndex::insert for each of the n rows (HOST, n x dim) in order (try_insert_embedding, hnsw.rs:1936-2051): level from the
 * xorshift generator seeded 42 (1631-1651), greedy descent above it, search_layer with ef_construction per layer, the first
 * m (m0 on layer 0) of its result as neighbours, back links pruned to the closest m / m0 by a stable sort of the id-ascending
 * list (2015-2036).  ids_out (nullable, [n]) receives the node ids.  If the batch would pass max_nodes nothing is inserted:
 * NMN_ERR_CAPACITY, nmn_last_error() = "HNSW index at capacity: {current} nodes (limit: {limit})" (hnsw.rs:102-107).
 * Waits for the device searches in flight, then uploads the new adjacency. */
nmn_status nmn_hnsw_insert(nmn_hnsw* h, const float* rows_host, uint64_t n, uint64_t* ids_out);
/* HNSWIndex::insert_sparse (hnsw.rs:1660-1662) for each of the n CSR rows (HOST) in order: row i is the (position, value) pairs
 * [indptr[i], indptr[i + 1]), made a SparseVector of the handle's dimension as try_from_parts makes it — nmn_hnsw_search_sparse's
 * rules, errors and texts, checked for the whole batch before anything is inserted; duplicated positions survive in input order.
 * The node is EmbeddingStorage::Sparse: the query side scores it with s.dot_dense(q) / s.dot(Q) and s.magnitude() — single f64
 * chains over its stored entries — and the pruning side with the Sparse arms of distance_embeddings (hnsw.rs:2437-2459, 2554-2565,
 * 2637-2643), so the graph and the score bits differ from those of nmn_hnsw_insert of the densified row (docs/hnsw.md §15).  Its
 * row in nmn_hnsw_vectors(h) is to_dense() (the last entry of a duplicated position wins), node id == row as ever.  max_nodes, its
 * text and the all-or-nothing batch are nmn_hnsw_insert's.  Dense handles only: a quantized handle is NMN_ERR_CONFIGURATION.
 * Every search entry serves a handle that holds both kinds; a sparse QUERY is walked on the host when the metric is Euclidean or
 * when the query or any sparse node holds a duplicated position.  nmn_hnsw_save refuses a handle with sparse nodes. */
nmn_status nmn_hnsw_insert_sparse(nmn_hnsw* h, const uint64_t* indptr, const uint32_t* positions, const float* values, uint64_t n,
                                  uint64_t* ids_out);
/* HNSWIndex::insert_auto (hnsw.rs:1671-1680) per row (HOST, n x dim): nnz = the count of x != 0.0 (NaN counts), sparsity =
 * 1.0f - (float)nnz / (float)dim; the row is Sparse(SparseVector::from_dense(row)) iff sparsity >= cfg.sparsity_threshold (a NaN
 * threshold: never), Dense(row) otherwise.  Refusals as above. */
nmn_status nmn_hnsw_insert_auto(nmn_hnsw* h, const float* rows_host, uint64_t n, uint64_t* ids_out);
/* The stored entries of a node, in SparseVector order: *nnz = their count, UINT32_MAX for a Dense (or Quantized) node.
 * positions_out / values_out ([cap], cap >= the count: NMN_ERR_BUFFER_TOO_SMALL otherwise) may both be NULL to ask for the count. */
nmn_status nmn_hnsw_sparse_row(nmn_hnsw* h, uint64_t node, uint32_t* positions_out, float* values_out, uint32_t cap, uint32_t* nnz);
uint64_t nmn_hnsw_len(const nmn_hnsw* h);          /* HNSWIndex::len, hnsw.rs:1620-1622 */
uint32_t nmn_hnsw_dim(const nmn_hnsw* h);
uint64_t nmn_hnsw_entry_point(const nmn_hnsw* h);  /* UINT64_MAX while empty (hnsw.rs:1581) */
uint32_t nmn_hnsw_max_layer(const nmn_hnsw* h);
/* level of every node (out[len], cap >= len) and one neighbour list, id-ascending (hnsw.rs:1306-1314); a layer above the
 * node's level has count 0.  out may be null to ask for the count. */
nmn_status nmn_hnsw_levels(nmn_hnsw* h, uint32_t* out, uint64_t cap);
nmn_status nmn_hnsw_neighbors(nmn_hnsw* h, uint64_t node, uint32_t layer, uint64_t* out, uint32_t cap, uint32_t* count);
/* HNSWIndex::search_with_ef (hnsw.rs:2069-2111), ef == 0: config.ef_search.  queries HOST nq x dim; out_ids nq x k (unused =
 * UINT64_MAX), out_scores nq x k = to_similarity(distance) (hnsw.rs:152-158; unused = -inf), out_counts nq.  Empty index:
 * counts 0.  k == 0: NMN_ERR_INVALID_TOP_K.  stats: sweep_kind NMN_SWEEP_GRAPH, rows_scanned = distance evaluations,
 * fallback_queries = queries answered by the spill launch.  Synchronous.  Concurrent host callers are coalesced: a call that
 * arrives while a walk of the handle is running waits, and leaves with every other waiting call as ONE launch that carries a
 * k and an ef per query (docs/hnsw.md §11); each caller receives exactly what it would have received alone, stats included.
 * NMN_HNSW_NO_COALESCE=1 makes callers take turns instead, for A/B runs.  With the environment variable
 * NMN_HNSW_HOST_SEARCH=1 the walk runs on the host instead (the code insertion uses; no coalescing): same bits, for A/B runs. */
nmn_status nmn_hnsw_search(nmn_hnsw* h, const float* queries, uint32_t nq, uint32_t k, uint32_t ef, uint64_t* out_ids,
                           float* out_scores, uint32_t* out_counts, nmn_search_stats* stats);
/* HNSWIndex::search_with_ef (hnsw.rs:2069-2111) with a k and an ef per query, all in one launch: the walk runs with
 * ef_i = max(ef[i], k[i]) (hnsw.rs:2102) and keeps the first k[i].  ef NULL, or an entry 0: config.ef_search.  out_ids /
 * out_scores are nq x kstride (slots past the count = UINT64_MAX / -inf), out_counts nq.  Every k[i] must be in 1 .. kstride:
 * 0 is NMN_ERR_INVALID_TOP_K, above kstride NMN_ERR_INVALID_ARGUMENT, before anything is enqueued or written.  The answer for
 * query i is bit for bit what nmn_hnsw_search(h, q_i, 1, k[i], ef[i], ..) returns alone; stats are the sums of those calls'.
 * Dense and quantized handles; coalesced with concurrent callers like nmn_hnsw_search. */
nmn_status nmn_hnsw_search_multi(nmn_hnsw* h, const float* queries, uint32_t nq, const uint32_t* k, const uint32_t* ef,
                                 uint32_t kstride, uint64_t* out_ids, float* out_scores, uint32_t* out_counts,
                                 nmn_search_stats* stats);
/* HNSWIndex::search_sparse_with_ef (hnsw.rs:2118-2166; ef == 0: config.ef_search, i.e. search_sparse): the walk of
 * nmn_hnsw_search with distance_sparse (hnsw.rs:1175-1181) in place of distance_dense.  HOST buffers, CSR: query i is the
 * (position, value) pairs [indptr[i], indptr[i + 1]) of positions / values, in any order, made a SparseVector of the handle's
 * dimension as SparseVector::try_from_parts does (sparse_vector.rs:155-193) BEFORE anything is enqueued or written: a position >=
 * nmn_hnsw_dim(h) is NMN_ERR_INVALID_ARGUMENT ("index {i} out of bounds for dimension {d}"), as is a decreasing indptr; values ==
 * 0.0 (either sign) are dropped, NaN is kept, the rest is stably sorted by position, so duplicates survive in input order.
 * On a dense handle Cosine and DotProduct score a row with SparseVector::dot_dense — ONE sequential f64 sum over the query's
 * stored entries, cast to f32 — and Cosine takes the query's magnitude through f64 too (sparse_vector.rs:450-466, 548-559): the
 * score bits differ from nmn_hnsw_search of the densified query, and a row costs O(stored entries), not O(dim).  Euclidean (either
 * handle) and DotProduct on a quantized handle are bit for bit nmn_hnsw_search of Q.to_dense() (a duplicated position: the last
 * wins); Cosine on a quantized handle is that with Q.magnitude() as the query's magnitude.  docs/hnsw.md §13.
 * Outputs, sentinels, ef == 0, k == 0 (NMN_ERR_INVALID_TOP_K) and the empty index are nmn_hnsw_search's; stats: sweep_kind
 * NMN_SWEEP_GRAPH, fallback_queries = queries the spill launch answered, rows_scanned by the handle's convention for dense queries.
 * A query with more than 4096 stored entries (possible above 4096 dimensions, or with duplicates) is walked on the host.
 * Coalesced with concurrent host callers like nmn_hnsw_search, dense, metric and sparse calls in one launch that carries a query
 * kind per query (docs/hnsw.md §14); each caller receives exactly what it receives alone, stats included.  A call on a dense
 * handle under Cosine / DotProduct shares no batch when the dimension is above 4096 or one of its queries has more than 2048 stored
 * entries.  NMN_HNSW_NO_COALESCE=1 and NMN_HNSW_HOST_SEARCH=1 apply as for nmn_hnsw_search. */
nmn_status nmn_hnsw_search_sparse(nmn_hnsw* h, const uint64_t* indptr, const uint32_t* positions, const float* values,
                                  uint32_t nq, uint32_t k, uint32_t ef, uint64_t* out_ids, float* out_scores,
                                  uint32_t* out_counts, nmn_search_stats* stats);
/* nmn_hnsw_search_sparse with a k and an ef per query, all in one launch: the CSR input and its checks are
 * nmn_hnsw_search_sparse's (same errors, same texts, before anything is enqueued or written); k, ef, kstride, the outputs, their
 * padding and the refusals are nmn_hnsw_search_multi's (k[i] == 0: NMN_ERR_INVALID_TOP_K, k[i] > kstride:
 * NMN_ERR_INVALID_ARGUMENT; ef NULL, or an entry 0: config.ef_search).  The answer for query i is bit for bit what
 * nmn_hnsw_search_sparse(h, q_i, 1, k[i], ef[i], ..) returns alone; stats are the sums of those calls'.  Dense and quantized
 * handles, all three metrics; coalesced like nmn_hnsw_search_sparse; NMN_HNSW_HOST_SEARCH=1 applies. */
nmn_status nmn_hnsw_search_sparse_multi(nmn_hnsw* h, const uint64_t* indptr, const uint32_t* positions, const float* values,
                                        uint32_t nq, const uint32_t* k, const uint32_t* ef, uint32_t kstride,
                                        uint64_t* out_ids, float* out_scores, uint32_t* out_counts, nmn_search_stats* stats);
/* What the coalescer of nmn_hnsw_search / nmn_hnsw_search_multi / nmn_hnsw_search_metric / nmn_hnsw_search_metric_multi /
 * nmn_hnsw_search_sparse / nmn_hnsw_search_sparse_multi has done so far: batches that carried two or more calls, and
 * the calls in them (the meaning nmn_index_coalesce_stats and nmn_sharded_coalesce_stats give these counters). */
nmn_status nmn_hnsw_coalesce_stats(nmn_hnsw* h, uint64_t* batches, uint64_t* calls);
/* The same with every buffer in DEVICE memory: enqueued on `stream` (NULL: the default stream), not waited for.  Two kernel
 * launches per chunk of queries (the walk with both heaps in LDS, then the spill launch for the queries whose candidate
 * heap outgrew LDS), nothing is read back; a shape the stream has served before allocates nothing.  nmn_hnsw_insert and
 * nmn_hnsw_destroy wait for the searches in flight. */
nmn_status nmn_hnsw_search_device(nmn_hnsw* h, const float* queries_dev, uint32_t nq, uint32_t k, uint32_t ef,
                                  uint64_t* out_ids_dev, float* out_scores_dev, uint32_t* out_counts_dev, void* stream);
/* SparseVector::try_from_parts (sparse_vector.rs:155-193), magnitude (548-559) and to_dense (400-406) of nq CSR queries that sit
 * in DEVICE memory, bit for bit what nmn_hnsw_search_sparse makes of them on the host (docs/hnsw.md §22): indptr_dev [nq + 1],
 * positions_dev / values_dev [nnz_total].  nnz_total and max_nnz are HOST scalars: the entries the two arrays hold, and the
 * caller's bound on the raw entries of one query — at most 4096 (above: NMN_ERR_INVALID_ARGUMENT), 0 = min(dim, 4096); dim is
 * 1 .. 8192.  Per query: entries with val == 0.0 (either sign) dropped, NaN kept, the rest stably sorted by position (duplicates
 * survive in input order).  out_off_dev [nq + 1]: the kept entries of query q are [off[q], off[q + 1]) of out_entries_dev
 * [nnz_total][2], pairs of {position, value bits}; out_mag_dev [nq]: ONE f64 chain from -0.0 over the kept values in that order,
 * one f64 sqrt, one cast; out_dup_dev [nq] (nullable): 1 iff two kept entries share a position; out_dense_dev [nq][dim]
 * (nullable): zeros, then the entries in order, the last of a duplicated position wins.  out_status_dev [nq], the first rule that
 * fails: 2 — indptr[q + 1] < indptr[q], the range not within the nnz_total entries, or more than max_nnz raw entries; 1 — a raw
 * entry whose position is >= dim (checked before its value is looked at); 0 — served.  A query with a status is canonicalised as
 * the entry-less query: count 0, that query's magnitude, a zero row.  Whatever the arrays hold, nothing outside them is read or
 * written (a query whose kept entries no longer fit out_entries_dev, possible only where ranges overlap behind a decreasing
 * indptr, is status 2 as well).  Three launches on `stream` of `device` (negative: the current one), not waited for, nothing read
 * back. */
nmn_status nmn_sparse_canonicalise_device(uint32_t dim, const uint64_t* indptr_dev, const uint32_t* positions_dev,
                                          const float* values_dev, uint32_t nq, uint64_t nnz_total, uint32_t max_nnz,
                                          uint64_t* out_off_dev, uint32_t* out_entries_dev, float* out_mag_dev, uint32_t* out_dup_dev,
                                          float* out_dense_dev, uint32_t* out_status_dev, int32_t device, void* stream);
/* nmn_hnsw_search_sparse with the CSR and every output in DEVICE memory, under nmn_hnsw_search_device's contract: enqueued on
 * `stream`, not waited for, nothing read back, a shape the stream has served before allocates nothing; nmn_hnsw_insert and
 * nmn_hnsw_destroy wait for it.  The CSR, nnz_total and max_nnz are nmn_sparse_canonicalise_device's, whose three launches run in
 * front of the walk's; the walk is routed as nmn_hnsw_search_sparse routes it, and a served query's ids, score bits and count are
 * that entry's.  out_status_dev [nq] (nullable): 0 served, 1 / 2 as above, 3 — a query with a duplicated position on a handle
 * with sparse nodes (only the device knows it has one; the host entry walks it on the host).  A query with a status is walked as
 * the entry-less query and a closing launch makes its row count 0, ids UINT64_MAX, scores -inf; the other rows are untouched.
 * k == 0, nq == 0, ef == 0 and the empty index are nmn_hnsw_search_sparse's.  NMN_ERR_CONFIGURATION before anything is enqueued
 * or written, because the host entry answers these from the host: a Binary handle; a handle with sparse nodes under Euclidean; a
 * handle with a sparse node that holds a duplicated position.  On every other handle duplicated positions are served. */
nmn_status nmn_hnsw_search_sparse_device(nmn_hnsw* h, const uint64_t* indptr_dev, const uint32_t* positions_dev,
                                         const float* values_dev, uint32_t nq, uint64_t nnz_total, uint32_t max_nnz, uint32_t k,
                                         uint32_t ef, uint64_t* out_ids_dev, float* out_scores_dev, uint32_t* out_counts_dev,
                                         uint32_t* out_status_dev, void* stream);
/* Entries of the results / candidate heaps a wave keeps in LDS (0 = default: 1024 results, 1024 .. 4096 candidates by ef).
 * Smaller heaps leave more LDS per workgroup; a query that outgrows them is answered by the spill launch, same bits. */
nmn_status nmn_hnsw_set_heap_capacity(nmn_hnsw* h, uint32_t results, uint32_t candidates);
/* nmn_hnsw_insert with the searches of try_insert_embedding (hnsw.rs:1936-2051) walked on the GPU, many new nodes per launch
 * (docs/hnsw.md §19).  The levels of all n rows are drawn first, in order; then batches of consecutive nodes are walked against
 * the graph as it is at launch, and the host commits them in order (the same connect-and-prune code), taking a node's device walk
 * only when no neighbour list that walk read has been assigned since the launch, and walking the node itself otherwise.  The
 * graph, the ids and the generator state are nmn_hnsw_insert's, list for list; arguments, NMN_ERR_CAPACITY, its text and the
 * all-or-nothing batch are nmn_hnsw_insert's too.  Walked on the device: a dense handle without sparse nodes, ef_construction
 * <= 1024, a results heap (nmn_hnsw_set_heap_capacity) of at least ef_construction + 1 entries, once the graph holds min_nodes
 * nodes, in a call that leaves the device at least four rows; every other node takes the host's walk, with the same result.  A device error during a batch sends the remaining rows of
 * the call down the host's path.  NMN_HNSW_BULK_BUILD=1 (read at every call) routes nmn_hnsw_insert through this entry. */
nmn_status nmn_hnsw_insert_bulk(nmn_hnsw* h, const float* rows_host, uint64_t n, uint64_t* ids_out);
/* How nmn_hnsw_insert_bulk (hnsw.rs:1936-2051 in batches) cuts its batches; never what it builds.  batch: nodes per launch, 1 ..
 * 1024 (a batch also ends behind the first node whose level exceeds the graph's top layer); 0 = adaptive, from 8, doubled up to 256
 * after a batch of which at most a quarter was walked again on the host, halved down to 4 after one of which half or more was.
 * min_nodes: the graph size from which the device walks (0 = 100 000, below which the host's walk was measured faster). */
nmn_status nmn_hnsw_set_bulk_policy(nmn_hnsw* h, uint32_t batch, uint32_t min_nodes);
/* Counters of nmn_hnsw_insert_bulk (hnsw.rs:1936-2051 in batches), cumulative per handle: launches; nodes walked on the device;
 * of those, the walks taken (accepted), walked again because a list they read had been assigned (conflicts) or because the
 * candidate heap or the read list filled (overflowed) — accepted + conflicts + overflowed == walks; nodes that never went to the
 * device (host_nodes); neighbour lists sent to the device between batches (patched_lists). */
typedef struct nmn_hnsw_bulk_stats {
    uint64_t batches;
    uint64_t walks;
    uint64_t accepted;
    uint64_t conflicts;
    uint64_t overflowed;
    uint64_t host_nodes;
    uint64_t patched_lists;
} nmn_hnsw_bulk_stats;
nmn_status nmn_hnsw_get_bulk_stats(nmn_hnsw* h, nmn_hnsw_bulk_stats* out);
/* The batches of the LAST nmn_hnsw_insert_bulk call (hnsw.rs:1936-2051 in batches), five floats each: nodes walked, nodes walked
 * again on the host, milliseconds of the walk launch (with its read-back), of validation and commits, of the patch.  *count
 * receives the number of batches; out (nullable) the first min(cap, *count) records. */
nmn_status nmn_hnsw_get_bulk_trace(nmn_hnsw* h, float* out, uint64_t cap, uint64_t* count);
/* The flat index holding the rows (exhaustive search over the same rows).  NULL on a quantized or binary handle: it keeps no f32
 * rows on the device. */
nmn_index* nmn_hnsw_vectors(nmn_hnsw* h);
/* Device memory the index holds: rows, magnitudes, mirrors, adjacency (dense; with sparse nodes also a 16-byte record per node
 * and 8 bytes per stored entry); codes, records, adjacency (quantized); words, adjacency (binary); the live mask, one bit per
 * node. */
uint64_t nmn_hnsw_hbm_bytes(nmn_hnsw* h);

/* nmn_hnsw_create with the storage strategy of HNSWBuildOptions: `storage` is NMN_HNSW_STORAGE_*, cfg->storage is not read.
 * DENSE is exactly nmn_hnsw_create.  QUANTIZED: nmn_hnsw_insert is insert_quantized (hnsw.rs:1711-1714) — every row becomes a
 * ScalarQuantizedVector (from_dense, 324-356: scale (max - min) / 255, or 1.0 below f32::EPSILON; codes rounded half away from
 * zero), resident in HBM as n x ld8 codes (ld8 = dim rounded up to 16) and one 16-byte record {scale, min_val, magnitude,
 * squared_magnitude} per row.  Searches and insertion score a row against a query by dot_dense / euclidean_distance_dense /
 * the cosine of EmbeddingStorage (414-527, 1035-1045) on the codes; pruning dequantizes both rows (2489-2500, 2585-2589,
 * 2662-2666).  Same graph, ids and score bits as the reference.  nmn_hnsw_vectors is NULL and nmn_hnsw_search_metric* are
 * refused with NMN_ERR_CONFIGURATION (they re-rank with the f32 rows of nmn_hnsw_vectors); every other entry works unchanged.
 * AUTO: NMN_ERR_CONFIGURATION.  A handle has one strategy. */
nmn_status nmn_hnsw_create_with_storage(const nmn_hnsw_config* cfg, int32_t storage, uint32_t dim, uint64_t capacity_hint,
                                        int32_t device, nmn_hnsw** out);
int32_t nmn_hnsw_storage(const nmn_hnsw* h); /* NMN_HNSW_STORAGE_DENSE, _QUANTIZED or _BINARY */
/* A handle whose every node is EmbeddingStorage::Binary(BinaryVector::from_dense(row, threshold)) (hnsw.rs:579;
 * binary_quantization.rs:83-99), inserted as insert_embedding does; `binary_threshold` is NMN_BINARY_SIGN / _MEAN / _MEDIAN.
 * nmn_hnsw_create_with_storage(.., NMN_HNSW_STORAGE_BINARY, ..) is the same with Sign.  A row is one bit per dimension, resident
 * in HBM as n x ldw u64 words (ldw = ceil(dim / 64) rounded up to 2: 16-byte rows, the padding zero) beside the adjacency; no f32
 * rows and no record per row live on the device, nmn_hnsw_vectors is NULL.  Searches and insertion score a row against a query on
 * to_dense(), +1.0 for a set bit and -1.0 otherwise (157-166): simd::dot_product / euclidean_distance, and under Cosine
 * 1 - dot / (sqrt(dim as f32) * |q|) (hnsw.rs:801-805, 981-984, 1098-1101); pruning under Cosine is the Hamming formula
 * 1 - (1 - hamming / dim) (2516-2518), under Euclidean / DotProduct the dense arithmetic on both to_dense() rows.  Same graph,
 * ids and score bits as the reference (docs/hnsw.md §18).  Served: nmn_hnsw_insert, nmn_hnsw_search, _search_multi,
 * _search_device, the accessors.  Refused with NMN_ERR_CONFIGURATION: nmn_hnsw_search_metric*, _search_sparse*, _search_tt*,
 * _cache_search*, _set_node_mask, _insert_sparse / _auto / _tt, _quantized_row, _save. */
nmn_status nmn_hnsw_create_binary(const nmn_hnsw_config* cfg, int32_t binary_threshold, uint32_t dim, uint64_t capacity_hint,
                                  int32_t device, nmn_hnsw** out);
int32_t nmn_hnsw_binary_threshold(const nmn_hnsw* h); /* NMN_BINARY_*; -1 when the handle's storage is not Binary */
/* The BinaryVector of a node: words_out[ceil(dim / 64)] (nullable; cap_words = its capacity), padding bits zero.  Any other
 * handle: NMN_ERR_CONFIGURATION. */
nmn_status nmn_hnsw_binary_row(nmn_hnsw* h, uint64_t node, uint64_t* words_out, uint32_t cap_words);
/* The ScalarQuantizedVector of a node: codes_out[dim], scale, min_val (each nullable).  Dense handle: NMN_ERR_CONFIGURATION. */
nmn_status nmn_hnsw_quantized_row(nmn_hnsw* h, uint64_t node, uint8_t* codes_out, float* scale, float* min_val);
/* HNSWIndex::get_vector: out[dim] = the row as inserted (dense), to_dense() of a sparse node, or dequantize() =
 * code.mul_add(scale, min_val) (quantized), or to_dense() = +1.0 / -1.0 per bit (binary). */
nmn_status nmn_hnsw_get_vector(nmn_hnsw* h, uint64_t node, float* out);
/* HNSWMemoryStats (hnsw.rs:2733-2768); embedding_bytes = 4 dim per dense node, 16 + dim per quantized node, 8 ceil(dim / 64)
 * per binary node (binary_quantization.rs:174-179), 56 + 8 nnz per sparse node (size_of::<SparseVector>() on a 64-bit target plus both Vec capacities taken as their lengths — what a cloned
 * vector has; std does not pin the capacity of a pushed one, docs/hnsw.md §15). */
typedef struct nmn_hnsw_memstats {
    uint64_t total_nodes;
    uint64_t dense_count;
    uint64_t sparse_count;
    uint64_t delta_count;
    uint64_t tt_count;
    uint64_t quantized_count;
    uint64_t pq_count;
    uint64_t binary_count;
    uint64_t embedding_bytes;
} nmn_hnsw_memstats;
nmn_status nmn_hnsw_memory_stats(nmn_hnsw* h, nmn_hnsw_memstats* out);
/* The handle's HNSWConfig; `storage` = the handle's strategy (nmn_hnsw_storage), `reserved` 0.  What nmn_hnsw_load read from a file. */
nmn_status nmn_hnsw_get_config(const nmn_hnsw* h, nmn_hnsw_config* out);

/* ---- tensor-train vectors: TT queries and insert_tt_vector (docs/hnsw.md §17) ----------------------------------------- */

/* A TTVector (tensor_compress/src/tensor_train.rs:267-281) crosses this interface as its parts.  One call carries nq trains of
 * ONE shape: shape[n_cores], ranks [nq][n_cores + 1] (a row per train), and one flat `cores` array into which core_off[nq + 1]
 * indexes: train q is cores[core_off[q] .. core_off[q + 1]), its cores back to back, core k being ranks[k] x shape[k] x ranks[k + 1]
 * floats, row-major, as TTCore::get indexes them (tensor_train.rs:240-243).  A train is well formed when n_cores is in 1..8, every
 * shape[k] >= 1, every rank >= 1, ranks[0] == ranks[n_cores] == 1, and core_off[q + 1] - core_off[q] is the sum of the core sizes;
 * the product of the shape (2^31 at most) is the vector's dimension.  Anything else is NMN_ERR_INVALID_ARGUMENT before anything is
 * enqueued or written, the text naming the query and the rule (the reference's panics and ignored tails are not restated).
 *
 * nmn_tt_reconstruct: out_rows[nq][dim] = tt_reconstruct (tensor_train.rs:401-436) of every train, bit for bit.
 * nmn_tt_norm: out_norms[nq] = tt_norm (440-474), the raw norm, bit for bit.
 * HOST buffers, synchronous, stateless, on the current device: one launch, a workgroup per train with everything in LDS.  A train
 * above the LDS limits (nmn_tt_limits: a rank above max_rank, more than max_storage core floats, or an intermediate level
 * shape[0] .. shape[k] x ranks[k + 1] above max_level floats) is prepared by the host restatement of the same loops, same bits;
 * NMN_HNSW_HOST_SEARCH=1 sends every train there. */
nmn_status nmn_tt_reconstruct(const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks, const uint64_t* core_off,
                              const float* cores, uint32_t nq, float* out_rows);
nmn_status nmn_tt_norm(const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks, const uint64_t* core_off, const float* cores,
                       uint32_t nq, float* out_norms);
nmn_status nmn_tt_limits(uint32_t* max_cores, uint32_t* max_rank, uint32_t* max_storage, uint32_t* max_level); /* each nullable */

/* HNSWIndex::search_tt_with_ef (hnsw.rs:1811-1841) per train: query_norm = tt_norm once, then search_layer_greedy_tt (2238-2272)
 * and search_layer_tt_native (1845-1903) with cosine_distance_tt_with_norm (1196-1221) — on a Dense, Sparse or Quantized node
 * 1 - dot_with_tt / (magnitude() * query_norm) with the query reconstructed (919-948), 1.0 when query_norm < 1e-10 or the node's
 * magnitude is 0.  The metric is Cosine WHATEVER the handle's distance_metric is, and the score is 1 - distance.  The trains are
 * prepared on the GPU (nmn_tt_reconstruct's kernel, one launch for the call) and walked by the kernel of nmn_hnsw_search with the
 * query's magnitude given.  The product of the shape must be nmn_hnsw_dim(h) (NMN_ERR_DIMENSION_MISMATCH).  HOST buffers,
 * synchronous; outputs, sentinels, ef == 0, k == 0 and the empty index are nmn_hnsw_search's; stats by the handle's convention.
 * Dense handles (sparse nodes included, under every metric) and quantized handles.  Not coalesced: concurrent callers take turns.
 * NMN_HNSW_HOST_SEARCH=1: host preparation and host walk, same bits.  A train whose norm is NaN is walked by the host. */
nmn_status nmn_hnsw_search_tt(nmn_hnsw* h, const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks, const uint64_t* core_off,
                              const float* cores, uint32_t nq, uint32_t k, uint32_t ef, uint64_t* out_ids, float* out_scores,
                              uint32_t* out_counts, nmn_search_stats* stats);
/* The same with the core data, the queries and the results in DEVICE memory, enqueued on `stream` and not waited for, nothing read
 * back (nmn_hnsw_search_device's contract).  ONE rank vector ranks[n_cores + 1] for the whole call, HOST memory, read before the
 * call returns; cores_dev is [nq][storage], storage = the sum of the core sizes.  The preparation runs on `stream` in front of the
 * walk, into the stream's scratch.  A train above the LDS limits is NMN_ERR_INVALID_ARGUMENT (there is no host to fall back to).
 * A train whose norm is NaN gives NaN distances, which the heaps do not order: its row of the outputs is unspecified. */
nmn_status nmn_hnsw_search_tt_device(nmn_hnsw* h, const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks,
                                     const float* cores_dev, uint32_t nq, uint32_t k, uint32_t ef, uint64_t* out_ids_dev,
                                     float* out_scores_dev, uint32_t* out_counts_dev, void* stream);
/* HNSWIndex::insert_tt_vector (hnsw.rs:1755-1759) for each of the n trains in order: the batch is reconstructed
 * (nmn_tt_reconstruct) and takes nmn_hnsw_insert's path — Dense nodes; max_nodes, its text and the all-or-nothing batch are that
 * entry's.  Dense handles only: a quantized handle is NMN_ERR_CONFIGURATION. */
nmn_status nmn_hnsw_insert_tt(nmn_hnsw* h, const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks, const uint64_t* core_off,
                              const float* cores, uint64_t n, uint64_t* ids_out);

/* ---- EmbeddingStorage::TensorTrain nodes (docs/hnsw.md §24) -------------------------------------------------------------- */

/* HNSWIndex::insert_embedding(EmbeddingStorage::from(tt)) (hnsw.rs:1256-1259, 1913-2051) for each of the n trains in order:
 * TensorTrain(TTVectorCached) nodes, which keep the train and norm = tt_norm(tt) (276-289) — NOT what nmn_hnsw_insert_tt makes.
 * The trains cross as they do there; validation, its texts, max_nodes and the all-or-nothing batch are that entry's, and the
 * product of the shape must be nmn_hnsw_dim(h) (NMN_ERR_DIMENSION_MISMATCH).  Calls may bring different shapes of that product:
 * every node keeps its own.  Dense handles only: quantized and binary handles are NMN_ERR_CONFIGURATION.  Like nmn_hnsw_insert,
 * the entry tests no row for finiteness: a train whose reconstruction holds a NaN or an infinity is inserted as it is.
 * Such a node is scored (a) by a dense or sparse query as a Dense node of its reconstruction, with the cached tt_norm as its
 * magnitude under Cosine; (b) by a TT query as 1 - tt_dot_product(node, query) / (node.norm * query_norm), 1.0 when a norm is
 * below 1e-10 or the shapes differ, nothing reconstructed; (c) in pruning, T x T under Cosine by the dot of the reconstructions over
 * the cached norms (1.0 when one is below 1e-10), every other arm by the Dense / Sparse arithmetic on the reconstruction with
 * simd::magnitude.  nmn_hnsw_get_vector returns tt_reconstruct; nmn_hnsw_memory_stats counts tt_count and 4 storage_size() bytes;
 * nmn_hnsw_save refuses such a handle (NMN_ERR_CONFIGURATION) before the file is touched; nmn_hnsw_insert_bulk walks on the host. */
nmn_status nmn_hnsw_insert_embedding_tt(nmn_hnsw* h, const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks,
                                        const uint64_t* core_off, const float* cores, uint64_t n, uint64_t* ids_out);
/* get_embedding of a TensorTrain node: *storage = the floats of its cores, UINT64_MAX for a node that is not a TT node.  Every
 * array is nullable: shape_out [8], *n_cores_out, ranks_out [9], cores_out [cap] (cap >= *storage: NMN_ERR_BUFFER_TOO_SMALL otherwise). */
nmn_status nmn_hnsw_tt_row(nmn_hnsw* h, uint64_t node, uint32_t* shape_out, uint32_t* n_cores_out, uint32_t* ranks_out, float* cores_out,
                           uint64_t cap, uint64_t* storage);
/* The limits of the device walk of TT queries on a handle with TensorTrain nodes, each output nullable: the largest rank of any TT
 * node; the TT nodes above nmn_tt_limits (max_rank, max_storage) — with any, every TT query walks on the host; and the floats of
 * LDS a call with this ef (0: ef_search) may spend on (its largest train's cores + 2 x max_node_rank x its largest rank).  A call
 * above them: nmn_hnsw_search_tt walks on the host with the same bits, nmn_hnsw_search_tt_device is NMN_ERR_INVALID_ARGUMENT. */
nmn_status nmn_hnsw_tt_walk_limits(nmn_hnsw* h, uint32_t ef, uint32_t* max_node_rank, uint64_t* nodes_above_limits, uint32_t* lds_floats);

/* ---- tt_decompose: from a dense vector and a TTConfig to a train (docs/hnsw.md §21) --------------------------------------- */

/* A TTConfig (tensor_train.rs:41-49) crosses this interface as its parts: shape[n_cores], max_rank, tolerance.
 * nmn_tt_config_for_dim: TTConfig::for_dim, ::high_compression and ::high_accuracy (tensor_train.rs:77-126) with optimal_shape and
 * factorize_balanced (130-199; the f64 log2 and pow are the host libm's).  shape_out holds up to 8 modes.  dim == 0 is the
 * reference's EmptyVector: NMN_ERR_INVALID_ARGUMENT, "empty vector". */
#define NMN_TT_PRESET_FOR_DIM 0u          /* max_rank 8,  tolerance 1e-4 */
#define NMN_TT_PRESET_HIGH_COMPRESSION 1u /* max_rank 4,  tolerance 1e-2 */
#define NMN_TT_PRESET_HIGH_ACCURACY 2u    /* max_rank 16, tolerance 1e-6 */
nmn_status nmn_tt_config_for_dim(uint64_t dim, uint32_t preset, uint32_t* shape_out, uint32_t* n_cores_out, uint32_t* max_rank_out,
                                 float* tolerance_out);
/* The slot of one train under a config, in floats: the sum of b[k] * shape[k] * b[k + 1] over the worst-case ranks b[0] = 1,
 * b[k + 1] = min(max_rank, b[k] * shape[k], shape[k + 1] * .. * shape[n_cores - 1]), b[n_cores] = 1.  No train tt_decompose
 * returns under the config is larger.  0 for a config the entries below refuse. */
uint64_t nmn_tt_max_storage(const uint32_t* shape, uint32_t n_cores, uint32_t max_rank);

/* Per-vector status of nmn_tt_decompose */
#define NMN_TT_OK 0u           /* Ok(TTVector) */
#define NMN_TT_EMPTY_MATRIX 1u /* Err(TTError::Decompose(DecomposeError::EmptyMatrix)): a step's rank was 0 with another SVD to come */

/* tt_decompose (tensor_compress/src/tensor_train.rs:315-397) of n vectors of `dim` floats under one config, bit for bit: the TT-SVD
 * sweep over left_unfold_for_tt (decompose.rs:559-570), svd_truncated (398-466: power iteration with deflation, 470-550 and
 * 344-387, or the randomized range finder with gaussian_matrix 271-294 and qr_orthonormalize 298-340), matmul (197-216), dot, norm
 * and normalize (220-239), frobenius_norm (76-78) — every product and sum in the reference's order and rounding.  The three
 * argument errors of tt_decompose refuse the whole call with NMN_ERR_INVALID_ARGUMENT and the reference's Display text: dim == 0
 * ("empty vector"), a shape whose product is not dim ("dimension D cannot be reshaped to [..] (product: P)") and max_rank < 1
 * ("invalid TT-rank: must be >= 1"); so does an n_cores outside 1..8 (this library's).  The tolerance is not checked, as
 * tt_decompose does not check it.  EmptyMatrix is a status of one vector, not a failure of the call.
 * status_out[n]; ranks_out[n][n_cores + 1] (all 0 where the status is not NMN_TT_OK; a two-core train may carry ranks {1, 0, 1});
 * cores_out (nullable: status and ranks only) receives the trains of the Ok vectors back to back, core_off_out[n + 1] indexing them
 * as nmn_tt_reconstruct, nmn_tt_norm and nmn_hnsw_search_tt take them (a failed vector has an empty range).  cores_cap is in floats:
 * n * nmn_tt_max_storage always suffices, less is NMN_ERR_INVALID_ARGUMENT only if the trains do not fit (nothing is written then).
 * HOST buffers, synchronous, stateless, on the current device: one launch, a wave per vector with the vector's whole state in LDS.
 * The host restatement of the same loops (same bits) takes a call whose config is above the device's limits
 * (nmn_tt_decompose_lds_floats), a call of fewer than NMN_TT_DECOMPOSE_MIN vectors (environment, read at every call; default 320,
 * the measured crossover against the host's 16 threads) and every call under NMN_HNSW_HOST_SEARCH=1.  The choice never depends on the vectors.
 * NaN and infinite inputs are not refused and are outside the bit-level promise. */
nmn_status nmn_tt_decompose(const float* vectors, uint64_t n, uint64_t dim, const uint32_t* shape, uint32_t n_cores, uint32_t max_rank,
                            float tolerance, uint32_t* status_out, uint32_t* ranks_out, uint64_t* core_off_out, float* cores_out,
                            uint64_t cores_cap);
/* The same with the vectors and every output in DEVICE memory, enqueued on `stream` and not waited for, nothing read back.  The
 * trains stay in their slots: train q starts at q * nmn_tt_max_storage (cores_cap >= n * that), core_off_dev[n + 1] (nullable)
 * receives q * nmn_tt_max_storage, ranks_dev carries each train's own ranks — what tt_prepare's per-query ranks read.  cores_dev
 * nullable: status and ranks only.  There is no host to fall back to: a config above the limits is NMN_ERR_INVALID_ARGUMENT.  The
 * first call of a config on a device uploads its Gaussian matrices (made on the host, kept for the life of the process). */
nmn_status nmn_tt_decompose_device(const float* vectors_dev, uint64_t n, uint64_t dim, const uint32_t* shape, uint32_t n_cores,
                                   uint32_t max_rank, float tolerance, uint32_t* status_dev, uint32_t* ranks_dev,
                                   uint64_t* core_off_dev, float* cores_dev, uint64_t cores_cap, void* stream);
/* What the device path serves: at most max_cores modes, no worst-case rank above max_rank, and a config whose LDS need
 * (nmn_tt_decompose_lds_floats: the unfolding, U, V, the u and v columns and, where a step can take the randomized path, the
 * Gaussian matrix, Q and B — sized from the worst-case ranks, never from a vector) is at most max_lds_floats; max_dim is the largest
 * dimension any shape can bring under that.  Each pointer nullable. */
nmn_status nmn_tt_decompose_limits(uint32_t* max_cores, uint32_t* max_rank, uint32_t* max_dim, uint32_t* max_lds_floats);
/* The LDS floats a config needs on the device; UINT64_MAX for a config above the limits, 0 for one the entries refuse */
uint64_t nmn_tt_decompose_lds_floats(const uint32_t* shape, uint32_t n_cores, uint32_t max_rank);

/* ---- tt_dot_product, tt_cosine_similarity, tt_euclidean_distance: trains compared without reconstruction (docs/hnsw.md §23) - */

#define NMN_TT_SIM_DOT 0u       /* tt_dot_product (tensor_train.rs:480-516) */
#define NMN_TT_SIM_COSINE 1u    /* tt_cosine_similarity (522-532): 0.0 when either tt_norm is < 1e-10, else dot / (norm_a * norm_b) */
#define NMN_TT_SIM_EUCLIDEAN 2u /* tt_euclidean_distance (539-546): sqrt(max(fma(-2, dot_ab, dot_aa + dot_bb), 0)); a NaN gives 0.0 */

/* out[nq][nt]: out[i][j] = the reference's function of (query i, target j), in that argument order, bit for bit — the Gram
 * contraction new_gram[x r2b + y] = one chain from +0.0 over k, ia, ib of sum + ((gram[ia r1b + ib] * A[ia,k,x]) * B[ib,k,y]), every
 * product and add rounded on its own; tt_dot_product(a, b) and tt_dot_product(b, a) differ in bits, and so do both from the dense
 * dot of the reconstructions.  Each set crosses as nmn_tt_norm's arguments and is checked by its rules (NMN_ERR_INVALID_ARGUMENT,
 * the text naming the set, the train and the rule); sets whose n_cores or modes differ are the reference's IncompatibleShapes:
 * NMN_ERR_INVALID_ARGUMENT, "incompatible TT shapes for operation" (the batch forms of the reference fail as a whole in the same
 * way); an unknown op is NMN_ERR_INVALID_ARGUMENT.  Nothing is written on any error; nq == 0 or nt == 0 returns NMN_OK and writes
 * nothing.  tt_dot_product(t, t) — the chain tt_norm runs before its square root — is computed once per train per call, never once
 * per pair.  HOST buffers, synchronous, stateless, on the current device: a workgroup stages one query's cores in LDS, each of its
 * waves walks one (query, target) pair at a time, the lanes sharing out the outputs of a Gram matrix; no chain is split.  A pair
 * with a train above nmn_tt_limits (max_cores, max_rank, max_storage; max_level does not apply) is computed by the host
 * restatement of the same loops, same bits; so is every pair under NMN_HNSW_HOST_SEARCH=1 and every call of fewer than
 * NMN_TT_SIMILARITY_MIN pairs (environment, read at every call; default 32, the measured crossover).  The choice never depends on a core's value. */
nmn_status nmn_tt_similarity(uint32_t op, const uint32_t* shape_q, uint32_t n_cores_q, const uint32_t* ranks_q,
                             const uint64_t* core_off_q, const float* cores_q, uint32_t nq, const uint32_t* shape_t,
                             uint32_t n_cores_t, const uint32_t* ranks_t, const uint64_t* core_off_t, const float* cores_t, uint32_t nt,
                             float* out);
/* out[i] = tt_dot_product(t_i, t_i); sqrt(out[i]) has the bits of nmn_tt_norm.  HOST buffers, nmn_tt_similarity's checks and routing
 * (NMN_TT_SIMILARITY_MIN counts trains here). */
nmn_status nmn_tt_self_dot(const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks, const uint64_t* core_off, const float* cores,
                           uint32_t n, float* out);
/* The same with every array but `shape` in DEVICE memory, enqueued on `stream` and not waited for, nothing read back, nothing
 * allocated — the layout nmn_tt_decompose_device leaves: ranks_dev [n][n_cores + 1] per train; train i's cores at core_off_dev[i]
 * (core_off_dev [n + 1]) or, when core_off_dev is null, at i * stride; no train holds more than `stride` floats (its slot:
 * nmn_tt_max_storage of the config) and cores_dev holds n * stride floats; status_dev [n] nullable (nmn_tt_decompose_device's).
 * n_cores above 8, a mode of 0 and a stride of 0 or above nmn_tt_limits' max_storage are NMN_ERR_INVALID_ARGUMENT: there is no host
 * to fall back to.  The ranks cannot be checked by the host, so the kernel checks them before it reads through them.  A train is
 * BAD when its status is not NMN_TT_OK, ranks[0] or ranks[n_cores] is not 1, a rank is 0 or above nmn_tt_limits' max_rank, its
 * core floats are more than `stride` (or than core_off_dev[i + 1] - core_off_dev[i]), or they would leave the n * stride floats of
 * cores_dev.  A bad train leaves the quiet NaN 0x7FC00000 in every output it takes part in; no load or store leaves the buffers
 * described here. */
nmn_status nmn_tt_self_dot_device(const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks_dev, const uint64_t* core_off_dev,
                                  const float* cores_dev, uint64_t stride, const uint32_t* status_dev, uint32_t n, float* out_dev,
                                  void* stream);
/* nmn_tt_similarity on two sets in DEVICE memory, each as nmn_tt_self_dot_device takes it: out_dev[nq][nt].  self_q_dev [nq] and
 * self_t_dev [nt] are what nmn_tt_self_dot_device wrote for the sets — required for NMN_TT_SIM_COSINE and NMN_TT_SIM_EUCLIDEAN,
 * ignored for NMN_TT_SIM_DOT — so targets that stay resident pay for their self dots once, not once per call (TTVectorCached,
 * tensor_store/src/hnsw.rs:276-289).  Enqueued on `stream`, not waited for, nothing read back, nothing allocated. */
nmn_status nmn_tt_similarity_device(uint32_t op, const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks_q_dev,
                                    const uint64_t* core_off_q_dev, const float* cores_q_dev, uint64_t stride_q,
                                    const uint32_t* status_q_dev, uint32_t nq, const uint32_t* ranks_t_dev,
                                    const uint64_t* core_off_t_dev, const float* cores_t_dev, uint64_t stride_t,
                                    const uint32_t* status_t_dev, uint32_t nt, const float* self_q_dev, const float* self_t_dev,
                                    float* out_dev, void* stream);

/* HNSWIndex::search_tt (hnsw.rs:1796-1801) per query: tt_decompose(query, config); Ok: search_tt_with_ef(tt, k, ef_search) — what
 * nmn_hnsw_search_tt returns for the train nmn_tt_decompose makes, Cosine whatever the handle's metric; Err of any kind:
 * search(query, k) — what nmn_hnsw_search returns, under the handle's metric.  The three argument errors of tt_decompose therefore
 * make the whole call a plain dense search.  queries[nq][dim], dim == nmn_hnsw_dim(h) (NMN_ERR_DIMENSION_MISMATCH).  Divergence: a
 * two-core train whose middle rank is 0 is Ok in the reference (its tt_norm is 0, so every distance is 1.0); here it is
 * refused as nmn_hnsw_search_tt refuses it, NMN_ERR_INVALID_ARGUMENT "TT: query Q: every rank must be >= 1", before anything is
 * written.  HOST buffers, synchronous; the decomposition is nmn_tt_decompose's (its routing), the two searches are those entries'
 * (their handles, storages and host routing), each with its own wait; stats are the sums of the two.  There is no device-buffer
 * form: the fallback rule cannot be honoured without reading the status back (docs/hnsw.md §21). */
nmn_status nmn_hnsw_search_tt_dense(nmn_hnsw* h, const float* queries, uint32_t nq, uint64_t dim, const uint32_t* shape,
                                    uint32_t n_cores, uint32_t max_rank, float tolerance, uint32_t k, uint64_t* out_ids,
                                    float* out_scores, uint32_t* out_counts, nmn_search_stats* stats);
/* HNSWIndex::insert_tt (hnsw.rs:1740-1749) and insert_batch_tt (1769-1790): every vector is decomposed (status only); if any
 * decomposition is an Err nothing is inserted and the call is NMN_ERR_INVALID_ARGUMENT with the reference's text,
 * "TT decomposition failed: {e:?}" or "Batch TT decomposition failed: {e:?}" with the Debug form of the TTError (EmptyVector,
 * ShapeMismatch { dim: .., shape: [..], product: .. }, InvalidRank, Decompose(EmptyMatrix)); the batch's text is followed by
 * " (vector I)", I the lowest failing index — the reference's sequential branch reports exactly that one, its rayon branch any.
 * Otherwise the vectors take nmn_hnsw_insert's path as Dense nodes: max_nodes, its text and the all-or-nothing batch are that
 * entry's.  Dense handles only: a quantized or binary handle is NMN_ERR_CONFIGURATION.  An empty batch returns NMN_OK and no ids. */
nmn_status nmn_hnsw_insert_tt_dense(nmn_hnsw* h, const float* vector, uint64_t dim, const uint32_t* shape, uint32_t n_cores,
                                    uint32_t max_rank, float tolerance, uint64_t* id_out);
nmn_status nmn_hnsw_insert_batch_tt(nmn_hnsw* h, const float* vectors, uint64_t n, uint64_t dim, const uint32_t* shape,
                                    uint32_t n_cores, uint32_t max_rank, float tolerance, uint64_t* ids_out);

/* ---- extended distance metrics: the re-rank of search_with_hnsw_and_metric ------------------------------------ */

/* `tensor_store::DistanceMetric` (tensor_store/src/distance.rs:13-52), the ExtendedDistanceMetric of vector_engine.  Both
 * vectors go through SparseVector::from_dense (a value is stored iff != 0.0); every sum is a sequential f64 sum over the
 * merged stored positions, rounded once to f32 (sparse_vector.rs:414-443, 548-599, 795-1059).  docs/hnsw.md §8. */
#define NMN_XMETRIC_COSINE 0            /* cosine_similarity, sparse_vector.rs:583-599 */
#define NMN_XMETRIC_ANGULAR 1           /* angular_distance, 795-798 */
#define NMN_XMETRIC_GEODESIC 2          /* geodesic_distance, 805-808 */
#define NMN_XMETRIC_JACCARD 3           /* jaccard_index, 816-845 */
#define NMN_XMETRIC_OVERLAP 4           /* overlap_coefficient, 852-878 */
#define NMN_XMETRIC_WEIGHTED_JACCARD 5  /* weighted_jaccard, 886-935 */
#define NMN_XMETRIC_EUCLIDEAN 6         /* euclidean_distance, 942-1006 */
#define NMN_XMETRIC_MANHATTAN 7         /* manhattan_distance, 1013-1059 */
#define NMN_XMETRIC_COMPOSITE 8         /* Composite(GeometricConfig), distance.rs:172-193 */
/* DistanceMetric; the three weights are GeometricConfig (distance.rs:115-125) and matter for NMN_XMETRIC_COMPOSITE only. */
typedef struct nmn_xmetric {
    int32_t kind; /* NMN_XMETRIC_* */
    float cosine_weight;
    float structural_weight;
    float magnitude_weight;
} nmn_xmetric;
/* Composite(GeometricConfig::default()) = (0.5, 0.3, 0.2), ::angular_heavy() = (0.8, 0.1, 0.1), ::structural_heavy() =
 * (0.2, 0.7, 0.1), ::conflict_detection() = (0.4, 0.5, 0.1) (distance.rs:127-166). */
void nmn_xmetric_geometric_default(nmn_xmetric* m);
void nmn_xmetric_geometric_angular_heavy(nmn_xmetric* m);
void nmn_xmetric_geometric_structural_heavy(nmn_xmetric* m);
void nmn_xmetric_geometric_conflict_detection(nmn_xmetric* m);
/* DistanceMetric::to_similarity (distance.rs:92-106): host arithmetic, no device needed.  NaN for an unknown kind. */
float nmn_xmetric_to_similarity(const nmn_xmetric* m, float raw);
/* DistanceMetric::higher_is_better (distance.rs:60-69): 1 / 0. */
int32_t nmn_xmetric_higher_is_better(const nmn_xmetric* m);
/* DistanceMetric::compute (distance.rs:76-88) and to_similarity(compute()) of every (query, row) pair, on the GPU:
 * out[q * n_rows + i] for local row local_rows[i].  HOST buffers; either output may be NULL.  The reference's bits, except
 * Angular / Geodesic: `acos` is the platform's libm there; here it is acos in f64 of the f32 cosine, rounded once.
 * Unknown kind: NMN_ERR_CONFIGURATION. */
nmn_status nmn_index_score_rows_xmetric(nmn_index* idx, const float* queries, uint32_t nq, const nmn_xmetric* metric,
                                        const uint64_t* local_rows, uint32_t n_rows, float* out_raw, float* out_similarity);
/* The same for ONE query against rows that live in HOST memory (n_rows x dim, tightly packed, any dim > 0): the re-rank of
 * search_with_hnsw_and_metric when the candidates' current vectors are not the rows of an index (lib.rs:2595-2598).  One device
 * block per call, the same kernel; out[i] for row i.  device -1: the current device. */
nmn_status nmn_xmetric_score_host_rows(int32_t device, const float* rows_host, uint32_t n_rows, uint32_t dim, const float* query,
                                       const nmn_xmetric* metric, float* out_raw, float* out_similarity);
/* VectorEngine::search_with_hnsw_and_metric (vector_engine/src/lib.rs:2560-2619) with node id == row of nmn_hnsw_vectors(h):
 * c = max(top_k.saturating_mul(2), 10) (2578), served as min(c, len); index.search(query, c) (2579; layer 0 runs with
 * max(ef_search, c), hnsw.rs:2055-2111), the walk's scores dropped; every candidate scored as
 * metric.to_similarity(metric.compute(query, row)) (2588-2601); stable sort by score descending, truncated to top_k
 * (2611-2617).  queries HOST nq x dim; out_ids nq x top_k (unused = UINT64_MAX), out_scores nq x top_k (unused = -inf),
 * out_counts nq.  Empty index: counts 0.  top_k == 0: NMN_ERR_INVALID_TOP_K; unknown kind: NMN_ERR_CONFIGURATION.  stats: sweep_kind NMN_SWEEP_GRAPH, rows_scanned = the walk's
 * distance evaluations, candidates_rescored = the most candidates re-ranked for one query.  NMN_HNSW_HOST_SEARCH=1 moves the
 * walk to the host as for nmn_hnsw_search; the re-rank still runs on the device. */
nmn_status nmn_hnsw_search_metric(nmn_hnsw* h, const float* queries, uint32_t nq, uint32_t top_k, const nmn_xmetric* metric,
                                  uint64_t* out_ids, float* out_scores, uint32_t* out_counts, nmn_search_stats* stats);
/* nmn_hnsw_search_metric for several queries in one call, each with its own top_k and its own metric (docs/hnsw.md §12).  HOST
 * buffers; top_k[i] in 1 .. kstride, metrics[i] one per query, out_ids / out_scores nq x kstride, out_counts nq.  Answer i is bit for
 * bit what nmn_hnsw_search_metric(h, q_i, 1, top_k[i], &metrics[i], ..) returns alone, padded to kstride with UINT64_MAX / -inf.
 * Refused before anything is enqueued or written: a quantized handle NMN_ERR_CONFIGURATION, top_k[i] == 0 NMN_ERR_INVALID_TOP_K,
 * top_k[i] > kstride NMN_ERR_INVALID_ARGUMENT, an unknown kind at any i NMN_ERR_CONFIGURATION.  stats: rows_scanned and
 * fallback_queries are the sums over the queries, candidates_rescored the maximum, sweep_kind / sweep_launches the lone call's.
 * Like nmn_hnsw_search_metric it joins the coalescer of nmn_hnsw_search: concurrent callers of any of the four leave as one walk,
 * the re-rank and the ordering behind it carry kind, weights and top_k per query.  A call that asks for more than 4 096 candidates
 * for a query (2 top_k, capped by the index's length) runs alone. */
nmn_status nmn_hnsw_search_metric_multi(nmn_hnsw* h, const float* queries, uint32_t nq, const uint32_t* top_k,
                                        const nmn_xmetric* metrics, uint32_t kstride, uint64_t* out_ids, float* out_scores,
                                        uint32_t* out_counts, nmn_search_stats* stats);
/* The same with every buffer in DEVICE memory, enqueued on `stream` behind the walk and not waited for: the walk's launches,
 * the re-rank and the ordering (one launch; above 16 384 candidates the large-k sort, query by query); nothing is read back.  The nq x c candidate block lives in the stream's scratch: a shape the
 * stream has served before allocates nothing. */
nmn_status nmn_hnsw_search_metric_device(nmn_hnsw* h, const float* queries_dev, uint32_t nq, uint32_t top_k,
                                         const nmn_xmetric* metric, uint64_t* out_ids_dev, float* out_scores_dev,
                                         uint32_t* out_counts_dev, void* stream);

/* ---- CacheIndex::search_with_metric behind the walk (tensor_cache/src/index.rs:186-375; docs/hnsw.md §16) ------ */

/* The live mask: one bit per node, on the host and in HBM beside the adjacency.  A new node is live.  Sets (live != 0) or clears
 * the bits of nodes[0 .. n) under the lock nmn_hnsw_insert takes, with the same wait for the device searches in flight, and
 * sends the touched words again.  A node at or past nmn_hnsw_len: NMN_ERR_NOT_FOUND, nothing flipped.  Only nmn_hnsw_cache_search*
 * read the mask: every other entry ignores it and launches exactly what it launches without.  nmn_hnsw_save does NOT store the
 * mask (a loaded handle has every node live); nmn_hnsw_hbm_bytes counts it. */
nmn_status nmn_hnsw_set_node_mask(nmn_hnsw* h, const uint64_t* nodes, uint64_t n, int32_t live);
/* 1: the node's bit is set, 0: cleared, -1: no such node. */
int32_t nmn_hnsw_node_live(nmn_hnsw* h, uint64_t node);
/* CacheIndex::search_with_metric (index.rs:186-272) with node ids in place of keys, on a dense-strategy handle:
 * c = max(3 k, 10) in 64 bits (204), served as min(c, len); index.search(query, c) under the handle's OWN HNSW metric (layer 0
 * runs with max(ef_search, c)), the walk's scores dropped; a candidate whose live bit is cleared is dropped (223-226); every other
 * is scored as metric.to_similarity(metric.compute(from_dense(query), stored)) where `stored` is from_dense(row) for a Dense node
 * and the stored entries AS THEY ARE for a Sparse node (229-246: a duplicated position pairs the i-th duplicate with the i-th,
 * which is not what its to_dense() row scores); kept iff similarity >= threshold in f32 (248: NaN on either side fails, equality
 * passes); stable sort by similarity descending, truncated to k (256-262).  queries HOST nq x dim; out_ids nq x k NODE ids
 * (unused = UINT64_MAX), out_scores nq x k similarities (unused = -inf), out_counts nq.  Empty index: counts 0.
 * Refused before anything is enqueued or written: a quantized handle NMN_ERR_CONFIGURATION (a CacheIndex never holds quantized
 * nodes), an unknown kind NMN_ERR_CONFIGURATION, k == 0 NMN_ERR_INVALID_TOP_K (the rule of nmn_hnsw_search_metric; the key
 * layer answers k == 0 itself).  Angular / Geodesic: the acos rule of nmn_index_score_rows_xmetric.
 * stats: rows_scanned and fallback_queries are the walk's, candidates_rescored = the most candidates of one query.
 * It joins the coalescer of nmn_hnsw_search: concurrent callers of any host-buffer search leave as one walk; the re-rank and the
 * ordering behind it carry kind, weights, top_k, threshold and the filter flag per query.  A call whose c is above 4 096 runs
 * alone.  NMN_HNSW_HOST_SEARCH=1 and NMN_HNSW_NO_COALESCE=1 act as for nmn_hnsw_search_metric. */
nmn_status nmn_hnsw_cache_search(nmn_hnsw* h, const float* queries, uint32_t nq, uint32_t k, float threshold,
                                 const nmn_xmetric* metric, uint64_t* out_ids, float* out_scores, uint32_t* out_counts,
                                 nmn_search_stats* stats);
/* CacheIndex::search_sparse_with_metric (index.rs:291-375): the same with index.search_sparse(query, c), and the query's own
 * entries go into compute().  The CSR, its canonicalisation, errors and texts are nmn_hnsw_search_sparse's.  The walk is that
 * entry's (on the host where docs/hnsw.md §15 routes it there); its candidate ids are then uploaded for the device re-rank and
 * ordering.  A query without a duplicated position is re-ranked as its to_dense() row (the same bits), one with a duplicate on
 * its entries.  Runs alone: it does not share a batch. */
nmn_status nmn_hnsw_cache_search_sparse(nmn_hnsw* h, const uint64_t* indptr, const uint32_t* positions, const float* values,
                                        uint32_t nq, uint32_t k, float threshold, const nmn_xmetric* metric, uint64_t* out_ids,
                                        float* out_scores, uint32_t* out_counts, nmn_search_stats* stats);
/* nmn_hnsw_cache_search with every buffer in DEVICE memory, enqueued on `stream` and not waited for, like
 * nmn_hnsw_search_metric_device: the walk's launches, the dense re-rank, on a handle with sparse nodes the merge re-rank, and the
 * filtered ordering (above min(NMN_XMETRIC_SORT_FROM, 16 384) candidates the large-k sort, query by query); nothing is read back. */
nmn_status nmn_hnsw_cache_search_device(nmn_hnsw* h, const float* queries_dev, uint32_t nq, uint32_t k, float threshold,
                                        const nmn_xmetric* metric, uint64_t* out_ids_dev, float* out_scores_dev,
                                        uint32_t* out_counts_dev, void* stream);
/* nmn_hnsw_cache_search_sparse as ONE stream-ordered chain, every buffer in DEVICE memory, no host round trip: the canonicaliser
 * (nmn_sparse_canonicalise_device), the sparse walk for c candidates, the re-rank on the to_dense() rows — a query with a
 * duplicated position on its own entries, by the merge kernel — the filtered ordering, and the launch that gives the queries with
 * a status their sentinel rows.  Answers are nmn_hnsw_cache_search_sparse's bit for bit.  The CSR arguments, the statuses and the
 * three refusals are nmn_hnsw_search_sparse_device's; the other refusals are nmn_hnsw_cache_search's. */
nmn_status nmn_hnsw_cache_search_sparse_device(nmn_hnsw* h, const uint64_t* indptr_dev, const uint32_t* positions_dev,
                                               const float* values_dev, uint32_t nq, uint64_t nnz_total, uint32_t max_nnz, uint32_t k,
                                               float threshold, const nmn_xmetric* metric, uint64_t* out_ids_dev,
                                               float* out_scores_dev, uint32_t* out_counts_dev, uint32_t* out_status_dev, void* stream);

/* ---- persistence of the device layout ----------------------------------- */

/* The reference persists a collection as PersistentVectorIndex — (key, vector, metadata) entries in JSON or bitcode —
 * and guards every load with VectorEngineConfig::max_index_file_bytes / max_index_entries (vector_engine/src/lib.rs:
 * 509-531, 644-646, 660-661, 3794-3899).  These entry points persist what the GPU path adds to that: the matrix of a
 * shard as it sits in HBM.  File: 64-byte header | rows x dim f32 (row stride removed) | rows f32 magnitudes.  A load
 * is sequential reads + bulk H2D copies; the magnitudes the upload recomputes on the GPU (reference order) must equal
 * the stored ones bit for bit, which is the file's integrity check.  The bf16 mirror is re-derived on first search.
 *   overrides   nullable: device, capacity_rows (>= the file's rows; spare room for appends), flags, cand_cap,
 *               row_base (0 = keep the file's); dim 0 or equal to the file's (else NMN_ERR_DIMENSION_MISMATCH)
 *   max_file_bytes / max_entries   0 = no limit; otherwise the reference's checks, in its order (file size before
 *               reading, entry count after the header) and with its texts: NMN_ERR_CONFIGURATION
 *               "index file size {} exceeds limit {}" / "index entry count {} exceeds limit {}". */
nmn_status nmn_index_save(nmn_index* idx, const char* path);
nmn_status nmn_index_load(const char* path, const nmn_index_desc* overrides, uint64_t max_file_bytes,
                          uint64_t max_entries, nmn_index** out);
/* The same for an IVF index: trained centroids, the list of every vector (`assign[]`) and the vectors in id order, so a
 * restart neither re-runs k-means (tensor_store/src/ivf.rs:222-233) nor re-assigns a single vector.  IVF-Flat only: a PQ or
 * Binary index returns NMN_ERR_CONFIGURATION (the reference's IVFIndexState drops the codebook too, ivf.rs:515-552). */
nmn_status nmn_ivf_save(nmn_ivf* ivf, const char* path);
nmn_status nmn_ivf_load(const char* path, const nmn_index_desc* overrides, uint64_t max_file_bytes, uint64_t max_entries,
                        nmn_ivf** out);
/* The same for an HNSW index, the most expensive one to build (nmn_hnsw_insert is one host thread by definition of its result).
 * The reference does not serialise HNSWIndex (tensor_store/src/hnsw.rs derives serde for the metric, ScalarQuantizedVector and
 * HNSWConfig only), so the format is this library's own; docs/hnsw.md §10 is its specification.  File: 64-byte header (kind 4,
 * flags bit 0 = quantized, rows = nodes, aux = bytes of the graph section, reserved = its FNV-1a 64) | graph section (the 48
 * bytes of nmn_hnsw_config, the level generator's state, entry point, max_layer, levels, every neighbour list) | rows (dense: a
 * flat section as nmn_index_save writes it; quantized: n x dim codes, n x {scale, min_val, magnitude, squared_magnitude}).
 * A loaded handle is indistinguishable from the one saved: same graph, same ids and score bits from every search entry, and
 * nmn_hnsw_insert continues exactly where the saved handle would have (levels, lists and generator state come back).  The heap
 * capacities of nmn_hnsw_set_heap_capacity are a run-time knob and are not stored.
 *   save   takes the handle's lock shared: searches may run, inserts wait.  Host state only, no device traffic, no kernel.
 *   load   no kernel of its own either: sequential reads, host checks, bulk copies.  EVERY check runs on the host before any
 *          allocation sized by an unchecked number and before anything reaches the search kernel: sizes against the bytes in the
 *          file, the checksum, the config, levels / entry point / max_layer, and of every list its count (<= m0 / m), ids (< n,
 *          strictly ascending) and that every id listed on layer L >= 1 has level >= L; the rows' magnitudes recomputed on the
 *          host (and, dense, on the device) must equal the stored bits.  A missing file is NMN_ERR_IO, the two limits are
 *          nmn_index_load's (NMN_ERR_CONFIGURATION, the same texts), anything else wrong with a file NMN_ERR_SERIALIZATION with
 *          a text that names the first failed check.  Files of the other kinds are refused, and nmn_index_load / nmn_ivf_load
 *          refuse an HNSW file.  capacity_hint sizes the row arrays as in nmn_hnsw_create (at least the file's nodes). */
nmn_status nmn_hnsw_save(nmn_hnsw* h, const char* path);
nmn_status nmn_hnsw_load(const char* path, int32_t device, uint64_t capacity_hint, uint64_t max_file_bytes, uint64_t max_entries,
                         nmn_hnsw** out);

/* ---- delta vectors (docs/delta.md) --------------------------------------------------------- */

/* DeltaVector and ArchetypeRegistry (tensor_store/src/delta_vector.rs:72-643), bit for bit: a row stored as its difference from an
 * archetype.  Every sum is the reference's strictly sequential f32 chain (an iterator's `.sum()` folds from -0.0, the explicit
 * accumulators from +0.0, products rounded before they are added, one correctly rounded square root and division per score); the
 * device kernels (nmn_delta.hip) and the host restatement in the same file run the same chains, so which of them answers a call
 * never shows in a bit.  A call of fewer than nmn_delta_options.min_device_rows rows (of a set: the set's rows; of pairs: the
 * pairs) is the host's. */
typedef struct nmn_archetypes nmn_archetypes;
typedef struct nmn_delta_set nmn_delta_set;
#define NMN_DELTA_MAX_DIMENSION 65535u /* MAX_DIMENSION: positions are u16 (delta_vector.rs:39) */
#define NMN_DELTA_VECTOR_BYTES 72u     /* size_of::<DeltaVector>() on a 64-bit target: 2 usize + 2 Vec headers + Option<f32> */
typedef struct nmn_delta_options {
    uint64_t min_device_rows; /* calls of fewer rows run on the host; 0: always the device, UINT64_MAX: never */
} nmn_delta_options;
/* the default: above the largest measured crossover of a device call against the host path (docs/delta.md, Measurements) */
#define NMN_DELTA_DEFAULT_MIN_DEVICE_ROWS 4096ull
void nmn_delta_options_default(nmn_delta_options* opt);
/* CoverageStats (delta_vector.rs:677-687) without archetype_usage, which is an output array of its own */
typedef struct nmn_coverage_stats {
    float avg_similarity;
    float avg_compression_ratio;
    float avg_delta_nnz;
    uint32_t reserved;
} nmn_coverage_stats;
/* What the device path serves, each output nullable: the largest dimension a delta row can have; the largest dimension whose query
 * nmn_delta_set_dot_dense keeps in LDS (above it the gather reads the query from global memory, same bits); the archetypes of one
 * register tile of find_best; the rows of one block of the offset scan of encode_batch. */
nmn_status nmn_delta_limits(uint32_t* max_dimension, uint32_t* lds_query_dim, uint32_t* archetype_tile, uint32_t* scan_block);

/* ArchetypeRegistry::new(max_archetypes) for rows of `dim` floats (dim >= 1).  device: HIP ordinal, -1 = the current one; nothing
 * is allocated on it before the first call that takes the device path. */
nmn_status nmn_archetypes_create(uint32_t dim, uint64_t max_archetypes, int32_t device, nmn_archetypes** out);
nmn_status nmn_archetypes_destroy(nmn_archetypes* a);
nmn_status nmn_archetypes_set_options(nmn_archetypes* a, const nmn_delta_options* opt);
/* register (442-452) for n rows (HOST, n x dim) in order: ids_out[i] is the new id, -1 where the reference returns None. */
nmn_status nmn_archetypes_register(nmn_archetypes* a, const float* rows, uint64_t n, int64_t* ids_out);
/* discover_archetypes (566-592): k.min(n).min(max - len) centroids of KMeans::fit (the GPU k-means of nmn_ivf_build, which sets
 * the shapes this call takes: anything it refuses is refused here with its text) appended in order.  *added_out is the return.
 * The k-means has no host restatement: this call always needs the device, whatever min_device_rows says (a call that returns 0
 * before the fit — no vectors, k == 0, a full registry — touches none). */
nmn_status nmn_archetypes_discover(nmn_archetypes* a, const float* rows, uint64_t n, uint64_t k, const nmn_kmeans_options* opt,
                                   uint64_t* added_out);
uint64_t nmn_archetypes_len(nmn_archetypes* a);
uint32_t nmn_archetypes_dim(nmn_archetypes* a);
uint64_t nmn_archetypes_max(nmn_archetypes* a);
nmn_status nmn_archetypes_get(nmn_archetypes* a, uint64_t id, float* out);          /* NMN_ERR_NOT_FOUND: None */
nmn_status nmn_archetypes_magnitude_sq(nmn_archetypes* a, uint64_t id, float* out); /* NMN_ERR_NOT_FOUND: None */
/* find_best_archetype (480-513) of n rows (HOST): ids_out[i] = -1 and sims_out[i] untouched on an empty registry (None). */
nmn_status nmn_archetypes_find_best(nmn_archetypes* a, const float* rows, uint64_t n, int64_t* ids_out, float* sims_out);
/* analyze_coverage (614-643): usage_out holds nmn_archetypes_len counters.  An empty registry or n == 0 is CoverageStats::default. */
nmn_status nmn_archetypes_analyze_coverage(nmn_archetypes* a, const float* rows, uint64_t n, float threshold,
                                           nmn_coverage_stats* stats_out, uint64_t* usage_out);
/* encode_batch (598-607): every row against its best archetype (try_from_dense_with_reference, 113-147); with_magnitude != 0 caches
 * sqrt(sum x * x) of the dense row as from_dense_with_reference_and_magnitude (151-161) does.  An empty registry gives an empty set.
 * A dimension above 65535 is NMN_ERR_INVALID_ARGUMENT with DeltaVectorError's Display — unless the registry is empty or n == 0: the
 * reference's `encode` is None before any DeltaVector is built, so the set is empty at any dimension. */
nmn_status nmn_archetypes_encode_batch(nmn_archetypes* a, const float* rows, uint64_t n, float threshold, int32_t with_magnitude,
                                       nmn_delta_set** out);
/* from_parts (170-205) for n rows: row i holds positions / deltas [indptr[i], indptr[i + 1]) against archetype_ids[i].  cached is
 * nullable; has_cached (nullable: every row of `cached` counts) marks the rows whose cached_magnitude is Some.  Refused with texts
 * of their own: an archetype id that is not registered, an indptr that does not start at 0 or does not ascend, a position that is
 * not below the dimension.  Unsorted and repeated positions are kept as they are. */
nmn_status nmn_delta_set_from_parts(nmn_archetypes* a, uint64_t n, const uint64_t* archetype_ids, const uint64_t* indptr,
                                    const uint16_t* positions, const float* deltas, const float* cached, const uint8_t* has_cached,
                                    nmn_delta_set** out);
/* A set is immutable and tied to the registry it was made against, which must outlive it. */
nmn_status nmn_delta_set_destroy(nmn_delta_set* s);
uint64_t nmn_delta_set_len(nmn_delta_set* s);
uint64_t nmn_delta_set_nnz(nmn_delta_set* s);
/* copies out, each output nullable: [n], [n + 1], [nnz], [nnz], [n], [n]; sorted_out[i] = 1 where row i's positions strictly ascend */
nmn_status nmn_delta_set_arrays(nmn_delta_set* s, uint64_t* archetype_ids, uint64_t* indptr, uint16_t* positions, float* deltas,
                                float* cached, uint8_t* has_cached, uint8_t* sorted_out);
/* compression_ratio (410-416) and memory_bytes (276-280) per row */
nmn_status nmn_delta_set_compression_ratio(nmn_delta_set* s, float* out);
nmn_status nmn_delta_set_memory_bytes(nmn_delta_set* s, uint64_t* out);
/* to_dense (209-217) per row: out [n][dim].  magnitude (260-267) per row: out [n]. */
nmn_status nmn_delta_set_decode(nmn_delta_set* s, float* out);
nmn_status nmn_delta_set_magnitudes(nmn_delta_set* s, float* out);
/* dot_dense (309-312) and cosine_similarity_dense (374-388) of every row with every query (HOST, nq x dim): out [nq][n];
 * query_magnitude is sqrt(sum q * q), the sequential chain. */
nmn_status nmn_delta_set_dot_dense(nmn_delta_set* s, const float* queries, uint32_t nq, float* out);
nmn_status nmn_delta_set_cosine_dense(nmn_delta_set* s, const float* queries, uint32_t nq, float* out);
/* dot_deltas_same_archetype (544-552; dot_same_archetype, 321-349): pairs [n_pairs][2] = (row of a, row of b); ok_out[i] = 0 and
 * out[i] untouched where the archetype ids differ (None).  Both sets belong to one registry. */
nmn_status nmn_delta_set_dot_same_archetype(nmn_delta_set* a, nmn_delta_set* b, const uint64_t* pairs, uint64_t n_pairs, float* out,
                                            uint8_t* ok_out);
/* Stream-ordered forms: DEVICE pointers on the handle's device, enqueued on `stream`, not waited for, nothing read back, nothing
 * allocated.  The handle must be resident: nmn_archetypes_to_device / nmn_delta_set_to_device (which do block) after the last
 * register; a handle that is not is NMN_ERR_INVALID_ARGUMENT with a text that says so, as is an empty registry (its answer is no
 * array).  ids_dev [n] int64, sims_dev [n]; scratch_dev: nq x (nmn_archetypes_len + 1) floats the call may overwrite.  The
 * residency flags are atomic, the mirrors behind them are not: nmn_archetypes_register, nmn_archetypes_to_device and
 * nmn_delta_set_to_device (and any host-buffer call that takes the device path after a register, which uploads the registry again)
 * must not run concurrently with a stream-ordered call on the same handles, nor while one is still in flight. */
nmn_status nmn_archetypes_to_device(nmn_archetypes* a);
nmn_status nmn_delta_set_to_device(nmn_delta_set* s);
nmn_status nmn_archetypes_find_best_device(nmn_archetypes* a, const float* rows_dev, uint64_t n, int64_t* ids_dev, float* sims_dev,
                                           void* stream);
nmn_status nmn_delta_set_dot_dense_device(nmn_delta_set* s, const float* queries_dev, uint32_t nq, float* scratch_dev, float* out_dev,
                                          void* stream);
nmn_status nmn_delta_set_cosine_dense_device(nmn_delta_set* s, const float* queries_dev, uint32_t nq, float* scratch_dev,
                                             float* out_dev, void* stream);

/* Top-k over a delta set (docs/delta.md, section 8).  The answer of query q is the first min(k, n) rows of all n rows sorted by the
 * project's order (docs/exactness.md): score descending, row ascending, -0.0 and +0.0 equal, every NaN equal to every other NaN and
 * below -inf.  The score is what nmn_delta_set_dot_dense (cosine = 0) or nmn_delta_set_cosine_dense (cosine != 0) returns for that
 * row, and the score returned is the row's own bits: a -0.0 stays -0.0, a NaN keeps its payload.  rows_out / scores_out are [nq][k],
 * counts_out[q] = min(k, n); the unused slots hold row UINT64_MAX and score -inf.  k == 0 and a set of 4294967295 rows or more are
 * NMN_ERR_INVALID_ARGUMENT.  Below min_device_rows the host scores and sorts: same bits.  On the device a k up to select_max_k is
 * served by one select workgroup per query, a larger k by the sort of the large-k path, one query at a time; so is a call of ONE
 * query over sort_single_query_rows rows or more, which one workgroup would serve more slowly.  The host-buffer form
 * takes its queries in blocks whose score words [queries][n] stay within block_budget_bytes. */
nmn_status nmn_deltaset_limits(uint32_t* select_chunk_rows, uint32_t* select_max_k, uint64_t* block_budget_bytes,
                               uint64_t* sort_single_query_rows);
nmn_status nmn_deltaset_search(nmn_delta_set* s, const float* queries, uint32_t nq, uint32_t k, int32_t cosine, uint64_t* rows_out,
                               float* scores_out, uint32_t* counts_out);
/* The stream-ordered form: DEVICE pointers, enqueued on `stream`, not waited for, nothing allocated, no mutex taken; the handles must
 * be resident as for the stream-ordered scores above.  scratch_dev: nmn_deltaset_search_scratch_bytes bytes (for the same nq and k,
 * asked after the last register), aligned to 16 bytes, which the call may overwrite. */
uint64_t nmn_deltaset_search_scratch_bytes(nmn_delta_set* s, uint32_t nq, uint32_t k);
nmn_status nmn_deltaset_search_device(nmn_delta_set* s, const float* queries_dev, uint32_t nq, uint32_t k, int32_t cosine,
                                      void* scratch_dev, uint64_t scratch_bytes, uint64_t* rows_dev, float* scores_dev,
                                      uint32_t* counts_dev, void* stream);

/* A delta set made where the rows are (docs/delta.md, section 9): encode_batch of n rows that are already on the device (rows_dev,
 * n x dim, DEVICE), into a resident set that holds NO host copy of its arrays.  Enqueues on `stream`: find_best, count and scan,
 * the slice lengths and their scan; then WAITS once on that stream for two u64 (the entry total and the slice total), allocates, and
 * enqueues the entry write, the 64-row entry-major slices and the magnitudes.  It returns with those enqueued and not waited for; the
 * set records an event at their end, and the library's own host-buffer calls on the set wait for it.  Stream-ordered callers order
 * themselves (same stream, or their own event).  ids_dev [n] int64 / sims_dev [n] (nullable, DEVICE) receive find_best's answers.
 * Refused with NMN_ERR_INVALID_ARGUMENT and a text of its own: an empty registry; a registry that is not resident or not current;
 * a dimension above 65535 (DeltaVectorError's Display).  n == 0 gives an empty set.  The host arrays (nmn_delta_set_arrays,
 * the compression ratios and memory bytes, any host-path call) are downloaded on first need, each once, under a lock of the set's;
 * nmn_deltaset_host_arrays_present says whether that has happened (1) or not (0).  The host-buffer encode_batch on its device path
 * returns such a set too. */
nmn_status nmn_deltaset_encode_device(nmn_archetypes* a, const float* rows_dev, uint64_t n, float threshold, int32_t with_magnitude,
                                      int64_t* ids_dev, float* sims_dev, void* stream, nmn_delta_set** out);
int32_t nmn_deltaset_host_arrays_present(nmn_delta_set* s);

/* ---- synthetic data (bench / tests) ------------------------------------------------------- */

/* value(seed,row,col): a counter-based generator that is bit-identical on host and device
 * (integer hash -> sum of four 16-bit uniforms -> one exact f32 scale; approx. N(0,1)).
 * `row` is the GLOBAL row id, so shards of one corpus agree with the unsharded corpus. */
float nmn_synth_value(uint64_t seed, uint64_t row, uint32_t col);
/* Fill host memory: out[i*dim + c] = value(seed, row0+i, c). */
nmn_status nmn_synth_fill_host(float* out, uint64_t seed, uint64_t row0, uint64_t n, uint32_t dim);
/* Fill local rows [row0,row0+n) of the shard on the GPU with value(seed, row_base+row, col) and
 * compute their norms; no host traffic (the 10M x 768 corpus is 30.7 GB). */
nmn_status nmn_index_fill_synthetic(nmn_index* idx, uint64_t seed, uint64_t row0, uint64_t n);
/* Overwrite one local row from host memory (used to plant near-duplicates); recomputes its norm. */
nmn_status nmn_index_set_row(nmn_index* idx, uint64_t row, const float* vec_host);

#ifdef __cplusplus
}
#endif
#endif /* NEUMANN_GPU_H */
