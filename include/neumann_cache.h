/* neumann_cache.h — tensor_cache::CacheIndex (tensor_cache/src/index.rs:30-451) on top of the GPU HNSW index: the key maps of the
 * semantic cache on the host, every lookup one nmn_hnsw_cache_search (docs/hnsw.md §16).
 *
 * Status codes are the nmn_status values of neumann_gpu.h; nmn_cache_index_last_error() returns the text of the calling thread's
 * last failure.  Every function may be called from many threads at once.
 *
 * The maps and their surprises are the reference's:
 *   insert on an existing key (91-118) forgets key -> node but NOT node -> key of the old node: the old node keeps answering under
 *     that key (a result list may hold the key twice) and len() does not grow;
 *   remove (383-391) deletes only the CURRENT node's node -> key entry: a node orphaned by an earlier re-insert still answers with
 *     the key although contains(key) is false;
 *   clear (420-428) replaces the index: node ids restart at 0 and the level generator at its seed.  Searches in flight finish on
 *     the index they started on and answer empty.
 * The live mask of the HNSW handle (nmn_hnsw_set_node_mask) always equals "node -> key has the node".
 * A CacheIndex never holds quantized nodes: the handle is a dense-strategy one. */
#ifndef NEUMANN_CACHE_H
#define NEUMANN_CACHE_H

#include <stddef.h>
#include <stdint.h>

#include "neumann_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nmn_cache_index nmn_cache_index;

/* CacheIndex::with_metric (73-83).  hnsw_config NULL: HNSWConfig::default(); xmetric NULL: DistanceMetric::Cosine (67-69).
 * device -1: the current device. */
nmn_status nmn_cache_index_create(uint32_t dim, const nmn_hnsw_config* hnsw_config, const nmn_xmetric* xmetric, int32_t device,
                                  nmn_cache_index** out);
nmn_status nmn_cache_index_destroy(nmn_cache_index* c);
const char* nmn_cache_index_last_error(void);

/* insert (91-118), insert_sparse (123-148), insert_auto (153-166): *node_out (nullable) = the node id.  len != dimension:
 * NMN_ERR_DIMENSION_MISMATCH.  insert_sparse: the (position, value) pairs are made a SparseVector as try_from_parts does (the
 * rules and errors of nmn_hnsw_insert_sparse).  insert_auto stores Sparse(from_dense(v)) iff from_dense(v).sparsity() =
 * 1.0 - nnz as f32 / dim as f32 (sparse_vector.rs:302-308) >= sparsity_threshold, the CALLER's threshold, in f32. */
nmn_status nmn_cache_index_insert(nmn_cache_index* c, const char* key, const float* v, uint32_t len, uint64_t* node_out);
nmn_status nmn_cache_index_insert_sparse(nmn_cache_index* c, const char* key, const uint32_t* positions, const float* values,
                                         uint64_t nnz, uint64_t* node_out);
nmn_status nmn_cache_index_insert_auto(nmn_cache_index* c, const char* key, const float* v, uint32_t len, float sparsity_threshold,
                                       uint64_t* node_out);

/* search (172-179), search_with_metric (186-272), search_sparse (278-285), search_sparse_with_metric (291-375): the steps of
 * nmn_hnsw_cache_search / nmn_hnsw_cache_search_sparse, nodes mapped to keys.  Results in order: keys_out receives the keys one
 * after the other, each ended by a NUL byte, *keys_len their total length; sims_out[k] the similarities; *count how many.
 * keys_cap too small: NMN_ERR_BUFFER_TOO_SMALL with *keys_len = the bytes needed and *count set, nothing else written.
 * k == 0 answers empty without touching the device; a k beyond the index's length is served as that length (no answer is longer),
 * so sims_out needs min(k, max(len, 1)) floats.  A query of another length: NMN_ERR_DIMENSION_MISMATCH.  `search` and
 * `search_sparse` use the metric given at create. */
nmn_status nmn_cache_index_search(nmn_cache_index* c, const float* query, uint32_t len, uint32_t k, float threshold, char* keys_out,
                                  uint64_t keys_cap, uint64_t* keys_len, float* sims_out, uint32_t* count);
nmn_status nmn_cache_index_search_with_metric(nmn_cache_index* c, const float* query, uint32_t len, uint32_t k, float threshold,
                                              const nmn_xmetric* metric, char* keys_out, uint64_t keys_cap, uint64_t* keys_len,
                                              float* sims_out, uint32_t* count);
nmn_status nmn_cache_index_search_sparse(nmn_cache_index* c, const uint32_t* positions, const float* values, uint64_t nnz, uint32_t k,
                                         float threshold, char* keys_out, uint64_t keys_cap, uint64_t* keys_len, float* sims_out,
                                         uint32_t* count);
nmn_status nmn_cache_index_search_sparse_with_metric(nmn_cache_index* c, const uint32_t* positions, const float* values, uint64_t nnz,
                                                     uint32_t k, float threshold, const nmn_xmetric* metric, char* keys_out,
                                                     uint64_t keys_cap, uint64_t* keys_len, float* sims_out, uint32_t* count);

/* remove (383-391): 1 if the key was there, 0 otherwise; a NEGATIVE nmn_status if the node's bit of the live mask could not be
 * cleared (a device error): nothing was removed then, the text is nmn_cache_index_last_error().  contains (395-397), len (401-403: the counter), dimension (412-414). */
int32_t nmn_cache_index_remove(nmn_cache_index* c, const char* key);
int32_t nmn_cache_index_contains(nmn_cache_index* c, const char* key);
uint64_t nmn_cache_index_len(nmn_cache_index* c);
uint32_t nmn_cache_index_dimension(const nmn_cache_index* c);
/* the metric given at create (86-88) */
nmn_status nmn_cache_index_metric(const nmn_cache_index* c, nmn_xmetric* out);
/* keys (432-434), in no particular order: the layout of the searches' keys_out; *n_keys how many */
nmn_status nmn_cache_index_keys(nmn_cache_index* c, char* keys_out, uint64_t keys_cap, uint64_t* keys_len, uint64_t* n_keys);
nmn_status nmn_cache_index_clear(nmn_cache_index* c);
nmn_status nmn_cache_index_memory_stats(nmn_cache_index* c, nmn_hnsw_memstats* out);
/* get_embedding (446-450) of the key's CURRENT node: *kind = 0 Dense (dense_out[dim] filled), 1 Sparse (*nnz entries; positions_out /
 * values_out filled if cap holds them, dense_out = to_dense()).  An unknown key: NMN_ERR_NOT_FOUND.  Every output is nullable. */
nmn_status nmn_cache_index_get_embedding(nmn_cache_index* c, const char* key, int32_t* kind, float* dense_out, uint32_t* positions_out,
                                         float* values_out, uint32_t cap, uint32_t* nnz);
/* The HNSW handle in use now (replaced by clear): for statistics such as nmn_hnsw_coalesce_stats.  Do not destroy it. */
nmn_hnsw* nmn_cache_index_hnsw(nmn_cache_index* c);

#ifdef __cplusplus
}
#endif

#endif /* NEUMANN_CACHE_H */
