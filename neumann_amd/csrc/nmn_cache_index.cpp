// nmn_cache_index.cpp — tensor_cache::CacheIndex (tensor_cache/src/index.rs:30-451) over nmn_hnsw: the key maps on the host, the
// lookup nmn_hnsw_cache_search[_sparse] (docs/hnsw.md §16).  No kernels in this file.
//
// One mutex guards the maps, the counter and the handle pointer.  An insert holds it across the HNSW insert and the map update, so a
// search never meets a live node without a key; remove clears the node's bit of the live mask under it, so the device mask always
// equals "node_to_key has the node".  A search takes a reference to the handle under the mutex, walks WITHOUT it, and maps nodes to
// keys under it again: a node removed meanwhile is dropped (the reference's filter_map does the same, index.rs:215), and if clear
// swapped the handle meanwhile the answer is empty — the old node ids mean nothing to the new maps.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/neumann_cache.h"

namespace {

thread_local std::string g_err;

nmn_status fail(nmn_status st, const std::string& what) {
    g_err = what;
    return st;
}
nmn_status pass(nmn_status st) {  // a failure of the layer below, with its text
    if (st != NMN_OK) g_err = nmn_last_error();
    return st;
}

struct Handle {
    nmn_hnsw* h = nullptr;
    ~Handle() {
        if (h) nmn_hnsw_destroy(h);
    }
};

}  // namespace

struct nmn_cache_index {
    uint32_t dim = 0;
    int32_t device = -1;
    nmn_hnsw_config cfg{};
    nmn_xmetric metric{};
    std::mutex mu;
    std::shared_ptr<Handle> index;
    std::unordered_map<std::string, uint64_t> key_to_node;
    std::unordered_map<uint64_t, std::string> node_to_key;
    uint64_t entry_count = 0;
};

namespace {

nmn_status fresh_handle(const nmn_cache_index* c, std::shared_ptr<Handle>* out) {
    auto h = std::make_shared<Handle>();
    const nmn_status st = nmn_hnsw_create(&c->cfg, c->dim, 0, c->device, &h->h);
    if (st != NMN_OK) return pass(st);
    *out = std::move(h);
    return NMN_OK;
}

nmn_status dimension_mismatch(uint32_t expected, uint64_t got) {
    return fail(NMN_ERR_DIMENSION_MISMATCH,
                "dimension mismatch: expected " + std::to_string(expected) + ", got " + std::to_string(got));
}

// 99-117: the maps around an HNSW insert, all under c->mu
template <class Insert>
nmn_status bind(nmn_cache_index* c, const char* key, Insert&& insert, uint64_t* node_out) {
    std::lock_guard<std::mutex> lk(c->mu);
    uint64_t node = 0;
    const nmn_status st = insert(c->index->h, &node);
    if (st != NMN_OK) return pass(st);
    const bool is_new = c->key_to_node.find(key) == c->key_to_node.end();  // (104: node_to_key keeps the old node of a known key)
    c->key_to_node[key] = node;
    c->node_to_key[node] = key;
    if (is_new) c->entry_count++;
    if (node_out) *node_out = node;
    return NMN_OK;
}

// keys one after the other, each ended by a NUL byte
nmn_status write_keys(const std::vector<const std::string*>& keys, char* out, uint64_t cap, uint64_t* len_out) {
    uint64_t need = 0;
    for (const std::string* k : keys) need += k->size() + 1;
    if (len_out) *len_out = need;
    if (need > cap || (need && !out)) return fail(NMN_ERR_BUFFER_TOO_SMALL, "keys_out holds fewer bytes than *keys_len");
    for (const std::string* k : keys) {
        memcpy(out, k->c_str(), k->size() + 1);
        out += k->size() + 1;
    }
    return NMN_OK;
}

// 212-271 behind the walk: nodes to keys, in result order
template <class Walk>
nmn_status lookup(nmn_cache_index* c, uint32_t k, Walk&& walk, char* keys_out, uint64_t keys_cap, uint64_t* keys_len, float* sims_out,
                  uint32_t* count) {
    if (count) *count = 0;
    if (keys_len) *keys_len = 0;
    if (k == 0) return NMN_OK;  // truncate(0): empty, and no need to walk for it
    if (!sims_out || !count) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_ptr<Handle> idx;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        idx = c->index;
    }
    // No answer is longer than the index: a k beyond its length asks for every node (c = min(max(3k, 10), len) is len either way),
    // so the rows the walk answers into are sized by the length, not by whatever the caller passed.
    const uint32_t kk = (uint32_t)std::min<uint64_t>(k, std::max<uint64_t>(nmn_hnsw_len(idx->h), 1));
    std::vector<uint64_t> ids;
    std::vector<float> sims, kept;
    std::vector<const std::string*> keys;
    try {
        ids.resize(kk);
        sims.resize(kk);
        kept.reserve(kk);
        keys.reserve(kk);
    } catch (const std::bad_alloc&) {
        return fail(NMN_ERR_OUT_OF_MEMORY, "nmn_cache_index: no host memory for the result rows");
    }
    uint32_t n = 0;
    const nmn_status st = walk(idx->h, kk, ids.data(), sims.data(), &n);
    if (st != NMN_OK) return pass(st);
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->index == idx) {
        for (uint32_t i = 0; i < n; i++) {
            const auto it = c->node_to_key.find(ids[i]);
            if (it == c->node_to_key.end()) continue;  // removed since the walk
            keys.push_back(&it->second);
            kept.push_back(sims[i]);
        }
    }
    *count = (uint32_t)keys.size();
    const nmn_status ws = write_keys(keys, keys_out, keys_cap, keys_len);
    if (ws != NMN_OK) return ws;
    if (!kept.empty()) memcpy(sims_out, kept.data(), kept.size() * 4);
    return NMN_OK;
}

}  // namespace

extern "C" const char* nmn_cache_index_last_error(void) { return g_err.c_str(); }

extern "C" nmn_status nmn_cache_index_create(uint32_t dim, const nmn_hnsw_config* hnsw_config, const nmn_xmetric* xmetric, int32_t device,
                                             nmn_cache_index** out) {
    if (!out) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    auto c = std::make_unique<nmn_cache_index>();
    c->dim = dim;
    c->device = device;
    if (hnsw_config)
        c->cfg = *hnsw_config;
    else
        nmn_hnsw_config_default(&c->cfg);
    c->metric = xmetric ? *xmetric : nmn_xmetric{NMN_XMETRIC_COSINE, 0.0f, 0.0f, 0.0f};
    if (c->metric.kind < NMN_XMETRIC_COSINE || c->metric.kind > NMN_XMETRIC_COMPOSITE)
        return fail(NMN_ERR_CONFIGURATION, "unknown extended distance metric");
    const nmn_status st = fresh_handle(c.get(), &c->index);
    if (st != NMN_OK) return st;
    *out = c.release();
    return NMN_OK;
}

extern "C" nmn_status nmn_cache_index_destroy(nmn_cache_index* c) {
    delete c;  // (the handle goes with its last reference: no search may be running on a destroyed index)
    return NMN_OK;
}

extern "C" nmn_status nmn_cache_index_insert(nmn_cache_index* c, const char* key, const float* v, uint32_t len, uint64_t* node_out) {
    if (!c || !key || (!v && len)) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (len != c->dim) return dimension_mismatch(c->dim, len);
    return bind(c, key, [&](nmn_hnsw* h, uint64_t* node) { return nmn_hnsw_insert(h, v, 1, node); }, node_out);
}

extern "C" nmn_status nmn_cache_index_insert_sparse(nmn_cache_index* c, const char* key, const uint32_t* positions, const float* values,
                                                    uint64_t nnz, uint64_t* node_out) {
    if (!c || !key || (nnz && (!positions || !values))) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    const uint64_t indptr[2] = {0, nnz};
    return bind(c, key, [&](nmn_hnsw* h, uint64_t* node) { return nmn_hnsw_insert_sparse(h, indptr, positions, values, 1, node); }, node_out);
}

extern "C" nmn_status nmn_cache_index_insert_auto(nmn_cache_index* c, const char* key, const float* v, uint32_t len,
                                                  float sparsity_threshold, uint64_t* node_out) {
    if (!c || !key || (!v && len)) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    // from_dense first (159), whatever the length: the dimension is checked by the insert the decision leads to
    std::vector<uint32_t> pos;
    std::vector<float> val;
    for (uint32_t i = 0; i < len; i++)
        if (v[i] != 0.0f) {
            pos.push_back(i);
            val.push_back(v[i]);
        }
    const float ratio = (float)pos.size() / (float)len;
    const float sparsity = len == 0 ? 0.0f : 1.0f - ratio;  // sparse_vector.rs:302-308
    if (sparsity >= sparsity_threshold) {
        if (len != c->dim) return dimension_mismatch(c->dim, len);
        return nmn_cache_index_insert_sparse(c, key, pos.data(), val.data(), pos.size(), node_out);
    }
    return nmn_cache_index_insert(c, key, v, len, node_out);
}

extern "C" nmn_status nmn_cache_index_search_with_metric(nmn_cache_index* c, const float* query, uint32_t len, uint32_t k, float threshold,
                                                         const nmn_xmetric* metric, char* keys_out, uint64_t keys_cap,
                                                         uint64_t* keys_len, float* sims_out, uint32_t* count) {
    if (!c || !metric || (!query && len)) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (len != c->dim) return dimension_mismatch(c->dim, len);
    return lookup(
        c, k,
        [&](nmn_hnsw* h, uint32_t kk, uint64_t* ids, float* sims, uint32_t* n) {
            return nmn_hnsw_cache_search(h, query, 1, kk, threshold, metric, ids, sims, n, nullptr);
        },
        keys_out, keys_cap, keys_len, sims_out, count);
}

extern "C" nmn_status nmn_cache_index_search(nmn_cache_index* c, const float* query, uint32_t len, uint32_t k, float threshold,
                                             char* keys_out, uint64_t keys_cap, uint64_t* keys_len, float* sims_out, uint32_t* count) {
    if (!c) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    return nmn_cache_index_search_with_metric(c, query, len, k, threshold, &c->metric, keys_out, keys_cap, keys_len, sims_out, count);
}

extern "C" nmn_status nmn_cache_index_search_sparse_with_metric(nmn_cache_index* c, const uint32_t* positions, const float* values,
                                                                uint64_t nnz, uint32_t k, float threshold, const nmn_xmetric* metric,
                                                                char* keys_out, uint64_t keys_cap, uint64_t* keys_len, float* sims_out,
                                                                uint32_t* count) {
    if (!c || !metric || (nnz && (!positions || !values))) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    const uint64_t indptr[2] = {0, nnz};
    return lookup(
        c, k,
        [&](nmn_hnsw* h, uint32_t kk, uint64_t* ids, float* sims, uint32_t* n) {
            return nmn_hnsw_cache_search_sparse(h, indptr, positions, values, 1, kk, threshold, metric, ids, sims, n, nullptr);
        },
        keys_out, keys_cap, keys_len, sims_out, count);
}

extern "C" nmn_status nmn_cache_index_search_sparse(nmn_cache_index* c, const uint32_t* positions, const float* values, uint64_t nnz,
                                                    uint32_t k, float threshold, char* keys_out, uint64_t keys_cap, uint64_t* keys_len,
                                                    float* sims_out, uint32_t* count) {
    if (!c) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    return nmn_cache_index_search_sparse_with_metric(c, positions, values, nnz, k, threshold, &c->metric, keys_out, keys_cap, keys_len,
                                                     sims_out, count);
}

extern "C" int32_t nmn_cache_index_remove(nmn_cache_index* c, const char* key) {
    if (!c || !key) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    const auto it = c->key_to_node.find(key);
    if (it == c->key_to_node.end()) return 0;
    const uint64_t node = it->second;
    // the mask follows node_to_key, and first: if the bit cannot be cleared the maps stay as they are and the caller hears of it
    if (c->node_to_key.count(node)) {
        const nmn_status st = nmn_hnsw_set_node_mask(c->index->h, &node, 1, 0);
        if (st != NMN_OK) return (int32_t)pass(st);
    }
    c->key_to_node.erase(it);
    c->node_to_key.erase(node);
    c->entry_count--;
    return 1;
}

extern "C" int32_t nmn_cache_index_contains(nmn_cache_index* c, const char* key) {
    if (!c || !key) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    return c->key_to_node.count(key) ? 1 : 0;
}

extern "C" uint64_t nmn_cache_index_len(nmn_cache_index* c) {
    if (!c) return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    return c->entry_count;
}

extern "C" uint32_t nmn_cache_index_dimension(const nmn_cache_index* c) { return c ? c->dim : 0; }

extern "C" nmn_status nmn_cache_index_metric(const nmn_cache_index* c, nmn_xmetric* out) {
    if (!c || !out) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = c->metric;
    return NMN_OK;
}

extern "C" nmn_status nmn_cache_index_keys(nmn_cache_index* c, char* keys_out, uint64_t keys_cap, uint64_t* keys_len, uint64_t* n_keys) {
    if (!c) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    std::vector<const std::string*> keys;
    keys.reserve(c->key_to_node.size());
    for (const auto& kv : c->key_to_node) keys.push_back(&kv.first);
    if (n_keys) *n_keys = keys.size();
    return write_keys(keys, keys_out, keys_cap, keys_len);
}

extern "C" nmn_status nmn_cache_index_clear(nmn_cache_index* c) {
    if (!c) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_ptr<Handle> fresh, old;
    const nmn_status st = fresh_handle(c, &fresh);  // ids from 0, the level generator at its seed (422)
    if (st != NMN_OK) return st;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        old = std::move(c->index);
        c->index = std::move(fresh);
        c->key_to_node.clear();
        c->node_to_key.clear();
        c->entry_count = 0;
    }
    return NMN_OK;  // `old` is destroyed here, or by the last search still running on it
}

extern "C" nmn_status nmn_cache_index_memory_stats(nmn_cache_index* c, nmn_hnsw_memstats* out) {
    if (!c || !out) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_ptr<Handle> idx;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        idx = c->index;
    }
    return pass(nmn_hnsw_memory_stats(idx->h, out));
}

extern "C" nmn_status nmn_cache_index_get_embedding(nmn_cache_index* c, const char* key, int32_t* kind, float* dense_out,
                                                    uint32_t* positions_out, float* values_out, uint32_t cap, uint32_t* nnz) {
    if (!c || !key) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(c->mu);  // (held across the reads: clear must not take the handle away under them)
    const auto it = c->key_to_node.find(key);
    if (it == c->key_to_node.end()) return fail(NMN_ERR_NOT_FOUND, "no such key");
    nmn_hnsw* h = c->index->h;
    uint32_t n = 0;
    nmn_status st = nmn_hnsw_sparse_row(h, it->second, nullptr, nullptr, 0, &n);
    if (st != NMN_OK) return pass(st);
    const bool sparse = n != 0xFFFFFFFFu;
    if (kind) *kind = sparse ? 1 : 0;
    if (nnz) *nnz = sparse ? n : 0;
    if (sparse && positions_out && values_out && cap >= n) {
        st = nmn_hnsw_sparse_row(h, it->second, positions_out, values_out, cap, &n);
        if (st != NMN_OK) return pass(st);
    }
    if (dense_out) return pass(nmn_hnsw_get_vector(h, it->second, dense_out));
    return NMN_OK;
}

extern "C" nmn_hnsw* nmn_cache_index_hnsw(nmn_cache_index* c) {
    if (!c) return nullptr;
    std::lock_guard<std::mutex> lk(c->mu);
    return c->index->h;
}
