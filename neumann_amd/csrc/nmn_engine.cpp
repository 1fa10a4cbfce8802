// nmn_engine.cpp — host-side mirror of Neumann's `VectorEngine` for the SIMILAR TOP-K path
// (C ABI: include/neumann_engine.h).  C++ because the reference is compiled code and the image has no
// Rust toolchain; names, argument meaning, validation order and error texts follow
// vector_engine/src/lib.rs (cited per function).  ALL scoring happens on the GPU through
// include/neumann_gpu.h; this file holds the entries: the key/value bookkeeping the reference keeps in
// `TensorStore`, the validation rules, every search, the IVF and HNSW handles.  Beside it (INTEGRATION.md,
// "Source layout of the engine"): nmn_engine_internal.h (the shared types), nmn_engine_filter.cpp (the
// metadata predicate evaluator and compiler), nmn_engine_mirror.cpp (the GPU-mirror cache),
// nmn_engine_persist.cpp with nmn_engine_json.h (index files).
//
// Built with -ffp-contract=off, like every file of the family: the zero-magnitude-query rule needs
// `simd::magnitude(query)` in reference order on the host (validation, not the hot path).
#include "nmn_engine_internal.h"

namespace nmn {
namespace engine {

// the text behind nmn_engine_last_error: one object for the whole library, reached through fail() alone
static thread_local std::string g_err;

nmn_status fail(nmn_status code, std::string msg) {
    g_err = std::move(msg);
    return code;
}
// Display texts of VectorError (lib.rs:151-183)
nmn_status err_not_found(const std::string& key) { return fail(NMN_ERR_NOT_FOUND, "Embedding not found: " + key); }
nmn_status err_dim(uint64_t expected, uint64_t got) {
    return fail(NMN_ERR_DIMENSION_MISMATCH,
                "Dimension mismatch: expected " + std::to_string(expected) + ", got " + std::to_string(got));
}
nmn_status err_empty() { return fail(NMN_ERR_EMPTY_VECTOR, "Empty vector provided"); }
nmn_status err_topk() { return fail(NMN_ERR_INVALID_TOP_K, "Invalid top_k value (must be > 0)"); }
nmn_status err_timeout(const char* op, int64_t ms) {
    return fail(NMN_ERR_SEARCH_TIMEOUT, std::string("search timeout: ") + op + " exceeded " + std::to_string(ms) + "ms");
}
nmn_status err_gpu(nmn_status st) {
    // StorageError(String) carries the shim's message (lib.rs:185-189: From<TensorStoreError>)
    const char* detail = nmn_last_error();
    return fail(st, std::string("Storage error: ") + nmn_status_str(st) + (detail && *detail ? std::string(": ") + detail : ""));
}

}  // namespace engine
}  // namespace nmn

using namespace nmn::engine;

static constexpr const char* kHnswDefaultEntry = "_default";  // the default collection's name in hnsw_cache (lib.rs:1332, 1866, 1923, 1979)

// ================================================================================================
extern "C" {

void nmn_engine_config_default(nmn_engine_config* c) {  // lib.rs:648-664
    if (!c) return;
    c->default_dimension = 0;
    c->sparse_threshold = 0.5f;
    c->parallel_threshold = 5000;
    c->default_metric = NMN_METRIC_COSINE;
    c->max_dimension = 0;
    c->max_keys_per_scan = 0;
    c->search_timeout_ms = -1;
    c->device = -1;
    c->cand_cap = 0;
    c->max_index_file_bytes = 100ll * 1024 * 1024;  // lib.rs:660
    c->max_index_entries = 1000000;                 // lib.rs:661
    c->n_devices = 0;
    for (uint32_t i = 0; i < NMN_ENGINE_MAX_DEVICES; i++) c->devices[i] = -1;
}

void nmn_filtered_config_default(nmn_filtered_config* c) {  // lib.rs:412-420
    if (!c) return;
    c->strategy = NMN_FILTER_AUTO;
    c->selectivity_threshold = 0.1f;
    c->oversample_factor = 3;
}

const char* nmn_engine_last_error(void) { return g_err.c_str(); }

nmn_status nmn_engine_create(const nmn_engine_config* config, nmn_engine** out) {
    if (!out) return fail(NMN_ERR_INVALID_ARGUMENT, "out is null");
    nmn_engine* e = new (std::nothrow) nmn_engine();
    if (!e) return fail(NMN_ERR_OUT_OF_MEMORY, "engine alloc");
    if (config) e->cfg = *config;
    else nmn_engine_config_default(&e->cfg);
    // VectorEngineConfig::validate (lib.rs:710-740)
    if (!(e->cfg.sparse_threshold >= 0.0f && e->cfg.sparse_threshold <= 1.0f)) {
        delete e;
        return fail(NMN_ERR_CONFIGURATION, "Configuration error: sparse_threshold must be between 0.0 and 1.0");
    }
    if (e->cfg.parallel_threshold == 0) {
        delete e;
        return fail(NMN_ERR_CONFIGURATION, "Configuration error: parallel_threshold must be greater than 0");
    }
    if (e->cfg.max_index_file_bytes == 0) {  // lib.rs:740-746
        delete e;
        return fail(NMN_ERR_CONFIGURATION, "Configuration error: max_index_file_bytes must be greater than 0");
    }
    if (e->cfg.max_index_entries == 0) {  // lib.rs:747-753
        delete e;
        return fail(NMN_ERR_CONFIGURATION, "Configuration error: max_index_entries must be greater than 0");
    }
    if (e->cfg.n_devices > NMN_ENGINE_MAX_DEVICES) {
        delete e;
        return fail(NMN_ERR_CONFIGURATION, "Configuration error: n_devices exceeds NMN_ENGINE_MAX_DEVICES");
    }
    // devices[]: one entry = that GPU; two or more = every mirror is one index over all of them; the collection-level
    // device objects that are not sharded (metadata columns, IVF indexes, the compute_similarity slot) live on devices[0]
    if (e->cfg.n_devices >= 1) e->cfg.device = e->cfg.devices[0];
    *out = e;
    return NMN_OK;
}

void nmn_engine_destroy(nmn_engine* e) { delete e; }

nmn_status nmn_engine_store_embedding_with_metadata(nmn_engine* e, const char* key, const float* v, uint64_t dim,
                                                    const nmn_meta_field* meta, uint32_t n_meta) {
    if (!e || !key) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (!v || dim == 0) return err_empty();  // lib.rs:1841-1843
    if (e->cfg.max_dimension && dim > e->cfg.max_dimension) return err_dim(e->cfg.max_dimension, dim);
    WriteLock g(e);
    return store_into(e, &e->dflt, key, v, dim, meta, n_meta);
}

nmn_status nmn_engine_store_embedding(nmn_engine* e, const char* key, const float* v, uint64_t dim) {
    const nmn_status st = nmn_engine_store_embedding_with_metadata(e, key, v, dim, nullptr, 0);
    if (st == NMN_OK) e->invalidate_hnsw(kHnswDefaultEntry);  // lib.rs:1866 (store_embedding_with_metadata itself, 3272-3309, does not)
    return st;
}

nmn_status nmn_engine_batch_store(nmn_engine* e, const char* const* keys, const float* rows, uint64_t n,
                                  uint64_t dim) {
    if (!e || !keys || (!rows && n)) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (n && dim == 0) return err_empty();
    if (e->cfg.max_dimension && dim > e->cfg.max_dimension) return err_dim(e->cfg.max_dimension, dim);
    WriteLock g(e);
    for (uint64_t i = 0; i < n; i++) {
        if (!keys[i]) return fail(NMN_ERR_INVALID_ARGUMENT, "null key");
        if (store_into(e, &e->dflt, keys[i], rows + i * dim, dim, nullptr, 0) == NMN_OK)
            e->invalidate_hnsw(kHnswDefaultEntry);  // batch_store_embeddings stores through store_embedding: lib.rs:1866 per vector
    }
    return NMN_OK;
}

static nmn_status get_from(Collection* c, const std::string& key, const std::string& shown, float* out, uint64_t cap,
                           uint64_t* dim_out) {
    if (!c) return err_not_found(shown);
    auto it = c->by_key.find(key);
    if (it == c->by_key.end()) return err_not_found(shown);
    const Entry& ent = c->slots[it->second];
    if (dim_out) *dim_out = ent.vec.size();
    if (out) memcpy(out, ent.vec.data(), std::min<uint64_t>(cap, ent.vec.size()) * sizeof(float));
    return NMN_OK;
}

nmn_status nmn_engine_get_embedding(nmn_engine* e, const char* key, float* out, uint64_t cap, uint64_t* dim_out) {
    if (!e || !key) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    WriteLock g(e);
    return get_from(&e->dflt, key, key, out, cap, dim_out);
}

nmn_status nmn_engine_delete_embedding(nmn_engine* e, const char* key) {
    if (!e || !key) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    WriteLock g(e);
    const nmn_status st = delete_from(&e->dflt, key, key);
    if (st == NMN_OK) e->invalidate_hnsw(kHnswDefaultEntry);  // lib.rs:1923
    return st;
}

int32_t nmn_engine_exists(nmn_engine* e, const char* key) {
    if (!e || !key) return 0;
    WriteLock g(e);
    return e->dflt.by_key.count(key) ? 1 : 0;
}

uint64_t nmn_engine_count(nmn_engine* e) {
    if (!e) return 0;
    WriteLock g(e);
    return e->dflt.live;
}

// max_keys_per_scan (lib.rs:638, 2322, 2341, 2948, 3179, 3225): every unbounded walk over the store stops after that many
// keys of the scan.  The reference's scan order is its HashSet's (slab_router.rs:287-305: unspecified); here it is slot
// order, so "the first N keys" is a deterministic prefix.  0 = None.
static uint64_t scan_limit(const nmn_engine* e) { return e->cfg.max_keys_per_scan ? e->cfg.max_keys_per_scan : UINT64_MAX; }

nmn_strlist* nmn_engine_list_keys(nmn_engine* e) {  // list_keys_bounded, lib.rs:2321-2329
    nmn_strlist* l = new (std::nothrow) nmn_strlist();
    if (!e || !l) return l;
    WriteLock g(e);
    const uint64_t limit = scan_limit(e);
    for (const auto& ent : e->dflt.slots) {
        if (l->items.size() >= limit) break;
        if (ent.live) l->items.push_back(ent.key);
    }
    return l;
}

// list_keys_paginated (lib.rs:2945-2980): scan -> take(min(skip + limit.unwrap_or(max_scan), max_scan)) -> skip -> take(limit);
// total_count = count() when asked for; has_more = skip + items < total, or (no total) items == limit.unwrap_or(0)
nmn_strlist* nmn_engine_list_keys_paginated(nmn_engine* e, uint64_t skip, int64_t limit, int32_t count_total,
                                            int64_t* total_count, int32_t* has_more) {
    nmn_strlist* l = new (std::nothrow) nmn_strlist();
    if (total_count) *total_count = -1;
    if (has_more) *has_more = 0;
    if (!e || !l) return l;
    WriteLock g(e);
    const uint64_t max_scan = scan_limit(e);
    uint64_t fetch = skip + (limit >= 0 ? (uint64_t)limit : max_scan);
    if (fetch < skip) fetch = UINT64_MAX;  // saturating_add
    fetch = std::min(fetch, max_scan);
    uint64_t seen = 0;
    for (const auto& ent : e->dflt.slots) {
        if (seen >= fetch) break;
        if (!ent.live) continue;
        if (seen++ < skip) continue;
        if (limit >= 0 && l->items.size() >= (uint64_t)limit) break;
        l->items.push_back(ent.key);
    }
    const uint64_t n = l->items.size();
    if (count_total) {
        if (total_count) *total_count = (int64_t)e->dflt.live;
        uint64_t reach = skip + n;
        if (reach < skip) reach = UINT64_MAX;
        if (has_more) *has_more = reach < e->dflt.live ? 1 : 0;
    } else if (has_more) {
        *has_more = n == (limit >= 0 ? (uint64_t)limit : 0ull) ? 1 : 0;
    }
    return l;
}

nmn_status nmn_engine_clear(nmn_engine* e, uint64_t* removed) {  // lib.rs:2340-2354
    if (!e) return fail(NMN_ERR_INVALID_ARGUMENT, "null engine");
    WriteLock g(e);
    const uint64_t max_keys = scan_limit(e);
    if (e->dflt.live <= max_keys) {
        if (removed) *removed = e->dflt.live;
        const uint64_t writes = e->dflt.writes;
        e->dflt = Collection();
        e->dflt.writes = writes + 1;
        return NMN_OK;
    }
    // more keys than one bounded scan covers: the first max_keys go ("call again until 0 is returned")
    std::vector<std::string> keys;
    for (const auto& ent : e->dflt.slots) {
        if (keys.size() >= max_keys) break;
        if (ent.live) keys.push_back(ent.key);
    }
    for (const auto& k : keys) delete_from(&e->dflt, k, k);
    if (removed) *removed = keys.size();
    return NMN_OK;
}

// ---- searches ------------------------------------------------------------------------------------
// How a search entry opens once its arguments are known not to be null and its Deadline runs: *out cleared, the query validated
// (is_empty, then top_k, then max_dimension where the reference checks it), an empty result list allocated.  The entry owns the
// list through `res` and releases it into *out when it succeeds.
static nmn_status begin_search(const nmn_engine* e, const float* q, uint64_t dim, uint64_t top_k, bool check_max_dim,
                               nmn_results** out, std::unique_ptr<nmn_results>* res) {
    *out = nullptr;
    const nmn_status st = validate_query(e, q, dim, top_k, check_max_dim);
    if (st != NMN_OK) return st;
    res->reset(new_results());
    return *res ? NMN_OK : fail(NMN_ERR_OUT_OF_MEMORY, "results alloc");
}

// The cached path of search_similar (lib.rs:1976-2001) and search_in_collection (1622-1646): if `collection` has an entry whose
// mapping is not empty, answer from index.search(query, top_k) — ids mapped to keys (ids past the mapping dropped), `prefix`
// stripped where a key has it, stable sort by score descending, truncate — and set *served.  No deadline check: the reference has
// none here.  Concurrent callers meet in the coalescer of nmn_hnsw_search and walk as one launch (docs/hnsw.md §11).
static nmn_status cached_hnsw_search(nmn_engine* e, const std::string& collection, const std::string& prefix, const float* q,
                                     uint64_t dim, uint64_t top_k, nmn_results* res, bool* served) {
    std::shared_ptr<const nmn_engine::HnswCacheEntry> ent;
    {
        std::lock_guard<std::mutex> g(e->cache_mu);
        auto it = e->hnsw_cache.find(collection);
        if (it != e->hnsw_cache.end()) ent = it->second;
    }
    if (!ent || ent->keys.empty()) return NMN_OK;  // `if !mapping.is_empty()`: an empty mapping falls through
    *served = true;
    if (!ent->index) return NMN_OK;  // an empty index under a mapping: `index.search` returns nothing (hnsw.rs:2070-2073)
    if (dim != ent->dim) return err_dim(ent->dim, dim);  // as search_with_hnsw: the reference's SIMD loops would read past the shorter slice
    const uint64_t len = nmn_hnsw_len(ent->index.get());
    const uint32_t k = (uint32_t)std::min<uint64_t>(top_k, std::max<uint64_t>(len, 1));  // the rule of nmn_engine_search_with_hnsw
    std::vector<uint64_t> ids(k);
    std::vector<float> sc(k);
    uint32_t count = 0;
    const nmn_status st = nmn_hnsw_search(ent->index.get(), q, 1, k, 0, ids.data(), sc.data(), &count, nullptr);
    if (st != NMN_OK) return err_gpu(st);
    std::vector<uint32_t> order;
    for (uint32_t i = 0; i < count; i++)
        if (ids[i] < ent->keys.size()) order.push_back(i);  // `mapping.get(idx)` -> filter_map
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return sc[a] > sc[b]; });  // b.score.partial_cmp(&a.score)
    if (order.size() > top_k) order.resize(top_k);
    for (uint32_t i : order) {
        const std::string& key = ent->keys[ids[i]];
        res->keys.push_back(key.compare(0, prefix.size(), prefix) == 0 ? key.substr(prefix.size()) : key);  // strip_prefix().unwrap_or(key)
        res->scores.push_back(sc[i]);
    }
    return NMN_OK;
}

nmn_status nmn_engine_search_similar_with_metric(nmn_engine* e, const float* q, uint64_t dim, uint64_t top_k,
                                                 int32_t metric, nmn_results** out) {
    if (!e || !out) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    const Deadline dl(e->cfg.search_timeout_ms);
    std::unique_ptr<nmn_results> res;
    nmn_status st = begin_search(e, q, dim, top_k, /*check_max_dim=*/false, out, &res);  // lib.rs:2056-2061
    if (st != NMN_OK) return st;
    // zero-magnitude queries: empty for cosine/dot, scored for euclidean (lib.rs:2063-2068)
    if (!(zero_magnitude(q, dim) && metric != NMN_METRIC_EUCLIDEAN)) {
        st = locked_search(e, [&] { return &e->dflt; }, q, dim, top_k, metric, "search_similar_with_metric", dl, res.get());
        if (st != NMN_OK) return st;
    }
    *out = res.release();
    return NMN_OK;
}

nmn_status nmn_engine_search_similar(nmn_engine* e, const float* q, uint64_t dim, uint64_t top_k, nmn_results** out) {
    if (!e || !out) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    const Deadline dl(e->cfg.search_timeout_ms);
    std::unique_ptr<nmn_results> res;
    nmn_status st = begin_search(e, q, dim, top_k, /*check_max_dim=*/true, out, &res);  // lib.rs:1953-1967
    if (st != NMN_OK) return st;
    if (!zero_magnitude(q, dim)) {  // lib.rs:1970-1974
        bool served = false;
        st = cached_hnsw_search(e, kHnswDefaultEntry, "emb:", q, dim, top_k, res.get(), &served);  // lib.rs:1976-2001
        if (st == NMN_OK && !served)
            st = locked_search(e, [&] { return &e->dflt; }, q, dim, top_k, NMN_METRIC_COSINE, "search_similar", dl, res.get());
        if (st != NMN_OK) return st;
    }
    *out = res.release();
    return NMN_OK;
}

// ---- metadata CRUD of stored embeddings (lib.rs:3311-3385): filtered searches see the change at once ----
static void value_out(const Value& v, nmn_value* out) {
    out->kind = v.kind;
    out->b = v.b ? 1 : 0;
    out->i = v.i;
    out->f = v.f;
    out->s = v.kind == NMN_VAL_STRING ? v.s.c_str() : nullptr;
}

nmn_metalist* nmn_engine_get_metadata(nmn_engine* e, const char* key, nmn_status* status) {  // lib.rs:3312-3327
    nmn_status dummy;
    if (!status) status = &dummy;
    if (!e || !key) {
        *status = fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
        return nullptr;
    }
    WriteLock g(e);
    auto it = e->dflt.by_key.find(key);
    if (it == e->dflt.by_key.end()) {
        *status = err_not_found(key);
        return nullptr;
    }
    nmn_metalist* l = new (std::nothrow) nmn_metalist();
    if (!l) {
        *status = fail(NMN_ERR_OUT_OF_MEMORY, "metadata list alloc");
        return nullptr;
    }
    for (const auto& kv : e->dflt.slots[it->second].meta) {
        l->names.push_back(kv.first);
        l->values.push_back(kv.second);
    }
    *status = NMN_OK;
    return l;
}
uint64_t nmn_metalist_len(const nmn_metalist* l) { return l ? l->names.size() : 0; }
const char* nmn_metalist_name(const nmn_metalist* l, uint64_t i) { return (l && i < l->names.size()) ? l->names[i].c_str() : nullptr; }
nmn_status nmn_metalist_value(const nmn_metalist* l, uint64_t i, nmn_value* out) {
    if (!l || !out || i >= l->values.size()) return fail(NMN_ERR_INVALID_ARGUMENT, "bad metadata index");
    value_out(l->values[i], out);  // out->s points into the list: valid until nmn_metalist_free
    return NMN_OK;
}
void nmn_metalist_free(nmn_metalist* l) { delete l; }

// update_metadata (lib.rs:3329-3351): set the given fields, keep the others and the vector
nmn_status nmn_engine_update_metadata(nmn_engine* e, const char* key, const nmn_meta_field* meta, uint32_t n_meta) {
    if (!e || !key || (n_meta && !meta)) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    WriteLock g(e);
    auto it = e->dflt.by_key.find(key);
    if (it == e->dflt.by_key.end()) return err_not_found(key);
    Entry& ent = e->dflt.slots[it->second];
    Meta changed;
    for (uint32_t i = 0; i < n_meta; i++)
        if (meta[i].name) {
            ent.meta[meta[i].name] = Value::from(meta[i].value);
            changed[meta[i].name] = ent.meta[meta[i].name];
        }
    Mirror* m = ent.mrow >= 0 ? mirror_of(&e->dflt, ent.vec.size()) : nullptr;
    if (m) columns_write_row(m, (uint64_t)ent.mrow, changed, /*overwrite=*/false);  // only the touched cells
    return NMN_OK;
}

// remove_metadata_field (lib.rs:3353-3364): NotFound only for a missing key; a missing field is not an error
nmn_status nmn_engine_remove_metadata_field(nmn_engine* e, const char* key, const char* field) {
    if (!e || !key || !field) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    WriteLock g(e);
    auto it = e->dflt.by_key.find(key);
    if (it == e->dflt.by_key.end()) return err_not_found(key);
    Entry& ent = e->dflt.slots[it->second];
    if (ent.meta.erase(field) == 0) return NMN_OK;
    Mirror* m = ent.mrow >= 0 ? mirror_of(&e->dflt, ent.vec.size()) : nullptr;
    if (m && m->cols) {
        auto fc = m->fields.find(field);
        if (fc != m->fields.end()) {
            const uint8_t kind = NMN_CELL_ABSENT;
            const uint64_t payload = 0;
            if (nmn_columns_write(m->cols, fc->second.id, (uint64_t)ent.mrow, 1, &kind, &payload) != NMN_OK) m->drop_columns();
        }
    }
    return NMN_OK;
}

int32_t nmn_engine_has_metadata_field(nmn_engine* e, const char* key, const char* field) {  // lib.rs:3366-3372
    if (!e || !key || !field) return 0;
    WriteLock g(e);
    auto it = e->dflt.by_key.find(key);
    return (it != e->dflt.by_key.end() && e->dflt.slots[it->second].meta.count(field)) ? 1 : 0;
}

// get_metadata_field (lib.rs:3374-3383): Ok(None) for a missing field -> *present = 0.  out->s (strings) points to
// thread-local storage that stays valid until this thread's next call of this function.
nmn_status nmn_engine_get_metadata_field(nmn_engine* e, const char* key, const char* field, nmn_value* out,
                                         int32_t* present) {
    if (!e || !key || !field || !out || !present) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    static thread_local Value hold;
    *present = 0;
    WriteLock g(e);
    auto it = e->dflt.by_key.find(key);
    if (it == e->dflt.by_key.end()) return err_not_found(key);
    const Meta& meta = e->dflt.slots[it->second].meta;
    auto f = meta.find(field);
    if (f == meta.end()) return NMN_OK;
    hold = f->second;
    value_out(hold, out);
    *present = 1;
    return NMN_OK;
}

// batch_delete_embeddings (lib.rs:2924-2940): missing keys are skipped, the number deleted is returned
nmn_status nmn_engine_batch_delete(nmn_engine* e, const char* const* keys, uint64_t n, uint64_t* deleted) {
    if (!e || (n && !keys)) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    WriteLock g(e);
    uint64_t cnt = 0;
    for (uint64_t i = 0; i < n; i++)
        if (keys[i] && e->dflt.by_key.count(keys[i]) && delete_from(&e->dflt, keys[i], keys[i]) == NMN_OK) cnt++;
    if (deleted) *deleted = cnt;
    return NMN_OK;
}

uint64_t nmn_engine_dimension(nmn_engine* e) {  // lib.rs:2298-2308: the first stored vector's length; 0 = None
    if (!e) return 0;
    WriteLock g(e);
    for (const auto& ent : e->dflt.slots)
        if (ent.live) return ent.vec.size();
    return 0;
}

int32_t nmn_engine_exists_in_collection(nmn_engine* e, const char* coll, const char* key) {  // lib.rs:1537-1540
    if (!e || !coll || !key) return 0;
    WriteLock g(e);
    Collection* c = e->storage(coll, false);
    return (c && c->by_key.count(key)) ? 1 : 0;
}

nmn_strlist* nmn_engine_list_collection_keys(nmn_engine* e, const char* coll) {  // lib.rs:1543-1550
    nmn_strlist* l = new (std::nothrow) nmn_strlist();
    if (!e || !coll || !l) return l;
    WriteLock g(e);
    Collection* c = e->storage(coll, false);
    if (c)
        for (const auto& ent : c->slots)
            if (ent.live) l->items.push_back(ent.key);
    return l;
}

// search_similar_paginated / search_entities_paginated (lib.rs:2988-3058): search min(skip + limit.unwrap_or(top_k),
// top_k) results, then skip / take; total_count (when asked for) is the number of results FOUND, not of rows stored.
static nmn_status paginate(nmn_status st, nmn_results* found_all, uint64_t skip, int64_t limit, int32_t count_total,
                           nmn_results** out, int64_t* total_count, int32_t* has_more) {
    if (st != NMN_OK) return st;
    const std::unique_ptr<nmn_results> all(found_all);
    const uint64_t found = all->keys.size();
    if (total_count) *total_count = count_total ? (int64_t)found : -1;
    std::unique_ptr<nmn_results> res(new_results());
    if (!res) return fail(NMN_ERR_OUT_OF_MEMORY, "results alloc");
    for (uint64_t i = skip; i < found && (limit < 0 || res->keys.size() < (uint64_t)limit); i++) {
        res->keys.push_back(all->keys[i]);
        res->scores.push_back(all->scores[i]);
    }
    if (has_more) {
        uint64_t reach = skip + res->keys.size();
        if (reach < skip) reach = UINT64_MAX;  // saturating_add
        *has_more = (limit >= 0 && count_total && reach < found) ? 1 : 0;
    }
    *out = res.release();
    return NMN_OK;
}

static uint64_t total_needed(uint64_t top_k, uint64_t skip, int64_t limit) {
    const uint64_t want = limit >= 0 ? (uint64_t)limit : top_k;
    uint64_t need = skip + want;
    if (need < skip) need = UINT64_MAX;  // saturating_add
    return std::min(need, top_k);
}

nmn_status nmn_engine_search_similar_paginated(nmn_engine* e, const float* q, uint64_t dim, uint64_t top_k, uint64_t skip,
                                               int64_t limit, int32_t count_total, nmn_results** out, int64_t* total_count,
                                               int32_t* has_more) {
    if (!out) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    nmn_results* all = nullptr;
    nmn_status st = nmn_engine_search_similar(e, q, dim, total_needed(top_k, skip, limit), &all);
    return paginate(st, all, skip, limit, count_total, out, total_count, has_more);
}

nmn_status nmn_engine_search_entities_paginated(nmn_engine* e, const float* q, uint64_t dim, uint64_t top_k, uint64_t skip,
                                                int64_t limit, int32_t count_total, nmn_results** out, int64_t* total_count,
                                                int32_t* has_more) {
    if (!out) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    nmn_results* all = nullptr;
    nmn_status st = nmn_engine_search_entities(e, q, dim, total_needed(top_k, skip, limit), &all);
    return paginate(st, all, skip, limit, count_total, out, total_count, has_more);
}

// ---- tensor_blob artifact similarity (tensor_blob/src/lib.rs:520-625) -----------------------------------
// The blob store keeps an optional `_embedding` (+ `_id`, `_filename`) in each artifact's `_blob:meta:{id}`
// record; `search_by_embedding` scans those records, keeps the ones of the query's dimension and ranks them by
// the f64 sparse cosine (NMN_METRIC_SPARSE_COSINE_F64).  Here the embeddings of the artifacts are one more
// mirrored key space; the artifact bytes, chunks, tags and links are the blob store's business, not this path's.
nmn_status nmn_engine_blob_set_embedding(nmn_engine* e, const char* artifact_id, const char* filename, const float* v,
                                         uint64_t dim) {
    if (!e || !artifact_id) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (!v || dim == 0) return err_empty();
    nmn_meta_field mf{};
    mf.name = "_filename";
    mf.value.kind = NMN_VAL_STRING;
    mf.value.s = filename ? filename : "";
    WriteLock g(e);
    return store_into(e, &e->artifacts, artifact_id, v, dim, &mf, 1);
}

nmn_status nmn_engine_blob_remove(nmn_engine* e, const char* artifact_id) {  // BlobStore::delete drops the record
    if (!e || !artifact_id) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    WriteLock g(e);
    return delete_from(&e->artifacts, artifact_id, artifact_id);
}

static void fill_filenames(Collection* c, nmn_results* res) {
    res->aux.clear();
    for (const auto& key : res->keys) {
        auto it = c->by_key.find(key);
        std::string fn;
        if (it != c->by_key.end()) {
            auto m = c->slots[it->second].meta.find("_filename");
            if (m != c->slots[it->second].meta.end()) fn = m->second.s;  // get_string(..).unwrap_or_default()
        }
        res->aux.push_back(std::move(fn));
    }
}

// search_by_embedding (lib.rs:591-625): no validation in the reference — an empty query or k == 0 simply finds nothing
nmn_status nmn_engine_blob_search_by_embedding(nmn_engine* e, const float* q, uint64_t dim, uint64_t k, nmn_results** out) {
    if (!e || !out) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    std::unique_ptr<nmn_results> res(new_results());
    if (!res) return fail(NMN_ERR_OUT_OF_MEMORY, "results alloc");
    if (q && dim && k) {
        const Deadline dl(-1);
        nmn_status st = locked_search(e, [&] { return &e->artifacts; }, q, dim, k, NMN_METRIC_SPARSE_COSINE_F64,
                                      "search_by_embedding", dl, res.get());
        if (st != NMN_OK) return st;
        ReadLock rd(e);
        fill_filenames(&e->artifacts, res.get());
    }
    *out = res.release();
    return NMN_OK;
}

// similar (lib.rs:563-583): search k + 1 with the artifact's own embedding, drop the artifact itself, take k
nmn_status nmn_engine_blob_similar(nmn_engine* e, const char* artifact_id, uint64_t k, nmn_results** out) {
    if (!e || !artifact_id || !out) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    std::vector<float> emb;
    {
        WriteLock g(e);
        auto it = e->artifacts.by_key.find(artifact_id);
        if (it == e->artifacts.by_key.end()) return err_not_found(artifact_id);  // BlobError::NotFound
        emb = e->artifacts.slots[it->second].vec;
    }
    nmn_results* found = nullptr;
    nmn_status st = nmn_engine_blob_search_by_embedding(e, emb.data(), emb.size(), k + 1, &found);
    if (st != NMN_OK) return st;
    const std::unique_ptr<nmn_results> all(found);
    std::unique_ptr<nmn_results> res(new_results());
    if (!res) return fail(NMN_ERR_OUT_OF_MEMORY, "results alloc");
    for (size_t i = 0; i < all->keys.size() && res->keys.size() < k; i++) {
        if (all->keys[i] == artifact_id) continue;
        res->keys.push_back(all->keys[i]);
        res->scores.push_back(all->scores[i]);
        res->aux.push_back(all->aux[i]);
    }
    *out = res.release();
    return NMN_OK;
}

// ---- IVF (lib.rs:2641-2812) --------------------------------------------------------------------------
void nmn_ivf_options_default(nmn_ivf_options* o) {  // IVFConfig::default + KMeansConfig::default
    if (!o) return;
    o->num_clusters = 100;
    o->nprobe = 0;  // default_nprobe(num_clusters) = ceil(sqrt(num_clusters)), ivf.rs:46-56
    o->max_iterations = 100;
    o->convergence_threshold = 1e-4f;
    o->seed = 42;
    o->init_method = NMN_KMEANS_INIT_PLUSPLUS;
}

nmn_status nmn_engine_build_ivf_index(nmn_engine* e, const nmn_ivf_options* options, nmn_engine_ivf** out) {
    return nmn_engine_build_ivf_index_ex(e, options, nullptr, out);
}

// build_ivf_index for IVFBuildOptions::{flat, pq, binary} (lib.rs:941-1000, 2641-2694): the same validation in the same order,
// then nmn_ivf_build_ex (storage NULL = Flat)
nmn_status nmn_engine_build_ivf_index_ex(nmn_engine* e, const nmn_ivf_options* options, const nmn_ivf_storage* storage,
                                         nmn_engine_ivf** out) {
    if (!e || !out) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    nmn_ivf_options o;
    if (options) o = *options;
    else nmn_ivf_options_default(&o);
    auto res = std::unique_ptr<nmn_engine_ivf>(new (std::nothrow) nmn_engine_ivf());
    if (!res) return fail(NMN_ERR_OUT_OF_MEMORY, "ivf alloc");
    res->nprobe = o.nprobe ? o.nprobe : (uint64_t)std::ceil(std::sqrt((float)o.num_clusters));
    WriteLock g(e);
    // `let keys = self.list_keys()` then every vector in that order; one dimension only (lib.rs:2653-2668)
    std::vector<float> rows;
    uint64_t dim = 0;
    for (const auto& ent : e->dflt.slots) {
        if (!ent.live) continue;
        if (dim == 0) dim = ent.vec.size();
        else if (ent.vec.size() != dim) return err_dim(dim, ent.vec.size());
        res->keys.push_back(ent.key);
        rows.insert(rows.end(), ent.vec.begin(), ent.vec.end());
    }
    const uint64_t n = res->keys.size();
    if (n == 0) {  // `return Ok((IVFIndex::new(options.config), Vec::new()))`: untrained, searches find nothing
        *out = res.release();
        return NMN_OK;
    }
    if (e->cfg.max_dimension && dim > e->cfg.max_dimension) return err_dim(e->cfg.max_dimension, dim);  // lib.rs:2671-2680
    res->dim = dim;
    // index.train(&vectors) then index.add(v) for every vector — both on the GPU, the k-means bit for bit
    // (nmn_ivf_build: exact centroid sweeps for the assignments, sequential per-(cluster, dimension) sums for the update)
    if (dim > 0xFFFFFFFFull) return fail(NMN_ERR_INVALID_ARGUMENT, "dimension does not fit the device index (> 2^32 - 1)");
    nmn_index_desc d{};
    d.dim = (uint32_t)dim;
    d.capacity_rows = n;
    d.device = e->cfg.device;
    d.cand_cap = e->cfg.cand_cap;
    nmn_kmeans_options ko{};
    ko.max_iterations = o.max_iterations;
    ko.convergence_threshold = o.convergence_threshold;
    ko.seed = o.seed;
    ko.init_method = o.init_method == NMN_KMEANS_INIT_RANDOM ? 0 : 1;
    nmn_status st = nmn_ivf_build_ex(&d, rows.data(), n, (uint32_t)std::min<uint64_t>(o.num_clusters, UINT32_MAX), &ko, storage, &res->index);
    if (st == NMN_ERR_CONFIGURATION) return fail(st, std::string("Configuration error: ") + nmn_last_error());  // (dim % M != 0: the reference panics)
    if (st != NMN_OK) return err_gpu(st);
    res->n_clusters = nmn_ivf_clusters(res->index);
    res->centroids.resize((size_t)res->n_clusters * dim);
    st = nmn_ivf_centroids(res->index, res->centroids.data(), res->centroids.size());
    if (st != NMN_OK) return err_gpu(st);
    *out = res.release();
    return NMN_OK;
}

void nmn_engine_ivf_free(nmn_engine_ivf* ivf) { delete ivf; }
uint64_t nmn_engine_ivf_len(const nmn_engine_ivf* ivf) { return (ivf && ivf->index) ? nmn_ivf_len(ivf->index) : 0; }
uint32_t nmn_engine_ivf_clusters(const nmn_engine_ivf* ivf) { return ivf ? ivf->n_clusters : 0; }
uint64_t nmn_engine_ivf_nprobe(const nmn_engine_ivf* ivf) { return ivf ? ivf->nprobe : 0; }
const char* nmn_engine_ivf_key(const nmn_engine_ivf* ivf, uint64_t id) {
    return (ivf && id < ivf->keys.size()) ? ivf->keys[id].c_str() : nullptr;
}
nmn_status nmn_engine_ivf_centroids(const nmn_engine_ivf* ivf, float* out, uint64_t cap_floats) {
    if (!ivf || !out) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (cap_floats < ivf->centroids.size()) return fail(NMN_ERR_BUFFER_TOO_SMALL, "centroid buffer too small");
    memcpy(out, ivf->centroids.data(), ivf->centroids.size() * sizeof(float));
    return NMN_OK;
}
nmn_status nmn_engine_ivf_cluster_sizes(nmn_engine_ivf* ivf, uint64_t* out) {
    if (!ivf || !out) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (!ivf->index) return NMN_OK;
    nmn_status st = nmn_ivf_cluster_sizes(ivf->index, out);
    return st == NMN_OK ? NMN_OK : err_gpu(st);
}

// estimate_ivf_memory (lib.rs:2821-2851): centroids C x d x 4 + the storage (Flat n x d x 4, PQ n x M, Binary n x ceil(d / 64) x 8)
// + n x 8 of ids; 0 for an empty engine.  Host arithmetic only.
nmn_status nmn_engine_estimate_ivf_memory(nmn_engine* e, const nmn_ivf_options* options, const nmn_ivf_storage* storage,
                                          uint64_t* out_bytes) {
    if (!e || !out_bytes) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out_bytes = 0;
    nmn_ivf_options o;
    if (options) o = *options;
    else nmn_ivf_options_default(&o);
    ReadLock g(e);
    const uint64_t count = e->dflt.live;
    if (count == 0) return NMN_OK;
    uint64_t dim = 0;  // `get_embedding(&keys[0])`: the first key's vector
    for (const auto& ent : e->dflt.slots)
        if (ent.live) {
            dim = ent.vec.size();
            break;
        }
    uint64_t vector_bytes = count * dim * 4;
    if (storage && storage->kind == NMN_IVF_PQ) vector_bytes = count * storage->pq_num_subspaces;
    else if (storage && storage->kind == NMN_IVF_BINARY) vector_bytes = count * ((dim + 63) / 64) * 8;
    *out_bytes = o.num_clusters * dim * 4 + vector_bytes + count * 8;
    return NMN_OK;
}

// search_with_ivf / search_with_ivf_nprobe (lib.rs:2731-2812); nprobe == 0 = the index's own
nmn_status nmn_engine_search_with_ivf(nmn_engine* e, nmn_engine_ivf* ivf, const float* q, uint64_t dim, uint64_t top_k,
                                      uint64_t nprobe, nmn_results** out) {
    if (!e || !ivf || !out) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    const Deadline dl(e->cfg.search_timeout_ms);
    std::unique_ptr<nmn_results> res;
    nmn_status st = begin_search(e, q, dim, top_k, /*check_max_dim=*/false, out, &res);  // lib.rs:2717-2722
    if (st != NMN_OK) return st;
    if (ivf->index) {  // untrained index: `return Vec::new()` (ivf.rs:326-328)
        if (dim != ivf->dim) return err_dim(ivf->dim, dim);  // the reference zips and silently truncates; refused here
        const uint64_t len = nmn_ivf_len(ivf->index);
        const uint32_t k = (uint32_t)std::min<uint64_t>(top_k, std::max<uint64_t>(len, 1));
        std::vector<uint64_t> ids(k);
        std::vector<float> dist(k);
        uint32_t count = 0;
        st = nmn_ivf_search(ivf->index, q, 1, k, (uint32_t)std::min<uint64_t>(nprobe ? nprobe : ivf->nprobe, UINT32_MAX), ids.data(),
                            dist.data(), &count, nullptr);
        if (st != NMN_OK) return err_gpu(st);
        if (dl.expired()) return err_timeout(nprobe ? "search_with_ivf_nprobe" : "search_with_ivf", dl.ms);  // lib.rs:2726-2731
        for (uint32_t i = 0; i < count; i++) {
            if (ids[i] >= ivf->keys.size()) continue;  // `key_mapping.get(vector_id)` -> filter_map
            res->keys.push_back(ivf->keys[ids[i]]);
            const float denom = 1.0f + dist[i];
            res->scores.push_back(1.0f / denom);  // "IVF returns distances, convert to similarity"
        }
    }
    *out = res.release();
    return NMN_OK;
}

// ---- HNSW (lib.rs:2378-2550) -------------------------------------------------------------------------
// build_hnsw_index_with_options (lib.rs:2423-2470) for a storage the index serves (Dense, Quantized)
static nmn_status build_hnsw_with_storage(nmn_engine* e, const nmn_hnsw_config& c, int32_t storage, nmn_engine_hnsw** out) {
    auto res = std::unique_ptr<nmn_engine_hnsw>(new (std::nothrow) nmn_engine_hnsw());
    if (!res) return fail(NMN_ERR_OUT_OF_MEMORY, "hnsw alloc");
    WriteLock g(e);
    std::vector<float> rows;
    uint64_t dim = 0;
    bool first = true;
    for (const auto& ent : e->dflt.slots) {  // `let keys = self.list_keys()`, every vector in that order
        if (!ent.live) continue;
        if (first) {
            first = false;
            dim = ent.vec.size();  // lib.rs:2434-2446
            if (e->cfg.max_dimension && dim > e->cfg.max_dimension) return err_dim(e->cfg.max_dimension, dim);
        } else if (ent.vec.size() != dim) {
            return err_dim(dim, ent.vec.size());  // lib.rs:2458-2463
        }
        res->keys.push_back(ent.key);
        rows.insert(rows.end(), ent.vec.begin(), ent.vec.end());
    }
    res->writes_at_build = e->dflt.writes;
    const uint64_t n = res->keys.size();
    if (n == 0) {  // `return Ok((HNSWIndex::with_config(..), Vec::new()))`
        *out = res.release();
        return NMN_OK;
    }
    res->dim = dim;
    if (dim > 0xFFFFFFFFull) return fail(NMN_ERR_INVALID_ARGUMENT, "dimension does not fit the device index (> 2^32 - 1)");
    nmn_status st = nmn_hnsw_create_with_storage(&c, storage, (uint32_t)dim, n, e->cfg.device, &res->index);
    if (st == NMN_ERR_CONFIGURATION) return fail(st, std::string("Configuration error: ") + nmn_last_error());
    if (st != NMN_OK) return err_gpu(st);
    st = nmn_hnsw_insert(res->index, rows.data(), n, nullptr);
    if (st == NMN_ERR_CAPACITY) return fail(st, std::string("Insert failed: ") + nmn_last_error());  // the reference panics here (hnsw.rs:1916-1918)
    if (st != NMN_OK) return err_gpu(st);
    res->own();
    *out = res.release();
    return NMN_OK;
}

nmn_status nmn_engine_build_hnsw_index(nmn_engine* e, const nmn_hnsw_config* cfg, nmn_engine_hnsw** out) {
    if (!e || !out) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    nmn_hnsw_config c;
    if (cfg) c = *cfg;
    else nmn_hnsw_config_default(&c);
    if (c.storage != NMN_HNSW_STORAGE_DENSE)
        return fail(NMN_ERR_CONFIGURATION, "Configuration error: build_hnsw_index is HNSWStorageStrategy::Dense; the strategy is chosen by nmn_engine_build_hnsw_index_with_options");
    return build_hnsw_with_storage(e, c, NMN_HNSW_STORAGE_DENSE, out);
}

static void fill_build_options(nmn_hnsw_build_options* o, int32_t storage, void (*preset)(nmn_hnsw_config*)) {
    if (!o) return;
    o->storage = storage;
    o->reserved = 0;
    preset(&o->hnsw_config);
}
void nmn_hnsw_build_options_default(nmn_hnsw_build_options* o) { fill_build_options(o, NMN_HNSW_STORAGE_DENSE, nmn_hnsw_config_default); }
void nmn_hnsw_build_options_memory_optimized(nmn_hnsw_build_options* o) {
    fill_build_options(o, NMN_HNSW_STORAGE_QUANTIZED, nmn_hnsw_config_high_speed);
}
void nmn_hnsw_build_options_high_recall(nmn_hnsw_build_options* o) { fill_build_options(o, NMN_HNSW_STORAGE_DENSE, nmn_hnsw_config_high_recall); }
void nmn_hnsw_build_options_sparse_optimized(nmn_hnsw_build_options* o) { fill_build_options(o, NMN_HNSW_STORAGE_AUTO, nmn_hnsw_config_default); }

nmn_status nmn_engine_build_hnsw_index_with_options(nmn_engine* e, const nmn_hnsw_build_options* opt, nmn_engine_hnsw** out) {
    if (!e || !out) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    nmn_hnsw_build_options o;
    if (opt) o = *opt;
    else nmn_hnsw_build_options_default(&o);
    if (o.storage == NMN_HNSW_STORAGE_AUTO)
        return fail(NMN_ERR_CONFIGURATION, "Configuration error: HNSWStorageStrategy::Auto (sparse storage) is not served on the GPU; Dense and Quantized are");
    if (o.storage != NMN_HNSW_STORAGE_DENSE && o.storage != NMN_HNSW_STORAGE_QUANTIZED)
        return fail(NMN_ERR_CONFIGURATION, "Configuration error: unknown HNSW storage strategy");
    o.hnsw_config.storage = NMN_HNSW_STORAGE_DENSE;  // (the older field plays no part)
    return build_hnsw_with_storage(e, o.hnsw_config, o.storage, out);
}

void nmn_engine_hnsw_free(nmn_engine_hnsw* h) { delete h; }
uint64_t nmn_engine_hnsw_len(const nmn_engine_hnsw* h) { return (h && h->index) ? nmn_hnsw_len(h->index) : 0; }
const char* nmn_engine_hnsw_key(const nmn_engine_hnsw* h, uint64_t id) {
    return (h && id < h->keys.size()) ? h->keys[id].c_str() : nullptr;
}
nmn_hnsw* nmn_engine_hnsw_index(nmn_engine_hnsw* h) { return h ? h->index : nullptr; }

// ---- hnsw_cache (lib.rs:1305-1334) ----
nmn_status nmn_engine_cache_hnsw_index_mapped(nmn_engine* e, const char* collection, nmn_engine_hnsw* h, const char* const* keys,
                                              uint64_t n_keys) {
    if (!e || !collection || !h || (!keys && n_keys)) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    auto ent = std::make_shared<nmn_engine::HnswCacheEntry>();
    h->own();
    ent->index = h->owner;
    ent->dim = h->dim;
    for (uint64_t i = 0; i < n_keys; i++) {
        if (!keys[i]) return fail(NMN_ERR_INVALID_ARGUMENT, "null key");
        ent->keys.emplace_back(keys[i]);
    }
    std::lock_guard<std::mutex> g(e->cache_mu);
    e->hnsw_cache[collection] = std::move(ent);  // `.insert(collection, (index, keys))`: replaces an entry of that name
    return NMN_OK;
}

nmn_status nmn_engine_cache_hnsw_index(nmn_engine* e, const char* collection, nmn_engine_hnsw* h) {
    if (!e || !collection || !h) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::vector<const char*> keys;
    keys.reserve(h->keys.size());
    for (const auto& k : h->keys) keys.push_back(k.c_str());
    return nmn_engine_cache_hnsw_index_mapped(e, collection, h, keys.data(), keys.size());
}

nmn_status nmn_engine_invalidate_hnsw_cache(nmn_engine* e, const char* collection) {
    if (!e || !collection) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    e->invalidate_hnsw(collection);
    return NMN_OK;
}

nmn_status nmn_engine_build_and_cache_index(nmn_engine* e, const nmn_hnsw_config* cfg) {  // lib.rs:1330-1334
    nmn_engine_hnsw* h = nullptr;
    nmn_status st = nmn_engine_build_hnsw_index(e, cfg, &h);
    if (st != NMN_OK) return st;
    st = nmn_engine_cache_hnsw_index(e, kHnswDefaultEntry, h);
    nmn_engine_hnsw_free(h);  // the cache keeps its own reference
    return st;
}

int32_t nmn_engine_hnsw_cache_contains(nmn_engine* e, const char* collection) {
    if (!e || !collection) return 0;
    std::lock_guard<std::mutex> g(e->cache_mu);
    return e->hnsw_cache.count(collection) ? 1 : 0;
}

nmn_strlist* nmn_engine_hnsw_cache_keys(nmn_engine* e, const char* collection, uint64_t* n) {
    if (n) *n = 0;
    if (!e || !collection) return nullptr;
    std::shared_ptr<const nmn_engine::HnswCacheEntry> ent;
    {
        std::lock_guard<std::mutex> g(e->cache_mu);
        auto it = e->hnsw_cache.find(collection);
        if (it == e->hnsw_cache.end()) return nullptr;
        ent = it->second;
    }
    auto* l = new (std::nothrow) nmn_strlist();
    if (!l) return nullptr;
    l->items = ent->keys;
    if (n) *n = l->items.size();
    return l;
}

nmn_status nmn_engine_search_with_hnsw(nmn_engine* e, nmn_engine_hnsw* h, const float* q, uint64_t dim, uint64_t top_k,
                                       nmn_results** out) {
    if (!e || !h || !out) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    const Deadline dl(e->cfg.search_timeout_ms);
    std::unique_ptr<nmn_results> res;
    nmn_status st = begin_search(e, q, dim, top_k, /*check_max_dim=*/false, out, &res);  // lib.rs:2525-2530
    if (st != NMN_OK) return st;
    if (h->index) {  // empty index: `return Vec::new()` (hnsw.rs:2070-2073)
        if (dim != h->dim) return err_dim(h->dim, dim);  // the reference's SIMD loops would read past the shorter slice; refused here
        const uint64_t len = nmn_hnsw_len(h->index);
        // search_layer runs with max(ef_search, top_k); any ef >= len keeps every node the walk reaches and never ends it early, so
        // a top_k beyond len is served as len
        const uint32_t k = (uint32_t)std::min<uint64_t>(top_k, std::max<uint64_t>(len, 1));
        std::vector<uint64_t> ids(k);
        std::vector<float> sc(k);
        uint32_t count = 0;
        st = nmn_hnsw_search(h->index, q, 1, k, 0, ids.data(), sc.data(), &count, nullptr);
        if (st != NMN_OK) return err_gpu(st);
        if (dl.expired()) return err_timeout("search_with_hnsw", dl.ms);  // lib.rs:2534-2539
        for (uint32_t i = 0; i < count; i++) {
            if (ids[i] >= h->keys.size()) continue;  // `key_mapping.get(node_id)` -> filter_map
            res->keys.push_back(h->keys[ids[i]]);
            res->scores.push_back(sc[i]);
        }
    }
    *out = res.release();
    return NMN_OK;
}

// search_with_hnsw_and_metric (lib.rs:2560-2619).  keys NULL: the handle's own key_mapping.
nmn_status nmn_engine_search_with_hnsw_and_metric_mapped(nmn_engine* e, nmn_engine_hnsw* h, const float* q, uint64_t dim,
                                                         uint64_t top_k, const nmn_xmetric* metric, const char* const* keys,
                                                         uint64_t n_keys, nmn_results** out) {
    if (!e || !h || !out || !metric) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    const Deadline dl(e->cfg.search_timeout_ms);
    if (!q || dim == 0) return err_empty();  // lib.rs:2570-2572
    if (top_k == 0) return err_topk();       // lib.rs:2573-2575
    if (metric->kind < NMN_XMETRIC_COSINE || metric->kind > NMN_XMETRIC_COMPOSITE)
        return fail(NMN_ERR_CONFIGURATION, "Configuration error: unknown extended distance metric");
    std::unique_ptr<nmn_results> res(new_results());
    if (!res) return fail(NMN_ERR_OUT_OF_MEMORY, "results alloc");
    if (!h->index) {  // empty index: `index.search` returns nothing (hnsw.rs:2070-2073)
        *out = res.release();
        return NMN_OK;
    }
    if (dim != h->dim) return err_dim(h->dim, dim);  // as search_with_hnsw: the reference's SIMD loops would read past the shorter slice
    const char* const op = "search_with_hnsw_and_metric";
    const uint64_t len = nmn_hnsw_len(h->index);
    const uint64_t k64 = std::min<uint64_t>(top_k, std::max<uint64_t>(len, 1));  // at most len candidates come back
    const uint32_t k = (uint32_t)k64;
    auto key_of = [&](uint64_t id) -> const char* {  // `key_mapping.get(*node_id)?`
        if (keys) return id < n_keys ? keys[id] : nullptr;
        return id < h->keys.size() ? h->keys[id].c_str() : nullptr;
    };
    ReadLock g(e);
    if (!keys && h->writes_at_build == e->dflt.writes && nmn_hnsw_storage(h->index) == NMN_HNSW_STORAGE_DENSE) {
        // fast path: nothing was stored, deleted or cleared since build_hnsw_index, so the handle's rows ARE the current vectors of
        // its keys: walk, re-rank and ordering as one stream-ordered chain
        std::vector<uint64_t> ids(k);
        std::vector<float> sc(k);
        uint32_t count = 0;
        nmn_status st = nmn_hnsw_search_metric(h->index, q, 1, k, metric, ids.data(), sc.data(), &count, nullptr);
        if (st != NMN_OK) return err_gpu(st);
        if (dl.expired()) return err_timeout(op, dl.ms);  // lib.rs:2581-2586, 2603-2608
        for (uint32_t i = 0; i < count; i++) {
            const char* key = key_of(ids[i]);
            if (!key) continue;
            res->keys.push_back(key);
            res->scores.push_back(sc[i]);
        }
        *out = res.release();
        return NMN_OK;
    }
    // changed path (and every call on a quantized handle, which keeps no f32 rows): the walk, then the CURRENT vector of every candidate's key (`self.get_embedding(key).ok()?`, lib.rs:2595) gathered
    // into a staging matrix and scored there by the same kernel
    const uint64_t c64 = std::min<uint64_t>(std::max<uint64_t>(top_k > UINT64_MAX / 2 ? UINT64_MAX : 2 * top_k, 10), std::max<uint64_t>(len, 1));
    const uint32_t c = (uint32_t)c64;
    std::vector<uint64_t> ids(c);
    std::vector<float> sc(c);
    uint32_t count = 0;
    nmn_status st = nmn_hnsw_search(h->index, q, 1, c, 0, ids.data(), sc.data(), &count, nullptr);
    if (st != NMN_OK) return err_gpu(st);
    if (dl.expired()) return err_timeout(op, dl.ms);  // lib.rs:2581-2586
    std::vector<const char*> cand_keys;
    std::vector<const Entry*> cand;
    uint64_t width = dim;
    for (uint32_t i = 0; i < count; i++) {
        const char* key = key_of(ids[i]);
        if (!key) continue;
        auto it = e->dflt.by_key.find(key);
        if (it == e->dflt.by_key.end()) continue;  // the key is gone
        const Entry& ent = e->dflt.slots[it->second];
        cand_keys.push_back(key);
        cand.push_back(&ent);
        width = std::max<uint64_t>(width, ent.vec.size());
    }
    const uint32_t m = (uint32_t)cand.size();
    if (m > 0) {
        // a vector of another length: both sides zero-padded to the longer one (from_dense drops the zeros: the reference's merge)
        if (width > 0xFFFFFFFFull) return fail(NMN_ERR_INVALID_ARGUMENT, "dimension does not fit the device index (> 2^32 - 1)");
        std::vector<float> stage((size_t)m * width, 0.0f), qpad(width, 0.0f);
        std::copy(q, q + dim, qpad.begin());
        for (uint32_t i = 0; i < m; i++) std::copy(cand[i]->vec.begin(), cand[i]->vec.end(), stage.begin() + (size_t)i * width);
        std::vector<float> sim(m);
        st = nmn_xmetric_score_host_rows(e->cfg.device, stage.data(), m, (uint32_t)width, qpad.data(), metric, nullptr, sim.data());
        if (st != NMN_OK) return err_gpu(st);
        if (dl.expired()) return err_timeout(op, dl.ms);  // lib.rs:2603-2608
        // `results.sort_by(|a, b| b.score.partial_cmp(&a.score).unwrap_or(Equal))`, stable; truncate(top_k)
        std::vector<uint32_t> order(m);
        for (uint32_t i = 0; i < m; i++) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return sim[a] > sim[b]; });
        for (uint32_t i = 0; i < m && i < top_k; i++) {
            res->keys.push_back(cand_keys[order[i]]);
            res->scores.push_back(sim[order[i]]);
        }
    } else if (dl.expired()) {
        return err_timeout(op, dl.ms);
    }
    *out = res.release();
    return NMN_OK;
}

nmn_status nmn_engine_search_with_hnsw_and_metric(nmn_engine* e, nmn_engine_hnsw* h, const float* q, uint64_t dim, uint64_t top_k,
                                                  const nmn_xmetric* metric, nmn_results** out) {
    return nmn_engine_search_with_hnsw_and_metric_mapped(e, h, q, dim, top_k, metric, nullptr, 0, out);
}

// estimate_hnsw_memory (lib.rs:2489-2509): vectors + count x M(16) x 2 x 8 of graph + 32 bytes a key; host arithmetic only
nmn_status nmn_engine_estimate_hnsw_memory(nmn_engine* e, uint64_t* out_bytes) {
    if (!e || !out_bytes) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out_bytes = 0;
    ReadLock g(e);
    const uint64_t count = e->dflt.live;
    if (count == 0) return NMN_OK;
    uint64_t dim = 0;
    for (const auto& ent : e->dflt.slots)
        if (ent.live) {
            dim = ent.vec.size();
            break;
        }
    *out_bytes = count * dim * 4 + count * 16 * 2 * 8 + count * 32;
    return NMN_OK;
}

// ---- unified entity mode (lib.rs:3060-3237) --------------------------------------------------------
// Entity keys ("user:1") carry their vector in the `_embedding` field of the entity's TensorData
// (fields::EMBEDDING, tensor_store/src/lib.rs:183).  On this path only that field matters, so the
// entities are one more key space with its own GPU mirror; `search_entities` is the same cosine scan
// over it (lib.rs:3155-3219: rows without `_embedding` or of another dimension are skipped).
nmn_status nmn_engine_set_entity_embedding(nmn_engine* e, const char* entity_key, const float* v, uint64_t dim) {
    if (!e || !entity_key) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (!v || dim == 0) return err_empty();  // lib.rs:3073-3075
    if (e->cfg.max_dimension && dim > e->cfg.max_dimension) return err_dim(e->cfg.max_dimension, dim);  // 3077-3084
    WriteLock g(e);
    return store_into(e, &e->entities, entity_key, v, dim, nullptr, 0);
}

nmn_status nmn_engine_get_entity_embedding(nmn_engine* e, const char* entity_key, float* out, uint64_t cap,
                                           uint64_t* dim_out) {
    if (!e || !entity_key) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    WriteLock g(e);
    return get_from(&e->entities, entity_key, entity_key, out, cap, dim_out);  // NotFound(entity_key), lib.rs:3110-3119
}

int32_t nmn_engine_entity_has_embedding(nmn_engine* e, const char* entity_key) {  // lib.rs:3123-3128
    if (!e || !entity_key) return 0;
    WriteLock g(e);
    return e->entities.by_key.count(entity_key) ? 1 : 0;
}

nmn_status nmn_engine_remove_entity_embedding(nmn_engine* e, const char* entity_key) {  // lib.rs:3135-3147
    if (!e || !entity_key) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    WriteLock g(e);
    return delete_from(&e->entities, entity_key, entity_key);
}

nmn_strlist* nmn_engine_scan_entities_with_embeddings(nmn_engine* e) {  // lib.rs:3224-3232
    nmn_strlist* l = new (std::nothrow) nmn_strlist();
    if (!e || !l) return l;
    WriteLock g(e);
    // `.scan("").take(max_scan).filter(entity_has_embedding)`: the reference's bound counts every key of its store in an
    // unspecified order; this key space only holds entities WITH an embedding, so the bound counts those
    const uint64_t limit = scan_limit(e);
    for (const auto& ent : e->entities.slots) {
        if (l->items.size() >= limit) break;
        if (ent.live) l->items.push_back(ent.key);
    }
    return l;
}

uint64_t nmn_engine_count_entities_with_embeddings(nmn_engine* e) {  // lib.rs:3235-3237: scan_entities_with_embeddings().len()
    if (!e) return 0;
    WriteLock g(e);
    return std::min<uint64_t>(e->entities.live, scan_limit(e));
}

nmn_status nmn_engine_search_entities(nmn_engine* e, const float* q, uint64_t dim, uint64_t top_k, nmn_results** out) {
    if (!e || !out) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    const Deadline dl(e->cfg.search_timeout_ms);
    std::unique_ptr<nmn_results> res;
    nmn_status st = begin_search(e, q, dim, top_k, /*check_max_dim=*/true, out, &res);  // lib.rs:3158-3173
    if (st != NMN_OK) return st;
    if (!zero_magnitude(q, dim)) {  // lib.rs:3175-3178
        bool bounded = false;
        {
            ReadLock rd(e);
            bounded = e->entities.live > scan_limit(e);
        }
        if (bounded) {
            // `let keys = self.store.scan("").into_iter().take(max_scan)` (lib.rs:3179-3180): only the first max_scan keys of
            // the scan take part (then the `_embedding` / dimension filter): a selection bitmap over the mirror's rows.
            // (The reference's scan("") counts EVERY key of the store towards max_scan; this mirror of the engine holds entity
            //  keys only, so the bound is applied to them — INTEGRATION.md §5 states the deviation.)
            // On the ladder of locked_search: the mirror is built / patched under the exclusive lock, the bitmap and the GPU
            // search run under the shared one, so bounded searches overlap with every other reader.
            st = on_mirror(e, [&] { return &e->entities; }, dim, [&](Collection* c, Mirror* m) -> nmn_status {
                if (dl.expired()) return err_timeout("search_entities", dl.ms);
                if (!m->has_rows()) return NMN_OK;
                std::vector<uint64_t> sel(m->live.size(), 0ull);
                uint64_t seen = 0, picked = 0;
                const uint64_t limit = scan_limit(e);
                for (const auto& ent : c->slots) {
                    if (seen >= limit) break;
                    if (!ent.live) continue;
                    seen++;
                    if (ent.vec.size() == dim && ent.mrow >= 0 && ((m->live[(uint64_t)ent.mrow >> 6] >> ((uint64_t)ent.mrow & 63)) & 1ull)) {
                        sel[(uint64_t)ent.mrow >> 6] |= 1ull << ((uint64_t)ent.mrow & 63);
                        picked++;
                    }
                }
                const HostSelection hs{sel.data(), picked};
                nmn_status s2 = gpu_topk(c, m, q, top_k, NMN_METRIC_COSINE, nullptr, res.get(), &hs);
                if (s2 == NMN_OK && dl.expired()) s2 = err_timeout("search_entities", dl.ms);
                return s2;
            });
        } else {
            st = locked_search(e, [&] { return &e->entities; }, q, dim, top_k, NMN_METRIC_COSINE, "search_entities", dl, res.get());
        }
        if (st != NMN_OK) return st;
    }
    *out = res.release();
    return NMN_OK;
}

// search_similar_filtered (lib.rs:3438-3579) and search_filtered_in_collection (lib.rs:1708-1813; `coll` given).  The reference
// wrote the two separately, and they disagree in a few places; each is decided below where its comment says "default entry" or
// "collection entry".
static nmn_status filtered_search(nmn_engine* e, const char* coll, const float* q, uint64_t dim, uint64_t top_k,
                                  const nmn_filter& filter, const nmn_filtered_config* config, nmn_results** out) {
    const bool in_coll = coll != nullptr;
    // the strategy deadline and the pre arm time out under the entry's own name; the post arm searches through search_similar /
    // search_in_collection and times out under theirs
    const char* const op = in_coll ? "search_filtered_in_collection" : "search_similar_filtered";
    const char* const post_op = in_coll ? "search_in_collection" : "search_similar";
    *out = nullptr;
    const Deadline dl(e->cfg.search_timeout_ms);
    // max_dimension: the default entry checks it (lib.rs:3438-3453), the collection entry does not (lib.rs:1708-1713)
    nmn_status st = validate_query(e, q, dim, top_k, /*check_max_dim=*/!in_coll);
    if (st != NMN_OK) return st;
    nmn_filtered_config cfg;
    if (config) cfg = *config;
    else nmn_filtered_config_default(&cfg);
    const bool zero = zero_magnitude(q, dim);
    auto run = [&](bool shared) -> nmn_status {
        int32_t post_metric = NMN_METRIC_COSINE;  // default entry: the post arm is search_similar, cosine
        if (in_coll) {
            // collection entry only: the configured dimension comes first; its post arm ranks by the configured metric
            auto cit = e->configs.find(coll);
            if (cit != e->configs.end()) {
                if (cit->second.dimension && dim != cit->second.dimension) return err_dim(cit->second.dimension, dim);
                post_metric = cit->second.metric;
            }
        }
        std::unique_ptr<nmn_results> res(new_results());
        if (!res) return fail(NMN_ERR_OUT_OF_MEMORY, "results alloc");
        Collection* c = e->storage(coll, false);
        // collection entry only: an absent collection or a zero-magnitude query finds nothing BEFORE the strategy and its
        // deadline check (lib.rs:1729-1733).  The default entry looks at the magnitude per arm, after that check, so an expired
        // deadline beats an empty answer there.
        if (in_coll && (!c || zero)) {
            *out = res.release();
            return NMN_OK;
        }
        // Auto: the default entry sends True to the post-filter without sampling (lib.rs:3480-3511); the collection entry samples
        // True like any other condition (lib.rs:1737-1764)
        int strategy = cfg.strategy;
        if (strategy == NMN_FILTER_AUTO)
            strategy = (!in_coll && filter.kind == nmn_filter::True) ? NMN_FILTER_POST : choose_strategy(c, filter, cfg);
        if (dl.expired()) return err_timeout(op, dl.ms);
        nmn_status rs = NMN_OK;
        if (strategy == NMN_FILTER_POST) {
            // search_with_post_filter (lib.rs:3560-3579 / 1797-1813): search k * oversample, then filter, take k
            uint64_t over = top_k * cfg.oversample_factor;
            if (cfg.oversample_factor && over / cfg.oversample_factor != top_k) over = UINT64_MAX;  // saturating_mul
            over = std::max(over, top_k);
            nmn_results cand;
            if (!zero) rs = search_common_mode(e, c, q, dim, over, post_metric, post_op, dl, &cand, shared);
            if (rs == NMN_OK) post_filter(c, filter, cand, top_k, res.get());
        } else if (!zero) {  // search_with_pre_filter (lib.rs:3520-3523 / 1776-1796): cosine in both entries
            rs = pre_filter_search(e, c, q, dim, top_k, filter, op, dl, res.get(), shared);
        }
        if (rs != NMN_OK) return rs;
        if (in_coll && dl.expired()) return err_timeout(op, dl.ms);  // collection entry only: the deadline once more at the end
        *out = res.release();
        return NMN_OK;
    };
    {
        ReadLock rd(e);
        st = run(true);
    }
    if (st == kRetryExclusive) {  // build / patch the mirror and its columns exclusively, then search shared again
        {
            WriteLock g(e);
            Collection* c = e->storage(coll, false);
            if (c) (void)prepare_filtered(e, c, dim);
        }
        ReadLock rd(e);
        st = run(true);
    }
    if (st == kRetryExclusive) {
        WriteLock g(e);
        st = run(false);
    }
    return st;
}

nmn_status nmn_engine_search_similar_filtered(nmn_engine* e, const float* q, uint64_t dim, uint64_t top_k,
                                              const nmn_filter* filter, const nmn_filtered_config* config,
                                              nmn_results** out) {
    if (!e || !out || !filter) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    return filtered_search(e, nullptr, q, dim, top_k, *filter, config, out);
}

nmn_status nmn_engine_compute_similarity(nmn_engine* e, const float* a, uint64_t na, const float* b, uint64_t nb,
                                         float* out) {
    if (!e || !out) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (!a || !b || na == 0 || nb == 0) return err_empty();  // lib.rs:2279-2281
    if (na != nb) return err_dim(na, nb);                    // lib.rs:2282-2287
    if (na > 0xFFFFFFFFull) return fail(NMN_ERR_INVALID_ARGUMENT, "dimension does not fit the device index (> 2^32 - 1)");
    WriteLock g(e);
    auto& slot = e->scratch[na];
    if (!slot) {
        slot = std::make_unique<Mirror>();
        nmn_index_desc d{};
        d.dim = (uint32_t)na;
        d.capacity_rows = 1;
        d.device = e->cfg.device;
        nmn_status st = nmn_index_create(&d, &slot->idx);
        if (st != NMN_OK) {
            e->scratch.erase(na);
            return err_gpu(st);
        }
    }
    nmn_status st = nmn_index_upload(slot->idx, b, 0, 1);
    if (st != NMN_OK) return err_gpu(st);
    const uint64_t row = 0;
    // a_magnitude == 0 -> 0.0 (lib.rs:2289-2292) is what the exact kernel returns for |q| == 0
    st = nmn_index_score_rows(slot->idx, a, 1, NMN_METRIC_COSINE, &row, 1, out);
    return st == NMN_OK ? NMN_OK : err_gpu(st);
}

// ---- collections ---------------------------------------------------------------------------------
nmn_status nmn_engine_create_collection(nmn_engine* e, const char* name, uint64_t dimension, int32_t metric) {
    if (!e || !name) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    WriteLock g(e);
    if (e->configs.count(name)) return fail(NMN_ERR_COLLECTION_EXISTS, std::string("Collection already exists: ") + name);
    CollectionConfig cc;
    cc.dimension = dimension;
    cc.metric = metric;
    e->configs[name] = cc;
    return NMN_OK;
}

nmn_status nmn_engine_delete_collection(nmn_engine* e, const char* name) {
    if (!e || !name) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    WriteLock g(e);
    if (!e->configs.count(name)) return fail(NMN_ERR_COLLECTION_NOT_FOUND, std::string("Collection not found: ") + name);
    e->configs.erase(name);
    e->colls.erase(name);  // "Delete all embeddings in the collection"
    return NMN_OK;
}

int32_t nmn_engine_collection_exists(nmn_engine* e, const char* name) {
    if (!e || !name) return 0;
    WriteLock g(e);
    return e->configs.count(name) ? 1 : 0;
}

uint64_t nmn_engine_collection_count(nmn_engine* e, const char* name) {
    if (!e || !name) return 0;
    WriteLock g(e);
    Collection* c = e->storage(name, false);
    return c ? c->live : 0;
}

nmn_strlist* nmn_engine_list_collections(nmn_engine* e) {
    nmn_strlist* l = new (std::nothrow) nmn_strlist();
    if (!e || !l) return l;
    WriteLock g(e);
    for (const auto& kv : e->configs) l->items.push_back(kv.first);
    return l;
}

nmn_status nmn_engine_store_in_collection(nmn_engine* e, const char* coll, const char* key, const float* v,
                                          uint64_t dim, const nmn_meta_field* meta, uint32_t n_meta) {
    if (!e || !coll || !key) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (!v || dim == 0) return err_empty();  // lib.rs:1454-1456
    WriteLock g(e);
    auto cit = e->configs.find(coll);
    if (cit != e->configs.end() && cit->second.dimension && dim != cit->second.dimension)
        return err_dim(cit->second.dimension, dim);  // lib.rs:1459-1469
    if (e->cfg.max_dimension && dim > e->cfg.max_dimension) return err_dim(e->cfg.max_dimension, dim);
    const nmn_status st = store_into(e, e->storage(coll, true), key, v, dim, meta, n_meta);
    if (st == NMN_OK) e->invalidate_hnsw(coll);  // lib.rs:1497
    return st;
}

nmn_status nmn_engine_get_from_collection(nmn_engine* e, const char* coll, const char* key, float* out,
                                          uint64_t cap, uint64_t* dim_out) {
    if (!e || !coll || !key) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    WriteLock g(e);
    return get_from(e->storage(coll, false), key, std::string(coll) + ":" + key, out, cap, dim_out);
}

nmn_status nmn_engine_delete_from_collection(nmn_engine* e, const char* coll, const char* key) {
    if (!e || !coll || !key) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    WriteLock g(e);
    Collection* c = e->storage(coll, false);
    const std::string shown = std::string(coll) + ":" + key;
    if (!c) return err_not_found(shown);
    const nmn_status st = delete_from(c, key, shown);
    if (st == NMN_OK) e->invalidate_hnsw(coll);  // lib.rs:1532
    return st;
}

nmn_status nmn_engine_search_in_collection(nmn_engine* e, const char* coll, const float* q, uint64_t dim,
                                           uint64_t top_k, nmn_results** out) {
    if (!e || !out || !coll) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    const Deadline dl(e->cfg.search_timeout_ms);
    nmn_status st = validate_query(e, q, dim, top_k, false);  // lib.rs:1593-1598
    if (st != NMN_OK) return st;
    int32_t metric = NMN_METRIC_COSINE;
    {
        ReadLock rd(e);
        auto cit = e->configs.find(coll);
        if (cit != e->configs.end()) {
            if (cit->second.dimension && dim != cit->second.dimension) return err_dim(cit->second.dimension, dim);
            metric = cit->second.metric;  // lib.rs:1614-1616
        }
    }
    std::unique_ptr<nmn_results> res(new_results());
    if (!res) return fail(NMN_ERR_OUT_OF_MEMORY, "results alloc");
    if (!(zero_magnitude(q, dim) && metric == NMN_METRIC_COSINE)) {  // lib.rs:1617-1620
        bool served = false;
        st = cached_hnsw_search(e, coll, "coll:" + std::string(coll) + ":emb:", q, dim, top_k, res.get(), &served);  // lib.rs:1622-1646
        if (st == NMN_OK && !served)
            st = locked_search(e, [&] { return e->storage(coll, false); }, q, dim, top_k, metric, "search_in_collection", dl, res.get());
        if (st != NMN_OK) return st;
    }
    *out = res.release();
    return NMN_OK;
}

nmn_status nmn_engine_search_filtered_in_collection(nmn_engine* e, const char* coll, const float* q, uint64_t dim,
                                                    uint64_t top_k, const nmn_filter* filter,
                                                    const nmn_filtered_config* config, nmn_results** out) {
    if (!e || !out || !coll || !filter) return fail(NMN_ERR_INVALID_ARGUMENT, "null argument");
    return filtered_search(e, coll, q, dim, top_k, *filter, config, out);
}

// ---- measurement aid: per-call latency of search_similar from one host thread (bench.py published_shapes) ----------
nmn_status nmn_engine_search_probe(nmn_engine* e, const float* queries, uint64_t n_queries, uint64_t dim, uint64_t top_k,
                                   uint64_t calls, float* out_us) {
    if (!e || !queries || !out_us || n_queries == 0) return NMN_ERR_INVALID_ARGUMENT;
    for (uint64_t i = 0; i < calls; i++) {
        nmn_results* r = nullptr;
        const auto t0 = std::chrono::steady_clock::now();
        const nmn_status st = nmn_engine_search_similar(e, queries + (i % n_queries) * dim, dim, top_k, &r);
        uint64_t got = nmn_results_len(r);
        volatile float sink = got ? nmn_results_score(r, got - 1) : 0.f;  // (the caller reads its answer)
        (void)sink;
        nmn_results_free(r);
        out_us[i] = std::chrono::duration<float, std::micro>(std::chrono::steady_clock::now() - t0).count();
        if (st != NMN_OK) return st;
    }
    return NMN_OK;
}

// ---- results / lists / filters -------------------------------------------------------------------
uint64_t nmn_results_len(const nmn_results* r) { return r ? r->keys.size() : 0; }
const char* nmn_results_key(const nmn_results* r, uint64_t i) { return (r && i < r->keys.size()) ? r->keys[i].c_str() : nullptr; }
float nmn_results_score(const nmn_results* r, uint64_t i) { return (r && i < r->scores.size()) ? r->scores[i] : NAN; }
const char* nmn_results_aux(const nmn_results* r, uint64_t i) { return (r && i < r->aux.size()) ? r->aux[i].c_str() : nullptr; }
void nmn_results_free(nmn_results* r) { delete r; }
uint64_t nmn_strlist_len(const nmn_strlist* l) { return l ? l->items.size() : 0; }
const char* nmn_strlist_get(const nmn_strlist* l, uint64_t i) { return (l && i < l->items.size()) ? l->items[i].c_str() : nullptr; }
void nmn_strlist_free(nmn_strlist* l) { delete l; }

}  // extern "C"
