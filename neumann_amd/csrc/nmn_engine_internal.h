// nmn_engine_internal.h — what the files of the host-side engine share (nmn_engine.cpp and the nmn_engine_*.cpp beside it): the
// error texts, the store's types, the C-ABI opaque structs, the engine with its lock, and the declarations of what crosses files.
// Internal: never installed.
//
// Linkage: every internal type lives in the named namespace nmn::engine — `struct nmn_engine` has members of these types and is
// seen from several translation units, so they must be the same types in each.  Functions that cross files have external
// linkage in that namespace and are declared here; helpers of one file stay `static` there.
//
// Every file that includes this is built with -ffp-contract=off: the zero-magnitude-query rule and the magnitudes of
// save_index_binary need `simd::magnitude` in reference order on the host (sumsq8_host).
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <new>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/neumann_engine.h"

namespace nmn {
namespace engine {

// The text behind nmn_engine_last_error is ONE thread_local string, private to nmn_engine.cpp: every file fails through these.
nmn_status fail(nmn_status code, std::string msg);
// Display texts of VectorError (lib.rs:151-183)
nmn_status err_not_found(const std::string& key);
nmn_status err_dim(uint64_t expected, uint64_t got);
nmn_status err_empty();
nmn_status err_topk();
nmn_status err_timeout(const char* op, int64_t ms);
nmn_status err_gpu(nmn_status st);  // StorageError(String) with the shim's message (lib.rs:185-189)

// ---- ScalarValue / FilterValue -------------------------------------------------------------------
struct Value {
    int kind = NMN_VAL_NULL;
    bool b = false;
    int64_t i = 0;
    double f = 0.0;
    std::string s;
    static Value from(const nmn_value& v) {
        Value o;
        o.kind = v.kind;
        o.b = v.b != 0;
        o.i = v.i;
        o.f = v.f;
        if (v.kind == NMN_VAL_STRING && v.s) o.s = v.s;
        return o;
    }
};

using Meta = std::map<std::string, Value>;

// simd::sum_of_squares in reference order (hnsw.rs:198-222) — host-side, validation only.
inline float sumsq8_host(const float* v, uint64_t n) {
    const uint64_t chunks = n / 8;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (uint64_t c = 0; c < chunks; c++)
        for (int l = 0; l < 8; l++) {
            const float p = v[8 * c + l] * v[8 * c + l];
            acc[l] = acc[l] + p;
        }
    float r = -0.0f;
    for (int l = 0; l < 8; l++) r = r + acc[l];
    for (uint64_t i = chunks * 8; i < n; i++) {
        const float p = v[i] * v[i];
        r = r + p;
    }
    return r;
}
inline bool zero_magnitude(const float* q, uint64_t n) { return std::sqrt(sumsq8_host(q, n)) == 0.0f; }

struct Entry {
    std::string key;
    std::vector<float> vec;
    Meta meta;
    bool live = false;
    int64_t mrow = -1;  // row of this entry in the GPU mirror of its dimension (-1: not mirrored yet)
};

// GPU mirror of the rows of one collection that have one dimension: the `hnsw_cache` slot of the
// reference (lib.rs:98,1311-1328) with a flat GPU index instead of an HNSW graph.
//
// Maintenance: the reference drops its cache on every store/delete
// (lib.rs:1497,1532,1866,1923) because an HNSW graph cannot be patched cheaply; a flat matrix can.
// New keys are APPENDED into spare capacity (one 3 KB H2D copy + one norm), overwrites rewrite their
// row in place, deletes clear the row's bit in a `live` bitmap that every search passes as (part of)
// the predicate mask.  The mirror is rebuilt only when the spare capacity is exhausted or more than a
// quarter of its rows are dead.  Searches always see exactly the store's current contents.
//
// Metadata: on the first pre-filtered search the metadata fields of the mirrored rows
// are laid out as typed columns in HBM (`cols`, one (kind, payload) cell per row and field; strings
// dictionary-encoded per field) and kept current by the same append / overwrite / tombstone hooks, so
// the predicate of every later filtered search is one kernel over the columns instead of a
// `store.get` + `evaluate_filter` per key (lib.rs:3526-3530).
struct FieldColumn {
    uint32_t id = 0;                                  // column id inside `cols`
    std::unordered_map<std::string, uint32_t> dict;   // string value -> dictionary id
    std::vector<std::string> strings;                 // dictionary id -> string value
};

struct Mirror {
    nmn_index* idx = nullptr;    // one GPU (nmn_engine_config.n_devices <= 1)
    nmn_sharded* sh = nullptr;   // several: the rows split into equal ranges over config.devices[] (include/neumann_gpu.h)
    bool has_rows() const { return idx || sh; }
    uint64_t rows() const { return idx ? nmn_index_rows(idx) : sh ? nmn_sharded_rows(sh) : 0; }
    nmn_status upload(const float* rows_host, uint64_t row0, uint64_t n) {
        return idx ? nmn_index_upload(idx, rows_host, row0, n) : nmn_sharded_upload(sh, rows_host, row0, n);
    }
    std::vector<uint32_t> row_to_slot;
    std::vector<uint64_t> live;  // bit r of word r/64: row r takes part
    uint64_t cap = 0, n_dead = 0;
    int32_t device = -1;
    // Rows whose vector changed on the host since the last upload (stores of existing keys, appended keys).  A store
    // only records the row; the next search of this mirror uploads all of them in runs of consecutive rows (one store =
    // one H2D + two kernels + two stream waits, ~25 us: 45k stores/s against 350k without a mirror).  Rows beyond
    // nmn_index_rows() are always dirty (appends are contiguous).
    std::vector<uint64_t> dirty;
    nmn_columns* cols = nullptr;  // null until a filtered search needs it (or after a device error)
    std::unordered_map<std::string, FieldColumn> fields;
    void drop_columns() {
        if (cols) nmn_columns_destroy(cols);
        cols = nullptr;
        fields.clear();
    }
    ~Mirror() {
        drop_columns();
        if (idx) nmn_index_destroy(idx);
        if (sh) nmn_sharded_destroy(sh);
    }
};

struct Collection {
    std::vector<Entry> slots;
    std::unordered_map<std::string, uint32_t> by_key;
    std::vector<uint32_t> free_slots;
    uint64_t live = 0;
    uint64_t writes = 0;  // stores, deletes and clears so far: an HNSW handle built at the same count still holds the current vectors
    std::unordered_map<uint64_t, std::unique_ptr<Mirror>> mirrors;  // by dimension
    bool has_dirty = false;                                          // some mirror here has stores pending
    void invalidate() { mirrors.clear(); }  // full drop (delete_collection / clear)
};

struct CollectionConfig {  // VectorCollectionConfig (lib.rs:455-475)
    uint64_t dimension = 0;  // 0 = None
    int32_t metric = NMN_METRIC_COSINE;
    bool auto_index = false;               // HNSW auto-indexing: carried through index files, not acted on (the reference only stores the field; the hnsw_cache hook itself is served)
    uint64_t auto_index_threshold = 1000;
};

struct Deadline {  // lib.rs:216-249
    bool has = false;
    std::chrono::steady_clock::time_point at;
    int64_t ms = 0;
    explicit Deadline(int64_t timeout_ms) {
        if (timeout_ms >= 0) {
            has = true;
            ms = timeout_ms;
            at = std::chrono::steady_clock::now() + std::chrono::milliseconds(timeout_ms);
        }
    }
    bool expired() const { return has && std::chrono::steady_clock::now() >= at; }
};

}  // namespace engine
}  // namespace nmn

// FilterCondition (lib.rs:296-324)
struct nmn_filter {
    enum Kind { Cmp, And, Or, True, Exists, Contains, StartsWith, In } kind = True;
    int op = NMN_OP_EQ;
    std::string field, text;
    nmn::engine::Value value;
    std::vector<nmn::engine::Value> values;
    std::unique_ptr<nmn_filter> a, b;
};

struct nmn_results {
    std::vector<std::string> keys;
    std::vector<float> scores;
    std::vector<std::string> aux;  // SimilarArtifact::filename for the artifact searches, otherwise empty
};
struct nmn_strlist {
    std::vector<std::string> items;
};
struct nmn_metalist {  // HashMap<String, TensorValue> of get_metadata (lib.rs:3312-3327)
    std::vector<std::string> names;
    std::vector<nmn::engine::Value> values;
};
// (IVFIndex, Vec<String>) as build_ivf_index returns it (lib.rs:2641-2694): the GPU index + id -> key mapping
struct nmn_engine_ivf {
    nmn_ivf* index = nullptr;           // null = untrained (built from an empty store)
    std::vector<std::string> keys;      // key_mapping: id -> key
    std::vector<float> centroids;
    uint32_t n_clusters = 0;
    uint64_t dim = 0, nprobe = 0;
    ~nmn_engine_ivf() {
        if (index) nmn_ivf_destroy(index);
    }
};

// (HNSWIndex, Vec<String>) as build_hnsw_index returns it (lib.rs:2378-2470): the GPU index + node id -> key mapping
struct nmn_engine_hnsw {
    nmn_hnsw* index = nullptr;          // null = built from an empty store
    std::vector<std::string> keys;
    uint64_t dim = 0;
    uint64_t writes_at_build = 0;       // Collection::writes of the default collection when the rows were read
    // `Arc<HNSWIndex>`: the handle's reference to `index`; the engine's hnsw_cache takes references of its own, so the index lives
    // until the handle is freed AND no cache entry or cached search holds it any more
    std::shared_ptr<nmn_hnsw> owner;
    void own() {
        if (index && !owner) owner.reset(index, [](nmn_hnsw* p) { nmn_hnsw_destroy(p); });
    }
    ~nmn_engine_hnsw() {
        if (index && !owner) nmn_hnsw_destroy(index);
    }
};

struct nmn_engine {
    using Collection = nmn::engine::Collection;
    nmn_engine_config cfg;
    // `&self` from many threads is safe.  Searches whose GPU mirror already exists run under the SHARED lock (the shim
    // merges them into query batches); everything that writes the store or builds a mirror / its columns takes the
    // exclusive lock.  The lock is phase-fair: a waiting writer stops NEW readers (glibc's rwlock prefers readers: a
    // steady stream of searches would starve every store), and when it is done the readers that waited go first, all
    // together (plain writer preference starved the searches under a steady stream of stores: measured 3 q/s).  One
    // mutex + two condition variables: a spin-and-yield ticket turnstile in front of a shared_mutex made 128 waiting
    // searches steal the CPU from the store they waited for (14 ms per store), and a hand-over queue serialised the
    // readers' entry (64 wake-ups in a chain per cohort).
    struct PhaseFairLock {
        std::mutex m;
        std::condition_variable readers_cv, writers_cv;
        int active_readers = 0, waiting_readers = 0, waiting_writers = 0;
        bool writer_active = false, readers_turn = false;
        void read_lock() {
            std::unique_lock<std::mutex> lk(m);
            if (writer_active || (waiting_writers > 0 && !readers_turn)) {
                waiting_readers++;
                readers_cv.wait(lk, [&] { return !writer_active && (waiting_writers == 0 || readers_turn); });
                if (--waiting_readers == 0) readers_turn = false;  // the cohort is in: the next writer's turn
            }
            active_readers++;
            reader_entries++;
        }
        void read_unlock() {
            std::lock_guard<std::mutex> g(m);
            if (--active_readers == 0 && waiting_writers > 0) writers_cv.notify_one();
        }
        void write_lock() {
            std::unique_lock<std::mutex> lk(m);
            waiting_writers++;
            writers_cv.wait(lk, [&] { return !writer_active && active_readers == 0 && !(readers_turn && waiting_readers > 0); });
            waiting_writers--;
            writer_active = true;
        }
        uint64_t reader_entries = 0;  // searches that entered so far
        // searches are waiting right now, or some ran since the caller last looked (*seen is updated)
        bool readers_around(uint64_t* seen) {
            std::lock_guard<std::mutex> g(m);
            const bool around = waiting_readers > 0 || reader_entries != *seen;
            *seen = reader_entries;
            return around;
        }
        void write_unlock() {
            std::lock_guard<std::mutex> g(m);
            writer_active = false;
            if (waiting_readers > 0) {
                readers_turn = true;
                readers_cv.notify_all();
            } else if (waiting_writers > 0) {
                writers_cv.notify_one();
            }
        }
    } rw;
    // A writer that finds searches waiting for the lock — or that searches ran since the previous write — uploads the
    // pending stores (Mirror::dirty, Collection::has_dirty) before it leaves: it already holds the exclusive lock the
    // upload needs.  With no search around they stay pending and a burst of stores becomes one upload.
    uint64_t reader_entries_seen = 0;
    Collection dflt;
    Collection entities;                              // unified entity mode: keys whose TensorData has `_embedding`
    Collection artifacts;                             // tensor_blob: `_blob:meta:{id}` records that carry `_embedding`
    std::map<std::string, Collection> colls;          // storage of named collections
    std::map<std::string, nmn::engine::CollectionConfig> configs;  // `collections` map (configured ones only)
    uint64_t mirror_builds = 0;
    uint64_t column_builds = 0;    // metadata column sets built from the store
    std::atomic<uint64_t> device_filters{0};   // predicates evaluated by the GPU kernel (bumped under the shared lock too)
    std::unordered_map<uint64_t, std::unique_ptr<nmn::engine::Mirror>> scratch;  // compute_similarity, by dim
    // `hnsw_cache: RwLock<HashMap<String, (Arc<HNSWIndex>, Vec<String>)>>` (lib.rs:1305-1334).  An entry is immutable and shared: a
    // search copies the pointer under cache_mu and walks without it, so an index in use outlives its invalidation.
    struct HnswCacheEntry {
        std::shared_ptr<nmn_hnsw> index;  // null: an empty index (built from an empty store)
        uint64_t dim = 0;
        std::vector<std::string> keys;    // the mapping: node id -> key, plain or storage key
    };
    std::mutex cache_mu;
    std::map<std::string, std::shared_ptr<const HnswCacheEntry>> hnsw_cache;
    void invalidate_hnsw(const std::string& collection) {  // lib.rs:1321-1323
        std::lock_guard<std::mutex> g(cache_mu);
        hnsw_cache.erase(collection);
    }

    Collection* storage(const char* coll, bool create) {
        if (!coll) return &dflt;
        auto it = colls.find(coll);
        if (it != colls.end()) return &it->second;
        if (!create) return nullptr;
        return &colls[coll];
    }
};

namespace nmn {
namespace engine {

// exclusive / shared lock of the engine (nmn_engine::PhaseFairLock)
void flush_dirty_mirrors(nmn_engine* e);
struct WriteLock {
    nmn_engine* e;
    explicit WriteLock(nmn_engine* e_) : e(e_) { e->rw.write_lock(); }
    ~WriteLock() {
        if (e->rw.readers_around(&e->reader_entries_seen)) flush_dirty_mirrors(e);
        e->rw.write_unlock();
    }
    WriteLock(const WriteLock&) = delete;
    WriteLock& operator=(const WriteLock&) = delete;
};
struct ReadLock {
    nmn_engine* e;
    explicit ReadLock(nmn_engine* e_) : e(e_) { e->rw.read_lock(); }
    ~ReadLock() { e->rw.read_unlock(); }
    ReadLock(const ReadLock&) = delete;
    ReadLock& operator=(const ReadLock&) = delete;
};

// gpu_topk runs the GPU search over a mirror and maps rows back to keys.
// `selected` (optional): a device bitmap of the rows that take part and how many bits it has set — the
// output of the predicate kernel, already ANDed with the live bitmap.
struct DeviceSelection {
    const uint64_t* mask_dev;
    uint64_t count;
};
// the same as a HOST bitmap over the mirror's rows (a subset of the live rows), e.g. the first max_keys_per_scan keys
struct HostSelection {
    const uint64_t* mask;
    uint64_t count;
};

// ---- FilterCondition -> predicate program (include/neumann_gpu.h, NMN_PRED_*) ------------------------
struct Program {
    std::vector<nmn_pred_op> ops;
    std::vector<uint64_t> consts;
};
struct Code {
    std::vector<nmn_pred_op> ops;
    uint32_t need = 1;  // stack slots the fragment uses
};

// A filtered search first runs under the SHARED lock (so that many of them overlap: each predicate evaluation gets a
// bitmap of its own, and the searches that consume them share corpus sweeps); anything that would have to change the
// engine — building the mirror or its metadata columns — makes it return this and run again under the exclusive lock.
constexpr nmn_status kRetryExclusive = 0x7e7e;

// ---- nmn_engine_filter.cpp ----
bool evaluate_filter(const Meta& meta, const nmn_filter& f);
Code compile_filter(const nmn_filter& f, const Mirror& m, Program& p);
int choose_strategy(const Collection* c, const nmn_filter& f, const nmn_filtered_config& cfg);
void post_filter(const Collection* c, const nmn_filter& f, const nmn_results& cand, uint64_t top_k, nmn_results* res);

// ---- nmn_engine_mirror.cpp ----
Mirror* mirror_of(Collection* c, uint64_t dim);
void columns_write_row(Mirror* m, uint64_t row, const Meta& meta, bool overwrite);
nmn_status store_into(nmn_engine* e, Collection* c, const char* key, const float* v, uint64_t dim, const nmn_meta_field* meta,
                      uint32_t n_meta);
nmn_status delete_from(Collection* c, const std::string& key, const std::string& shown);
nmn_status get_mirror(nmn_engine* e, Collection* c, uint64_t dim, Mirror** out);
nmn_status gpu_topk(Collection* c, Mirror* m, const float* q, uint64_t top_k, int32_t metric, const DeviceSelection* selected,
                    nmn_results* res, const HostSelection* host_sel = nullptr);
nmn_status search_common(nmn_engine* e, Collection* c, const float* q, uint64_t dim, uint64_t top_k, int32_t metric,
                         const char* op, const Deadline& dl, const DeviceSelection* selected, Mirror* prebuilt, nmn_results* res);
nmn_status search_common_mode(nmn_engine* e, Collection* c, const float* q, uint64_t dim, uint64_t top_k, int32_t metric,
                              const char* op, const Deadline& dl, nmn_results* res, bool shared);
nmn_status pre_filter_search(nmn_engine* e, Collection* c, const float* q, uint64_t dim, uint64_t top_k, const nmn_filter& f,
                             const char* op, const Deadline& dl, nmn_results* res, bool shared);
nmn_status prepare_filtered(nmn_engine* e, Collection* c, uint64_t dim);

// The lock ladder of the unfiltered searches: `body(collection, mirror)` under the shared lock when the mirror of (collection, dim)
// exists and has nothing pending, else after the exclusive lock has built / patched it.  `resolve` returns the collection (or
// null: nothing stored there) and runs under the lock.  The body checks its own deadline.
template <typename Resolve, typename Body>
nmn_status on_mirror(nmn_engine* e, Resolve resolve, uint64_t dim, Body body) {
    for (int attempt = 0; attempt < 2; attempt++) {
        {
            ReadLock rd(e);
            Collection* c = resolve();
            if (!c) return NMN_OK;
            auto it = c->mirrors.find(dim);
            if (it != c->mirrors.end() && it->second->dirty.empty()) return body(c, it->second.get());
        }
        // the mirror is missing or has stores pending: build / patch it under the exclusive lock, then search under
        // the shared one like everybody else (a search under the exclusive lock cannot share a sweep with anybody)
        WriteLock wr(e);
        Collection* c = resolve();
        if (!c) return NMN_OK;
        Mirror* m = nullptr;
        nmn_status st = get_mirror(e, c, dim, &m);
        if (st != NMN_OK) return st;
    }
    WriteLock wr(e);  // stores keep arriving between our two locks: serve this one exclusively
    Collection* c = resolve();
    if (!c) return NMN_OK;
    Mirror* m = nullptr;
    nmn_status st = get_mirror(e, c, dim, &m);
    if (st != NMN_OK) return st;
    return body(c, m);
}

// search_common on that ladder
template <typename Resolve>
nmn_status locked_search(nmn_engine* e, Resolve resolve, const float* q, uint64_t dim, uint64_t top_k, int32_t metric,
                         const char* op, const Deadline& dl, nmn_results* res) {
    return on_mirror(e, resolve, dim, [&](Collection* c, Mirror* m) {
        return search_common(e, c, q, dim, top_k, metric, op, dl, nullptr, m, res);
    });
}

inline nmn_status validate_query(const nmn_engine* e, const float* q, uint64_t dim, uint64_t top_k, bool check_max_dim) {
    if (!q || dim == 0) return err_empty();          // query.is_empty() first (lib.rs:1953)
    if (top_k == 0) return err_topk();               // then top_k (lib.rs:1956)
    if (check_max_dim && e->cfg.max_dimension && dim > e->cfg.max_dimension)
        return err_dim(e->cfg.max_dimension, dim);   // lib.rs:1960-1967
    return NMN_OK;
}

inline nmn_results* new_results() { return new (std::nothrow) nmn_results(); }

}  // namespace engine
}  // namespace nmn
