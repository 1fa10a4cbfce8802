// nmn_engine_mirror.cpp — the GPU mirror of a collection's rows and its metadata columns: built lazily, kept current by the two
// writers of the store (store_into / delete_from), flushed before a search; and the searches that run over it (gpu_topk,
// search_common, pre_filter_search).  ALL scoring happens on the GPU through include/neumann_gpu.h.
#include <hip/hip_runtime_api.h>  // hipMemcpy of a selection bitmap (no kernels in this file)

#include "nmn_engine_internal.h"

namespace nmn {
namespace engine {

Mirror* mirror_of(Collection* c, uint64_t dim) {
    auto it = c->mirrors.find(dim);
    if (it == c->mirrors.end()) return nullptr;
    if (!it->second->has_rows()) {  // built when no row of this dimension existed: nothing to patch, rebuild lazily
        c->mirrors.erase(it);
        return nullptr;
    }
    return it->second.get();
}

// ---- metadata columns of a mirror -------------------------------------------------------------------
// ScalarValue -> (kind, payload) cell; strings get (or take) an id in the field's dictionary
static void encode_cell(FieldColumn& fc, const Value& v, uint8_t* kind, uint64_t* payload) {
    *payload = 0;
    switch (v.kind) {
        case NMN_VAL_BOOL: *kind = NMN_CELL_BOOL; *payload = v.b ? 1 : 0; break;
        case NMN_VAL_INT: *kind = NMN_CELL_INT; memcpy(payload, &v.i, 8); break;
        case NMN_VAL_FLOAT: *kind = NMN_CELL_FLOAT; memcpy(payload, &v.f, 8); break;
        case NMN_VAL_STRING: {
            *kind = NMN_CELL_STRING;
            auto it = fc.dict.find(v.s);
            if (it == fc.dict.end()) {
                it = fc.dict.emplace(v.s, (uint32_t)fc.strings.size()).first;
                fc.strings.push_back(v.s);
            }
            *payload = it->second;
            break;
        }
        default: *kind = NMN_CELL_NULL; break;
    }
}

// keep the device copy of one word of the live bitmap current (no-op without columns)
static void columns_sync_valid(Mirror* m, uint64_t word) {
    if (!m->cols) return;
    if (nmn_columns_write_valid(m->cols, word, 1, &m->live[word]) != NMN_OK) m->drop_columns();
}

// write the metadata cells of one (new or overwritten) row; `overwrite` first drops the old cells
void columns_write_row(Mirror* m, uint64_t row, const Meta& meta, bool overwrite) {
    if (!m->cols) return;
    if (overwrite && nmn_columns_clear_row(m->cols, row) != NMN_OK) return m->drop_columns();
    for (const auto& kv : meta) {
        auto it = m->fields.find(kv.first);
        if (it == m->fields.end()) {
            FieldColumn fc;
            if (nmn_columns_add(m->cols, &fc.id) != NMN_OK) return m->drop_columns();
            it = m->fields.emplace(kv.first, std::move(fc)).first;
        }
        uint8_t kind;
        uint64_t payload;
        encode_cell(it->second, kv.second, &kind, &payload);
        if (nmn_columns_write(m->cols, it->second.id, row, 1, &kind, &payload) != NMN_OK) return m->drop_columns();
    }
}

// build the column set of a mirror from the store (first filtered search, or after drop_columns)
static nmn_status columns_build(nmn_engine* e, Collection* c, Mirror* m) {
    if (m->cols) return NMN_OK;
    nmn_status st = nmn_columns_create(m->device, m->cap, &m->cols);
    if (st != NMN_OK) return err_gpu(st);
    const uint64_t n = m->row_to_slot.size();
    struct Staging {
        std::vector<uint8_t> kinds;
        std::vector<uint64_t> payload;
    };
    std::unordered_map<std::string, Staging> staging;
    for (uint64_t r = 0; r < n; r++) {
        if (!((m->live[r >> 6] >> (r & 63)) & 1ull)) continue;  // a dead row's slot may belong to another key now
        for (const auto& kv : c->slots[m->row_to_slot[r]].meta) {
            Staging& sg = staging[kv.first];
            if (sg.kinds.empty()) {
                sg.kinds.assign(n, NMN_CELL_ABSENT);
                sg.payload.assign(n, 0ull);
            }
            encode_cell(m->fields[kv.first], kv.second, &sg.kinds[r], &sg.payload[r]);
        }
    }
    for (auto& kv : staging) {
        FieldColumn& fc = m->fields[kv.first];
        st = nmn_columns_add(m->cols, &fc.id);
        if (st == NMN_OK) st = nmn_columns_write(m->cols, fc.id, 0, n, kv.second.kinds.data(), kv.second.payload.data());
        if (st != NMN_OK) {
            m->drop_columns();
            return err_gpu(st);
        }
    }
    st = nmn_columns_write_valid(m->cols, 0, m->live.size(), m->live.data());
    if (st != NMN_OK) {
        m->drop_columns();
        return err_gpu(st);
    }
    e->column_builds++;
    return NMN_OK;
}

// mark a mirrored row dead; rebuild later once a quarter of the mirror is dead
static void mirror_tombstone(Collection* c, uint64_t dim, int64_t row) {
    Mirror* m = mirror_of(c, dim);
    if (!m || row < 0) return;
    m->live[(uint64_t)row >> 6] &= ~(1ull << ((uint64_t)row & 63));
    m->n_dead++;
    if (m->n_dead * 4 > m->row_to_slot.size()) c->mirrors.erase(dim);
    else columns_sync_valid(m, (uint64_t)row >> 6);
}

static void mark_dirty(Collection* c, Mirror* m, uint64_t dim, uint64_t row) {
    (void)dim;
    m->dirty.push_back(row);
    c->has_dirty = true;
}

// append one vector to the mirror of its dimension; returns its row, or -1 (mirror absent / dropped)
static int64_t mirror_append(Collection* c, uint64_t dim, const float* v, uint32_t slot, const Meta& meta) {
    Mirror* m = mirror_of(c, dim);
    if (!m) return -1;
    const uint64_t row = m->row_to_slot.size();
    (void)v;  // uploaded by mirror_flush from the slot's host copy
    if (row >= m->cap) {
        c->mirrors.erase(dim);  // out of spare capacity: rebuild on the next search
        return -1;
    }
    mark_dirty(c, m, dim, row);
    m->row_to_slot.push_back(slot);
    if ((row >> 6) >= m->live.size()) m->live.push_back(0ull);
    m->live[row >> 6] |= 1ull << (row & 63);
    columns_write_row(m, row, meta, false);  // a fresh row's cells are still ABSENT
    columns_sync_valid(m, row >> 6);
    return (int64_t)row;
}

nmn_status store_into(nmn_engine* e, Collection* c, const char* key, const float* v, uint64_t dim,
                      const nmn_meta_field* meta, uint32_t n_meta) {
    Entry ent;
    ent.key = key;
    ent.vec.assign(v, v + dim);
    c->writes++;
    for (uint32_t i = 0; i < n_meta; i++)
        if (meta[i].name) ent.meta[meta[i].name] = Value::from(meta[i].value);
    ent.live = true;
    auto it = c->by_key.find(ent.key);
    if (it != c->by_key.end()) {
        // put() overwrites the whole TensorData (vector and metadata)
        Entry& old = c->slots[it->second];
        const uint64_t old_dim = old.vec.size();
        Mirror* m = old.mrow >= 0 ? mirror_of(c, old_dim) : nullptr;
        if (m && old_dim == dim) {
            mark_dirty(c, m, dim, (uint64_t)old.mrow);
            ent.mrow = old.mrow;
            columns_write_row(m, (uint64_t)old.mrow, ent.meta, true);
        } else {
            if (m) mirror_tombstone(c, old_dim, old.mrow);
            ent.mrow = mirror_append(c, dim, v, it->second, ent.meta);
        }
        old = std::move(ent);
    } else {
        uint32_t slot;
        if (!c->free_slots.empty()) {
            slot = c->free_slots.back();
            c->free_slots.pop_back();
        } else {
            slot = (uint32_t)c->slots.size();
            c->slots.emplace_back();
        }
        ent.mrow = mirror_append(c, dim, v, slot, ent.meta);
        c->slots[slot] = std::move(ent);
        c->by_key[c->slots[slot].key] = slot;
        c->live++;
    }
    (void)e;
    return NMN_OK;
}

nmn_status delete_from(Collection* c, const std::string& key, const std::string& shown) {
    auto it = c->by_key.find(key);
    if (it == c->by_key.end()) return err_not_found(shown);
    c->writes++;
    Entry& ent = c->slots[it->second];
    mirror_tombstone(c, ent.vec.size(), ent.mrow);
    ent = Entry();
    c->free_slots.push_back(it->second);
    c->by_key.erase(it);
    c->live--;
    return NMN_OK;
}

// Upload the vectors recorded in m->dirty (exclusive lock held): runs of consecutive rows, one nmn_index_upload each.
// A row that died meanwhile still gets a vector (appends must stay contiguous; the live bitmap keeps it out of every
// scan).  On a device error the mirror is dropped and rebuilt by the caller's get_mirror.
static bool mirror_flush(Collection* c, Mirror* m, uint64_t dim) {
    if (m->dirty.empty() || !m->has_rows()) {
        m->dirty.clear();
        return true;
    }
    std::sort(m->dirty.begin(), m->dirty.end());
    m->dirty.erase(std::unique(m->dirty.begin(), m->dirty.end()), m->dirty.end());
    std::vector<float> buf;
    size_t i = 0;
    while (i < m->dirty.size()) {
        size_t j = i + 1;
        while (j < m->dirty.size() && m->dirty[j] == m->dirty[j - 1] + 1 && j - i < 65536) j++;
        buf.assign((j - i) * dim, 0.0f);
        for (size_t r = i; r < j; r++) {
            const uint64_t row = m->dirty[r];
            if (row >= m->row_to_slot.size()) continue;
            const Entry& ent = c->slots[m->row_to_slot[row]];
            if (ent.live && ent.mrow == (int64_t)row && ent.vec.size() == dim)
                memcpy(buf.data() + (r - i) * dim, ent.vec.data(), dim * sizeof(float));
        }
        if (m->upload(buf.data(), m->dirty[i], j - i) != NMN_OK) return false;
        i = j;
    }
    m->dirty.clear();
    return true;
}

static void flush_collection(Collection* c) {
    if (!c->has_dirty) return;
    c->has_dirty = false;
    for (auto it = c->mirrors.begin(); it != c->mirrors.end();) {
        if (!it->second->dirty.empty() && !mirror_flush(c, it->second.get(), it->first)) it = c->mirrors.erase(it);
        else ++it;
    }
}
void flush_dirty_mirrors(nmn_engine* e) {  // exclusive lock held
    flush_collection(&e->dflt);
    flush_collection(&e->entities);
    flush_collection(&e->artifacts);
    for (auto& kv : e->colls) flush_collection(&kv.second);
}

// Lazily (re)build the GPU mirror of the rows of `c` with dimension `dim`.
nmn_status get_mirror(nmn_engine* e, Collection* c, uint64_t dim, Mirror** out) {
    auto it = c->mirrors.find(dim);
    if (it != c->mirrors.end()) {
        if (mirror_flush(c, it->second.get(), dim)) {
            *out = it->second.get();
            return NMN_OK;
        }
        c->mirrors.erase(it);  // device error while patching: rebuild from the store
    }
    auto m = std::make_unique<Mirror>();
    m->device = e->cfg.device;
    uint64_t n = 0;
    for (const auto& ent : c->slots)
        if (ent.live && ent.vec.size() == dim) n++;  // `if stored_vec.len() != query.len() { return None }`
    if (n > 0) {
        // (an FFI caller's u64 dimension must not be truncated into a smaller, valid one; nmn_index_create's own limit is
        // one query in LDS: 40960 floats)
        if (dim > 0xFFFFFFFFull) return fail(NMN_ERR_INVALID_ARGUMENT, "dimension does not fit the device index (> 2^32 - 1)");
        nmn_index_desc d{};
        d.dim = (uint32_t)dim;
        // an engine serves concurrent search_similar callers, which share sweeps: rows of 300 / 200 / 100 floats are
        // stored with a stride of 384 / 256 / 128 so those batches take the matrix-core sweep (10M x 300, 64 queries:
        // 2.3 k -> 39.4 k q/s; one query alone 800 -> 718 q/s).  NMN_ENGINE_TIGHT_ROWS=1 keeps the stride at dim.
        static const bool tight_rows = getenv("NMN_ENGINE_TIGHT_ROWS") != nullptr;
        d.flags = tight_rows ? 0u : NMN_INDEX_WIDE_ROWS;
        m->cap = n + std::max<uint64_t>(n / 2, 1024);  // spare rows for appended keys
        d.capacity_rows = m->cap;
        d.row_base = 0;
        d.device = e->cfg.device;
        d.cand_cap = e->cfg.cand_cap;
        nmn_status st;
        if (e->cfg.n_devices >= 2) {
            // one logical index over the configured GPUs: the rows dealt evenly over them, every search on all of them at once,
            // per-shard top-k gathered (RCCL over xGMI / peer copies) and merged on devices[0] (nmn_sharded.hip).  The
            // metadata columns of the collection stay on devices[0]; a predicate's bitmap is sliced per shard by the search.
            nmn_sharded_desc sd{};
            sd.dim = d.dim;
            sd.flags = d.flags;
            sd.capacity_rows = m->cap;
            sd.row_base = 0;
            sd.n_shards = e->cfg.n_devices;
            sd.gather = NMN_GATHER_AUTO;
            sd.devices = e->cfg.devices;
            sd.cand_cap = e->cfg.cand_cap;
            // 64-row blocks dealt round-robin: the rows HELD (n of the n + 50 % capacity) and every later append are spread
            // evenly over the GPUs; contiguous ranges of the capacity would fill GPU 0, then GPU 1, ... and leave the last idle
            sd.layout = NMN_SHARDED_LAYOUT_CYCLIC;
            m->device = e->cfg.devices[0];
            st = nmn_sharded_create(&sd, &m->sh);
        } else {
            st = nmn_index_create(&d, &m->idx);
        }
        if (st != NMN_OK) return err_gpu(st);
        m->row_to_slot.reserve(n);
        // stage in chunks so the host copy stays small next to the store itself
        const uint64_t chunk = std::max<uint64_t>(1, (64ull << 20) / (dim * sizeof(float)));
        std::vector<float> buf;
        buf.reserve((size_t)std::min(chunk, n) * dim);
        uint64_t row0 = 0;
        auto flush = [&]() -> nmn_status {
            if (buf.empty()) return NMN_OK;
            const uint64_t cnt = buf.size() / dim;
            nmn_status s2 = m->upload(buf.data(), row0, cnt);
            row0 += cnt;
            buf.clear();
            return s2;
        };
        for (uint32_t s = 0; s < c->slots.size(); s++) {
            Entry& ent = c->slots[s];
            if (!ent.live || ent.vec.size() != dim) continue;
            buf.insert(buf.end(), ent.vec.begin(), ent.vec.end());
            ent.mrow = (int64_t)m->row_to_slot.size();
            m->row_to_slot.push_back(s);
            if (buf.size() >= chunk * dim) {
                st = flush();
                if (st != NMN_OK) return err_gpu(st);
            }
        }
        st = flush();
        if (st != NMN_OK) return err_gpu(st);
        m->live.assign((n + 63) / 64, ~0ull);
        if (n & 63) m->live.back() = (1ull << (n & 63)) - 1ull;
    }
    e->mirror_builds++;
    *out = m.get();
    c->mirrors[dim] = std::move(m);
    return NMN_OK;
}

nmn_status gpu_topk(Collection* c, Mirror* m, const float* q, uint64_t top_k, int32_t metric,
                    const DeviceSelection* selected, nmn_results* res, const HostSelection* host_sel) {
    if (!m->has_rows()) return NMN_OK;  // no rows of this dimension
    const uint64_t rows = m->rows();
    const uint64_t taking_part = host_sel ? host_sel->count : selected ? selected->count : rows - std::min<uint64_t>(m->n_dead, rows);
    uint64_t k = std::min<uint64_t>(top_k, taking_part);
    if (k == 0) return NMN_OK;
    std::vector<uint64_t> out_rows(k);
    std::vector<float> out_scores(k);
    uint32_t count = 0;
    nmn_status st;
    if (m->sh) {
        // several GPUs: the bitmap travels as a host bitmap over global rows (the search slices it per shard); a
        // predicate's selection is read back from devices[0] first (rows / 8 bytes)
        std::vector<uint64_t> sel_host;
        const uint64_t* mask = host_sel ? host_sel->mask : m->n_dead ? m->live.data() : nullptr;
        if (selected) {
            sel_host.resize((size_t)((rows + 63) / 64));
            if (hipMemcpy(sel_host.data(), selected->mask_dev, sel_host.size() * 8, hipMemcpyDeviceToHost) != hipSuccess)
                return fail(NMN_ERR_STORAGE, "Storage error: reading the selection bitmap back");
            mask = sel_host.data();
        }
        st = nmn_sharded_search(m->sh, q, 1, (uint32_t)k, (nmn_metric)metric, mask, out_rows.data(), out_scores.data(), &count,
                                nullptr);
    } else if (selected) {
        st = nmn_index_search_dmask_hint(m->idx, q, 1, (uint32_t)k, (nmn_metric)metric, selected->mask_dev, selected->count,
                                         out_rows.data(), out_scores.data(), &count, nullptr);
    } else {
        // deleted rows stay in the matrix until the next rebuild: the live bitmap keeps them out of every scan
        st = nmn_index_search(m->idx, q, 1, (uint32_t)k, (nmn_metric)metric,
                              host_sel ? host_sel->mask : m->n_dead ? m->live.data() : nullptr,
                              out_rows.data(), out_scores.data(), &count, nullptr);
    }
    if (st != NMN_OK) return err_gpu(st);
    for (uint32_t i = 0; i < count; i++) {
        res->keys.push_back(c->slots[m->row_to_slot[out_rows[i]]].key);
        res->scores.push_back(out_scores[i]);
    }
    return NMN_OK;
}

// shared body of search_similar / search_similar_with_metric / search_in_collection
nmn_status search_common(nmn_engine* e, Collection* c, const float* q, uint64_t dim, uint64_t top_k, int32_t metric,
                         const char* op, const Deadline& dl, const DeviceSelection* selected,
                         Mirror* prebuilt, nmn_results* res) {
    Mirror* m = prebuilt;
    if (!m) {
        nmn_status st = get_mirror(e, c, dim, &m);  // "let keys = self.store.scan(prefix)" stage
        if (st != NMN_OK) return st;
    }
    if (dl.expired()) return err_timeout(op, dl.ms);  // lib.rs:2005-2010
    nmn_status st = gpu_topk(c, m, q, top_k, metric, selected, res);
    if (st != NMN_OK) return st;
    if (dl.expired()) return err_timeout(op, dl.ms);  // lib.rs:2019-2024
    return NMN_OK;
}

// Pre-filter strategy (lib.rs:3514-3557 / 1776-1796): the predicate runs on the GPU over the mirror's
// metadata columns and leaves the selection bitmap in HBM; the masked scan reads it in place.  Exact.
nmn_status pre_filter_search(nmn_engine* e, Collection* c, const float* q, uint64_t dim, uint64_t top_k,
                             const nmn_filter& f, const char* op, const Deadline& dl, nmn_results* res, bool shared) {
    Mirror* m = nullptr;
    if (shared) {
        auto it = c->mirrors.find(dim);
        if (it == c->mirrors.end()) return kRetryExclusive;
        m = it->second.get();
        if (!m->dirty.empty() || (m->has_rows() && !m->cols)) return kRetryExclusive;
    } else {
        nmn_status st = get_mirror(e, c, dim, &m);
        if (st != NMN_OK) return st;
    }
    if (!m->has_rows()) return NMN_OK;
    nmn_status st = shared ? NMN_OK : columns_build(e, c, m);
    if (st != NMN_OK) return st;
    Program p;
    Code code = compile_filter(f, *m, p);
    p.ops = std::move(code.ops);
    // predicate and search in one call (nmn_index_search_pred): concurrent filtered searches then wait for ONE batch —
    // their predicates are evaluated together on the batch's stream, right before the sweep that serves them all
    if (dl.expired()) return err_timeout(op, dl.ms);  // lib.rs:2005-2010
    const uint64_t rows = m->rows();
    const uint64_t k = std::min<uint64_t>(std::min<uint64_t>(top_k, rows), NMN_MAX_TOP_K);
    if (k == 0 || rows != m->row_to_slot.size()) {
        if (k == 0) return NMN_OK;
        return fail(NMN_ERR_STORAGE, "mirror and metadata columns disagree on the row count");
    }
    if (top_k > NMN_MAX_TOP_K || m->sh) {
        // beyond the candidate pipeline: evaluate, then the large-k path over the bitmap (the two-step form); also the
        // form of a mirror that spans several GPUs (evaluate on devices[0], search every shard under its slice)
        DeviceSelection sel{nullptr, 0};
        uint32_t slot = 0;
        st = nmn_columns_eval_acquire(m->cols, p.ops.data(), (uint32_t)p.ops.size(), p.consts.data(), p.consts.size(),
                                      m->row_to_slot.size(), &sel.count, &slot, &sel.mask_dev);
        if (st != NMN_OK) return err_gpu(st);
        e->device_filters++;
        st = NMN_OK;
        if (sel.count != 0)  // else `if matching_keys.is_empty() { return Vec::new() }`
            st = search_common(e, c, q, dim, top_k, NMN_METRIC_COSINE, op, dl, &sel, m, res);
        (void)nmn_columns_eval_release(m->cols, slot);
        return st;
    }
    std::vector<uint64_t> out_rows(k);
    std::vector<float> out_scores(k);
    uint32_t count = 0;
    uint64_t selected = 0;
    st = nmn_index_search_pred(m->idx, m->cols, p.ops.data(), (uint32_t)p.ops.size(), p.consts.data(), p.consts.size(), q, 1,
                               (uint32_t)k, NMN_METRIC_COSINE, out_rows.data(), out_scores.data(), &count, &selected, nullptr);
    if (st != NMN_OK) return err_gpu(st);
    e->device_filters++;
    for (uint32_t i = 0; i < count; i++) {
        res->keys.push_back(c->slots[m->row_to_slot[out_rows[i]]].key);
        res->scores.push_back(out_scores[i]);
    }
    if (dl.expired()) return err_timeout(op, dl.ms);  // lib.rs:2019-2024
    return NMN_OK;
}

// what a shared-lock filtered search needs to find in place (exclusive lock held)
nmn_status prepare_filtered(nmn_engine* e, Collection* c, uint64_t dim) {
    Mirror* m = nullptr;
    nmn_status st = get_mirror(e, c, dim, &m);
    if (st != NMN_OK || !m->has_rows()) return st;
    return columns_build(e, c, m);
}

// search_common for the post-filter arm: under the shared lock only when the mirror exists already
nmn_status search_common_mode(nmn_engine* e, Collection* c, const float* q, uint64_t dim, uint64_t top_k, int32_t metric,
                              const char* op, const Deadline& dl, nmn_results* res, bool shared) {
    Mirror* prebuilt = nullptr;
    if (shared) {
        auto it = c->mirrors.find(dim);
        if (it == c->mirrors.end() || !it->second->dirty.empty()) return kRetryExclusive;
        prebuilt = it->second.get();
    }
    return search_common(e, c, q, dim, top_k, metric, op, dl, nullptr, prebuilt, res);
}

}  // namespace engine
}  // namespace nmn

using namespace nmn::engine;

extern "C" {

uint64_t nmn_engine_device_filter_evals(nmn_engine* e) {
    if (!e) return 0;
    WriteLock g(e);
    return e->device_filters;
}

uint64_t nmn_engine_column_builds(nmn_engine* e) {
    if (!e) return 0;
    WriteLock g(e);
    return e->column_builds;
}

uint64_t nmn_engine_mirror_builds(nmn_engine* e) {
    if (!e) return 0;
    WriteLock g(e);
    return e->mirror_builds;
}

// rows the mirror of (default collection, dim) holds on each of its GPUs: out[0 .. min(cap, shards)); returns the number of
// shards (1 for a single-GPU mirror, 0 when no mirror of that dimension exists)
uint32_t nmn_engine_mirror_shard_rows(nmn_engine* e, uint64_t dim, uint64_t* out, uint32_t cap) {
    if (!e) return 0;
    WriteLock g(e);
    auto it = e->dflt.mirrors.find(dim);
    if (it == e->dflt.mirrors.end() || !it->second->has_rows()) return 0;
    Mirror* m = it->second.get();
    if (!mirror_flush(&e->dflt, m, dim)) {  // (a failed flush leaves a mirror nobody may trust: dropped, as every other caller does)
        e->dflt.mirrors.erase(it);
        return 0;
    }
    if (m->idx) {
        if (out && cap) out[0] = nmn_index_rows(m->idx);
        return 1;
    }
    const uint32_t G = nmn_sharded_shards(m->sh);
    for (uint32_t i = 0; i < G && i < cap && out; i++) out[i] = nmn_index_rows(nmn_sharded_shard(m->sh, i));
    return G;
}

// device memory of the mirror of (default collection, dim), summed over its shards: out[0] = f32 rows, out[1] = the 8-bit / bf16
// mirrors that exist right now, out[2] = per-row factors (nmn_index_hbm_bytes); returns the number of shards (0: no such mirror)
uint32_t nmn_engine_mirror_hbm_bytes(nmn_engine* e, uint64_t dim, uint64_t out[3]) {
    if (!e || !out) return 0;
    // an accounting query: the shared lock, and no flush of pending rows — the sizes depend on the shards' CAPACITY, not on which
    // rows have been copied (it used to take the exclusive lock, flush, and ignore the flush's verdict)
    ReadLock g(e);
    out[0] = out[1] = out[2] = 0;
    auto it = e->dflt.mirrors.find(dim);
    if (it == e->dflt.mirrors.end() || !it->second->has_rows()) return 0;
    Mirror* m = it->second.get();
    const uint32_t G = m->idx ? 1u : nmn_sharded_shards(m->sh);
    for (uint32_t i = 0; i < G; i++) {
        uint64_t a = 0, b = 0, c = 0;
        (void)nmn_index_hbm_bytes(m->idx ? m->idx : nmn_sharded_shard(m->sh, i), &a, &b, &c);
        out[0] += a;
        out[1] += b;
        out[2] += c;
    }
    return G;
}

int32_t nmn_engine_mirror_cached(nmn_engine* e, const char* coll) {
    if (!e) return 0;
    WriteLock g(e);
    Collection* c = e->storage(coll, false);
    return (c && !c->mirrors.empty()) ? 1 : 0;
}

}  // extern "C"
