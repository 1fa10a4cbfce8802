// nmn_hnsw_build.hip — how the HNSW graph grows (docs/hnsw.md): the reference's insert on the host (try_insert_embedding,
// hnsw.rs:1936-2051), the adjacency and the rows as they are sent to HBM, the bulk build whose walks run on the device (§19), and
// the insert entry points.  The walk templates and the distances they call are nmn_hnsw_host.h's.
// THIS TRANSLATION UNIT IS BUILT WITH -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt (build.py), host and device:
// every distance restates the reference's unfused f32 arithmetic and must give its bits (docs/hnsw.md, "Source layout").
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <shared_mutex>
#include <vector>

#include "nmn_hnsw_host.h"

#pragma clang fp contract(off)

using namespace nmn;
using namespace nmn::hnsw;

namespace {

// random_level, hnsw.rs:1631-1651 (usize = 64 bits)
uint32_t next_level(nmn_hnsw* h) {
    uint64_t s = h->rng;
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    h->rng = s;
    const double f = (double)s / (double)UINT64_MAX;
    const double lv = std::floor(-std::log(f) * h->cfg.ml);
    if (!(lv > 0.0)) return 0;
    return lv >= 32.0 ? 32u : (uint32_t)lv;
}

// try_insert_embedding, hnsw.rs:1936-2051 (the row and its magnitude are already in h->rows / h->mags)
// The insert is split into what it searches and what it commits (docs/hnsw.md §19): nmn_hnsw_insert runs the two interleaved per
// layer, as the reference does; nmn_hnsw_insert_bulk may take a layer's `selected` from the device's walk instead of searching.
// `mark(node, layer)` is told every list a commit assigns — the new node's own, and that of every selected neighbour, pruned or not.
struct NoMark {
    void operator()(uint32_t, uint32_t) {}
};

// hnsw.rs:2005-2040: connect the new node to `selected` on `layer`, prune every back link list that outgrew m / m0
template <class Mark>
void host_commit_layer(nmn_hnsw* h, uint32_t node_id, uint32_t layer, const std::vector<uint32_t>& selected,
                       std::vector<std::pair<float, uint32_t>>& wd, Mark& mark) {
    const uint32_t m = layer == 0 ? h->cfg.m0 : h->cfg.m;
    {
        std::vector<uint32_t>& mine = h->nbr[node_id][layer];
        mine.insert(mine.end(), selected.begin(), selected.end());
        std::sort(mine.begin(), mine.end());
        mark(node_id, layer);
    }
    for (uint32_t nb : selected) {
        std::vector<uint32_t>& lst = h->nbr[nb][layer];
        lst.insert(std::upper_bound(lst.begin(), lst.end(), node_id), node_id);  // push + sort: stays id-ascending
        mark(nb, layer);
        if (lst.size() > m) {
            wd.clear();
            for (uint32_t id : lst) wd.emplace_back(pair_of_nodes_distance(h, nb, id), id);
            std::stable_sort(wd.begin(), wd.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
            lst.clear();
            for (size_t i = 0; i < m; i++) lst.push_back(wd[i].second);
            std::sort(lst.begin(), lst.end());
        }
    }
}

// try_insert_embedding after random_level, hnsw.rs:1957-2051 (the row and its magnitude are already in h->rows / h->mags)
template <class Mark>
void host_insert_node_at(nmn_hnsw* h, uint32_t node_id, uint32_t node_level, HostVisited& vis, Mark& mark) {
    h->level.push_back((uint8_t)node_level);
    h->nbr.emplace_back(node_level + 1);
    if (h->entry == ~0ull) {
        h->entry = node_id;
        h->max_layer = node_level;
        return;
    }
    const uint32_t current_max = h->max_layer;
    const float* q = h->rows.data() + (size_t)node_id * h->dim;
    const HQ qmag = host_query(h, q);  // (a quantized node's own query is its to_dense(), hnsw.rs:1985: the row kept here)
    const auto dist = [&](uint32_t node) { return node_distance(h, node, q, qmag); };
    uint64_t evals = 0;
    uint32_t cur = (uint32_t)h->entry;
    for (uint32_t layer = current_max; layer >= node_level + 1; layer--) cur = host_greedy(h, dist, cur, layer, &evals);
    std::vector<Ent> found;
    std::vector<std::pair<float, uint32_t>> wd;
    for (int layer = (int)std::min(node_level, current_max); layer >= 0; layer--) {
        host_search_layer(h, dist, cur, h->cfg.ef_construction, (uint32_t)layer, vis, found, &evals);
        const uint32_t m = layer == 0 ? h->cfg.m0 : h->cfg.m;
        std::vector<uint32_t> selected;
        for (size_t i = 0; i < found.size() && i < m; i++) selected.push_back(found[i].id);
        host_commit_layer(h, node_id, (uint32_t)layer, selected, wd, mark);
        if (!found.empty()) cur = found[0].id;
    }
    if (node_level > current_max) {
        h->entry = node_id;
        h->max_layer = node_level;
    }
}

// try_insert_embedding, hnsw.rs:1936-2051
void host_insert_node(nmn_hnsw* h, uint32_t node_id, HostVisited& vis) {
    const uint32_t node_level = next_level(h);
    NoMark none;
    host_insert_node_at(h, node_id, node_level, vis, none);
}

// The same node with the searches already done by hnsw_insert_walk_kernel: sel / selcnt as the kernel wrote them for this node
// (layer 0's ids first, layer l >= 1 at m0 + (l - 1) m).  The index is not empty.
template <class Mark>
void host_commit_walked(nmn_hnsw* h, uint32_t node_id, uint32_t node_level, const uint32_t* sel, const uint32_t* selcnt,
                        Mark& mark) {
    h->level.push_back((uint8_t)node_level);
    h->nbr.emplace_back(node_level + 1);
    const uint32_t current_max = h->max_layer;
    std::vector<std::pair<float, uint32_t>> wd;
    std::vector<uint32_t> selected;
    for (int layer = (int)std::min(node_level, current_max); layer >= 0; layer--) {
        const uint32_t* ids = sel + (layer == 0 ? 0u : h->cfg.m0 + (uint32_t)(layer - 1) * h->cfg.m);
        selected.assign(ids, ids + selcnt[layer]);
        host_commit_layer(h, node_id, (uint32_t)layer, selected, wd, mark);
    }
    if (node_level > current_max) {
        h->entry = node_id;
        h->max_layer = node_level;
    }
}

}  // namespace

namespace nmn {
namespace hnsw {

nmn_status canonicalise_sparse(uint32_t dim, const uint64_t* indptr, const uint32_t* positions, const float* values, uint32_t nq,
                               SparseQueries* out) {
    for (uint32_t q = 0; q < nq; q++)
        if (indptr[q + 1] < indptr[q]) return set_error(NMN_ERR_INVALID_ARGUMENT, "HNSW: indptr decreases");
    if (indptr[nq] > indptr[0] && (!positions || !values)) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    out->off.assign(1, 0);
    out->off.reserve((size_t)nq + 1);
    out->mag.resize(nq);
    out->dup.assign(nq, 0);
    std::vector<std::pair<uint32_t, float>> pairs;
    for (uint32_t q = 0; q < nq; q++) {
        pairs.clear();
        for (uint64_t i = indptr[q]; i < indptr[q + 1]; i++) {
            if (positions[i] >= dim) {  // SparseVectorError::IndexOutOfBounds, sparse_vector.rs:40-42
                char buf[128];
                snprintf(buf, sizeof buf, "index %u out of bounds for dimension %u", positions[i], dim);
                return set_error(NMN_ERR_INVALID_ARGUMENT, buf);
            }
            if (values[i] != 0.0f) pairs.emplace_back(positions[i], values[i]);
        }
        std::stable_sort(pairs.begin(), pairs.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        for (size_t i = 0; i < pairs.size(); i++) {
            if (i && pairs[i].first == pairs[i - 1].first) out->dup[q] = 1;
            out->pos.push_back(pairs[i].first);
            out->val.push_back(pairs[i].second);
        }
        out->off.push_back(out->pos.size());
        out->mag[q] = h_sparse_mag(out->val.data() + out->off[q], out->nnz(q));
    }
    return NMN_OK;
}

nmn_status wait_in_flight(nmn_hnsw* h) {  // caller holds rw exclusively
    std::lock_guard<std::mutex> lk(h->dev_mu);
    for (hipEvent_t e : h->ev_pending) {
        HN_TRY(hipEventSynchronize(e));
        h->ev_free.push_back(e);
    }
    h->ev_pending.clear();
    return NMN_OK;
}

// the adjacency as it sits in HBM: layer 0 [n][m0] + counts, upper layers [n_upper][up_layers][m] + counts + a row per node
// reserve_n / reserve_upper / layers (nmn_hnsw_insert_bulk, docs/hnsw.md §19): the arrays sized and laid out for a graph of that
// many nodes, upper nodes and upper layers — the slots past the present graph empty — so that hnsw_patch_kernel can fill them in
nmn_status upload_graph(nmn_hnsw* h, size_t reserve_n, uint32_t reserve_upper, uint32_t layers) {
    const size_t n_now = h->level.size();
    const size_t n = std::max(n_now, reserve_n);
    const uint32_t m = h->cfg.m, m0 = h->cfg.m0;
    std::vector<uint32_t> l0(n * (size_t)m0, kNone), l0cnt(n), upidx(n, kNone);
    uint32_t n_upper = 0;
    for (size_t i = 0; i < n_now; i++)
        if (h->level[i] > 0) upidx[i] = n_upper++;
    const uint32_t n_upper_now = n_upper;
    n_upper = std::max(n_upper, reserve_upper);
    const uint32_t L = std::max<uint32_t>(std::max<uint32_t>(h->max_layer, 1), layers);
    std::vector<uint32_t> up((size_t)n_upper * L * m, kNone), upcnt((size_t)n_upper * L, 0);
    for (size_t i = 0; i < n_now; i++) {
        const auto& a = h->nbr[i][0];
        l0cnt[i] = (uint32_t)a.size();
        std::copy(a.begin(), a.end(), l0.begin() + i * m0);
        for (uint32_t l = 1; l <= h->level[i]; l++) {
            const auto& b = h->nbr[i][l];
            const size_t slot = (size_t)upidx[i] * L + (l - 1);
            upcnt[slot] = (uint32_t)b.size();
            std::copy(b.begin(), b.end(), up.begin() + slot * m);
        }
    }
    bool synced = true;  // (the caller waited for every search in flight)
    const hipStream_t none = (hipStream_t)-1;
    HN_TRY(grow(h->d_l0, l0.size() * 4, none, &synced));
    HN_TRY(grow(h->d_l0cnt, n * 4, none, &synced));
    HN_TRY(grow(h->d_upidx, n * 4, none, &synced));
    HN_TRY(grow(h->d_up, up.size() * 4, none, &synced));
    HN_TRY(grow(h->d_upcnt, upcnt.size() * 4, none, &synced));
    if (n) {
        HN_TRY(hipMemcpy(h->d_l0.p, l0.data(), l0.size() * 4, hipMemcpyHostToDevice));
        HN_TRY(hipMemcpy(h->d_l0cnt.p, l0cnt.data(), n * 4, hipMemcpyHostToDevice));
        HN_TRY(hipMemcpy(h->d_upidx.p, upidx.data(), n * 4, hipMemcpyHostToDevice));
    }
    if (!up.empty()) {
        HN_TRY(hipMemcpy(h->d_up.p, up.data(), up.size() * 4, hipMemcpyHostToDevice));
        HN_TRY(hipMemcpy(h->d_upcnt.p, upcnt.data(), upcnt.size() * 4, hipMemcpyHostToDevice));
    }
    h->up_layers = L;
    h->n_upper = n_upper_now;
    if (reserve_n) return NMN_OK;  // (the upload that ends the call does the rest)
    // the live mask: every node that came since the last upload is live (an insert, a load — the file does not hold the mask)
    h->live.resize((n + 31) / 32, 0u);
    for (uint64_t i = h->live_n; i < n; i++) h->live[i >> 5] |= 1u << (i & 31);
    h->live_n = n;
    HN_TRY(grow(h->d_live, h->live.size() * 4, none, &synced));
    if (n) HN_TRY(hipMemcpy(h->d_live.p, h->live.data(), h->live.size() * 4, hipMemcpyHostToDevice));
    if (h->n_sparse) {  // the record of every node and the entries of the sparse ones, in node order
        std::vector<uint4> rec(n);
        std::vector<uint2> ent;
        ent.reserve(h->sp_pos.size());
        for (size_t i = 0; i < n; i++) {
            if (!node_is_sparse(h, (uint32_t)i)) {
                rec[i] = make_uint4(0u, 0u, kNone, 0u);
                continue;
            }
            const uint64_t off = ent.size();
            uint32_t mbits;
            memcpy(&mbits, &h->mags[i], 4);
            rec[i] = make_uint4((uint32_t)off, (uint32_t)(off >> 32), h->sp_nnz[i], mbits);
            const SpView s = node_entries(h, (uint32_t)i);
            for (uint64_t e = 0; e < s.nnz; e++) {
                uint32_t bits;
                memcpy(&bits, &s.val[e], 4);
                ent.push_back(make_uint2(s.pos[e], bits));
            }
        }
        HN_TRY(grow(h->d_nrec, n * sizeof(uint4), none, &synced));
        HN_TRY(grow(h->d_nent, std::max<size_t>(ent.size(), 1) * sizeof(uint2), none, &synced));
        HN_TRY(hipMemcpy(h->d_nrec.p, rec.data(), n * sizeof(uint4), hipMemcpyHostToDevice));
        if (!ent.empty()) HN_TRY(hipMemcpy(h->d_nent.p, ent.data(), ent.size() * sizeof(uint2), hipMemcpyHostToDevice));
    }
    if (!h->tt_nodes.empty()) {  // docs/hnsw.md §24: the walk's norms, the slot per node, the record per TT node, the pool of cores
        std::vector<float> wn(n);
        HN_TRY(hipMemcpy(wn.data(), h->vectors->norms, n * 4, hipMemcpyDeviceToHost));  // simd::magnitude of every row
        std::vector<uint32_t> slot(n, kNone);
        std::vector<TTNodeDev> rec(h->tt_nodes.size());
        for (size_t i = 0; i < n; i++) {
            if (!node_is_tt(h, (uint32_t)i)) continue;
            slot[i] = h->tt_slot[i];
            wn[i] = h->mags[i];  // the cached tt_norm: what cosine_distance_dense / _sparse divide by
        }
        for (size_t t = 0; t < rec.size(); t++) {
            const nmn_hnsw::TTNode& tn = h->tt_nodes[t];
            TTNodeDev& r = rec[t];
            memset(&r, 0, sizeof r);
            r.off_lo = (uint32_t)tn.off;
            r.off_hi = (uint32_t)(tn.off >> 32);
            r.n_cores = tn.n_cores;
            memcpy(&r.norm_bits, &tn.norm, 4);
            memcpy(r.modes, tn.shape, sizeof r.modes);
            memcpy(r.ranks, tn.ranks, sizeof r.ranks);
        }
        HN_TRY(grow(h->d_wnorms, n * 4, none, &synced));
        HN_TRY(grow(h->d_ttslot, n * 4, none, &synced));
        HN_TRY(grow(h->d_ttrec, rec.size() * sizeof(TTNodeDev), none, &synced));
        HN_TRY(grow(h->d_ttcores, std::max<size_t>(h->tt_cores.size(), 1) * 4, none, &synced));
        HN_TRY(hipMemcpy(h->d_wnorms.p, wn.data(), n * 4, hipMemcpyHostToDevice));
        HN_TRY(hipMemcpy(h->d_ttslot.p, slot.data(), n * 4, hipMemcpyHostToDevice));
        HN_TRY(hipMemcpy(h->d_ttrec.p, rec.data(), rec.size() * sizeof(TTNodeDev), hipMemcpyHostToDevice));
        if (!h->tt_cores.empty()) HN_TRY(hipMemcpy(h->d_ttcores.p, h->tt_cores.data(), h->tt_cores.size() * 4, hipMemcpyHostToDevice));
    }
    return NMN_OK;
}

// quantized handle: rows [first, first + count) of the host's codes and records into the device arrays (caller waited for the searches)
nmn_status upload_codes(nmn_hnsw* h, uint64_t first, uint64_t count) {
    if (count == 0) return NMN_OK;
    const uint32_t dim = h->dim, ld8 = h->ld8;
    if (h->storage == NMN_HNSW_STORAGE_BINARY) {  // the words alone, the padding word (an odd count) zero
        std::vector<uint8_t> stage((size_t)count * ld8, 0);
        for (uint64_t i = 0; i < count; i++)
            memcpy(stage.data() + (size_t)i * ld8, h->bwords.data() + (size_t)(first + i) * h->bin_w, (size_t)h->bin_w * 8);
        HN_TRY(hipMemcpy((uint8_t*)h->d_codes + (size_t)first * ld8, stage.data(), stage.size(), hipMemcpyHostToDevice));
        return NMN_OK;
    }
    std::vector<uint8_t> stage((size_t)count * ld8, 0);
    std::vector<float> rec((size_t)count * 4);
    for (uint64_t i = 0; i < count; i++) {
        const uint64_t r = first + i;
        memcpy(stage.data() + (size_t)i * ld8, h->codes.data() + (size_t)r * dim, dim);
        rec[4 * i + 0] = h->qscale[r];
        rec[4 * i + 1] = h->qmin[r];
        rec[4 * i + 2] = h->mags[r];
        rec[4 * i + 3] = h->qxsq[r];
    }
    HN_TRY(hipMemcpy((uint8_t*)h->d_codes + (size_t)first * ld8, stage.data(), stage.size(), hipMemcpyHostToDevice));
    HN_TRY(hipMemcpy((float*)h->d_rec + (size_t)first * 4, rec.data(), rec.size() * 4, hipMemcpyHostToDevice));
    return NMN_OK;
}

// quantized handle: device arrays for `cap` rows; the `have` rows already inserted are sent again from the host's copy
nmn_status alloc_codes(nmn_hnsw* h, uint64_t cap, uint64_t have) {
    void *nc = nullptr, *nr = nullptr;
    HN_TRY(hipMalloc(&nc, std::max<size_t>((size_t)cap * h->ld8, 256)));
    if (h->storage == NMN_HNSW_STORAGE_QUANTIZED) {  // (a binary handle keeps no record per row)
        hipError_t e = hipMalloc(&nr, std::max<size_t>((size_t)cap * 16, 256));
        if (e != hipSuccess) {
            (void)hipFree(nc);
            return set_error_hip(e, "hipMalloc");
        }
    }
    if (h->d_codes) (void)hipFree(h->d_codes);
    if (h->d_rec) (void)hipFree(h->d_rec);
    h->d_codes = nc;
    h->d_rec = nr;
    h->vec_cap = cap;
    return upload_codes(h, 0, have);
}

nmn_status ensure_vectors(nmn_hnsw* h, uint64_t need) {
    if ((h->vectors || h->d_codes) && need <= h->vec_cap) return NMN_OK;
    uint64_t cap = std::max<uint64_t>(h->vec_cap, 1024);
    while (cap < need) cap *= 2;
    if (h->cfg.max_nodes > 0) cap = std::min<uint64_t>(cap, std::max<uint64_t>(h->cfg.max_nodes, need));
    if (h->storage != NMN_HNSW_STORAGE_DENSE) return alloc_codes(h, cap, h->level.size());
    nmn_index_desc d{};
    d.dim = h->dim;
    d.capacity_rows = cap;
    d.device = h->device;
    nmn_index* nv = nullptr;
    nmn_status st = nmn_index_create(&d, &nv);
    if (st != NMN_OK) return st;
    const uint64_t have = h->level.size();
    if (have) {
        st = nmn_index_upload(nv, h->rows.data(), 0, have);
        if (st != NMN_OK) {
            nmn_index_destroy(nv);
            return st;
        }
    }
    if (h->vectors) nmn_index_destroy(h->vectors);
    h->vectors = nv;
    h->vec_cap = cap;
    return NMN_OK;
}

}  // namespace hnsw
}  // namespace nmn

namespace {
// ---- nmn_hnsw_insert_bulk (docs/hnsw.md §19) ---------------------------------------------------------------------------------------
// The device side of one call: which upper slot every node has, and which lists the commits of the running batch have assigned —
// a stamp per list holding the number of the batch that last assigned it (layer 0 by node, the upper layers by slot of `up`).
struct BulkCall {
    std::vector<uint32_t> upidx, stamp0, stamp_up;
    std::vector<std::pair<uint32_t, uint32_t>> dirty;  // the lists stamped by this batch, once each: what the patch sends
    uint32_t batch_no = 0, layers = 1, n_upper = 0;
    uint32_t& stamp(uint32_t node, uint32_t layer) {
        return layer == 0 ? stamp0[node] : stamp_up[(size_t)upidx[node] * layers + (layer - 1)];
    }
    void operator()(uint32_t node, uint32_t layer) {
        uint32_t& s = stamp(node, layer);
        if (s != batch_no) {
            s = batch_no;
            dirty.emplace_back(node, layer);
        }
    }
    bool assigned(uint32_t node, uint32_t layer) {  // (an id no list can hold counts as assigned: the host walks that node)
        if (node >= stamp0.size() || (layer > 0 && (upidx[node] == kNone || layer > layers))) return true;
        return stamp(node, layer) == batch_no;
    }
};

double ms_since(const std::chrono::steady_clock::time_point& t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// Whether the device walks for this handle at all, and with which heaps (the search kernel's LDS rule with ef = ef_construction)
bool bulk_eligible(const nmn_hnsw* h) {
    const uint32_t efc = h->cfg.ef_construction;
    if (h->storage != NMN_HNSW_STORAGE_DENSE || h->n_sparse || !h->tt_nodes.empty() || !h->vectors) return false;
    if (efc == 0 || efc > kLdsResultsMax) return false;
    if (h->lds_rcap && h->lds_rcap < efc + 1) return false;
    return true;
}

// One batch: launch, read back.  Caller holds rw exclusively and host_mu.  On return `out` holds status [nb], selcnt [nb][layers],
// rdend [nb][layers], sel [nb][sel_stride], reads [nb][rd_cap].
hipError_t bulk_walk(nmn_hnsw* h, uint64_t call_first, uint32_t first, uint32_t nb, uint32_t rd_cap, std::vector<uint32_t>& out) {
    const uint32_t n = (uint32_t)h->level.size(), efc = h->cfg.ef_construction;
    InsertArgs a{};
    a.g = graph_args(h, n).g;
    const uint32_t layers = a.g.max_layer + 1;
    a.levels = (const uint8_t*)h->bk_lv.p;
    a.lv_base = (uint32_t)call_first;
    a.first = first;
    a.nb = nb;
    a.ef = efc;
    a.rcap = results_need(efc, n);
    a.ccap = cand_cap(efc, h->lds_ccap, h->dim, n);
    a.qlds = (h->dim + 7u) & ~7u;
    a.vwords = std::max<uint32_t>((n + 31) / 32, 1);
    a.sel_stride = a.g.m0 + a.g.max_layer * a.g.m;
    a.rd_cap = rd_cap;
    const size_t words = (size_t)nb * (1 + 2 * (size_t)layers + a.sel_stride + rd_cap);
    bool synced = false;
    hipStream_t s = h->host_stream;
    hipError_t e = grow(h->bk_vis, (size_t)nb * a.vwords * 4, s, &synced);
    if (e == hipSuccess) e = grow(h->bk_out, words * 4, s, &synced);
    if (e != hipSuccess) return e;
    a.visited = (uint32_t*)h->bk_vis.p;
    a.status = (uint32_t*)h->bk_out.p;
    a.selcnt = a.status + nb;
    a.rdend = a.selcnt + (size_t)nb * layers;
    a.sel = a.rdend + (size_t)nb * layers;
    a.reads = a.sel + (size_t)nb * a.sel_stride;
    const size_t lds = (size_t)a.qlds * 4 + 32 * 4 + 32 * 4 + 8 * 4 + ((size_t)a.rcap + a.ccap) * sizeof(Ent);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    launch_insert_walk(nb, lds, s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    out.resize(words);
    e = hipMemcpyAsync(out.data(), h->bk_out.p, words * 4, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(s);
}

// The lists of `bc.dirty` (and the upper slots of the batch's new nodes, `new_upper`) as records of hnsw_patch_kernel, sent and
// scattered behind whatever is on the stream; the next walk launch is enqueued behind the scatter.
hipError_t bulk_patch(nmn_hnsw* h, const BulkCall& bc, const std::vector<uint32_t>& new_upper, size_t nodes_cap, size_t upper_cap,
                      std::vector<uint32_t>& stage) {
    const uint32_t m = h->cfg.m, m0 = h->cfg.m0, stride = 3 + std::max(m, m0);
    const size_t nrec = bc.dirty.size() + new_upper.size();
    if (nrec == 0) return hipSuccess;
    stage.assign(nrec * stride, kNone);
    size_t r = 0;
    for (uint32_t node : new_upper) {  // (first: a list record below may target the slot)
        uint32_t* rec = stage.data() + r++ * stride;
        rec[0] = 2u;
        rec[1] = node;
        rec[2] = bc.upidx[node];
    }
    for (const auto& d : bc.dirty) {
        uint32_t* rec = stage.data() + r++ * stride;
        const std::vector<uint32_t>& lst = h->nbr[d.first][d.second];
        rec[0] = d.second == 0 ? 0u : 1u;
        rec[1] = d.second == 0 ? d.first : (uint32_t)((size_t)bc.upidx[d.first] * bc.layers + (d.second - 1));
        rec[2] = (uint32_t)lst.size();
        std::copy(lst.begin(), lst.end(), rec + 3);
    }
    bool synced = false;
    hipStream_t s = h->host_stream;
    hipError_t e = grow(h->bk_patch, stage.size() * 4, s, &synced);
    if (e != hipSuccess) return e;
    e = hipMemcpyAsync(h->bk_patch.p, stage.data(), stage.size() * 4, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    PatchArgs a{};
    a.l0 = (uint32_t*)h->d_l0.p;
    a.l0cnt = (uint32_t*)h->d_l0cnt.p;
    a.up_idx = (uint32_t*)h->d_upidx.p;
    a.up = (uint32_t*)h->d_up.p;
    a.upcnt = (uint32_t*)h->d_upcnt.p;
    a.rec = (const uint32_t*)h->bk_patch.p;
    a.nrec = (uint32_t)nrec;
    a.stride = stride;
    a.m = m;
    a.m0 = m0;
    a.nodes = nodes_cap;
    a.up_slots = upper_cap * bc.layers;
    launch_patch((uint32_t)std::min<size_t>(nrec, 65535), s, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(s);  // (`stage` is pageable and reused; the wait is also what the patch time of the trace measures)
}

// The n rows [have, have + n) of a dense-query insert, already in h->rows and on the device: levels first, then batches.
// Caller (insert_rows) holds rw exclusively and has waited for every search in flight.
void bulk_insert_nodes(nmn_hnsw* h, uint64_t have, uint64_t n, HostVisited& vis, uint64_t* ids_out) {
    const bool q8 = h->storage == NMN_HNSW_STORAGE_QUANTIZED, bin = h->storage == NMN_HNSW_STORAGE_BINARY;
    const uint32_t dim = h->dim;
    std::vector<uint8_t> lv(n);
    for (uint64_t i = 0; i < n; i++) lv[i] = (uint8_t)next_level(h);  // random_level once per insert, in order (hnsw.rs:1957)
    h->bulk_trace.clear();
    nmn_hnsw_bulk_stats& st = h->bulk_stats;
    auto prelude = [&](uint64_t i) {  // what insert_rows does for a Dense row before the node is linked
        if (h->n_sparse) {
            h->sp_nnz.resize(have + i + 1, kNone);
            h->sp_off.resize(have + i + 1, 0);
            h->sp_mag64.resize(have + i + 1, 0.0);
        }
        if (!q8 && !bin) {
            const float* v = h->rows.data() + (have + i) * dim;
            h->mags.push_back(sqrtf(h_dot8(v, v, dim)));
        }
        if (ids_out) ids_out[i] = have + i;
    };
    uint64_t i = 0;
    NoMark none;
    const uint64_t min_nodes = h->bulk_min_nodes ? h->bulk_min_nodes : kBulkMinNodes;
    const bool eligible = bulk_eligible(h);
    // the host's path: an ineligible handle, the first node of an empty index, a graph below min_nodes, and a call that leaves the
    // device fewer than kBulkMinRows rows — a launch waits one walk's latency, several host walks long (docs/hnsw.md §19.5), and
    // the device phase uploads the whole adjacency once more
    while (i < n && (!eligible || h->entry == ~0ull || h->level.size() < min_nodes || n - i < kBulkMinRows)) {
        prelude(i);
        host_insert_node_at(h, (uint32_t)(have + i), lv[i], vis, none);
        st.host_nodes++;
        i++;
    }
    if (i == n) return;
    // the device side of the call, sized once: everything below is known from the levels
    std::lock_guard<std::mutex> hl(h->host_mu);
    BulkCall bc;
    const size_t n_final = have + n;
    bc.upidx.assign(n_final, kNone);
    for (size_t k = 0; k < h->level.size(); k++)
        if (h->level[k] > 0) bc.upidx[k] = bc.n_upper++;
    uint32_t upper_final = bc.n_upper, top = h->max_layer;
    for (uint64_t k = i; k < n; k++) {
        upper_final += lv[k] > 0 ? 1u : 0u;
        top = std::max<uint32_t>(top, lv[k]);
    }
    bc.layers = std::max<uint32_t>(top, 1);
    bc.stamp0.assign(n_final, 0u);
    bc.stamp_up.assign((size_t)upper_final * bc.layers, 0u);
    const uint32_t rd_cap = 4 * h->cfg.ef_construction + 256;
    bool device = upload_graph(h, n_final, upper_final, bc.layers) == NMN_OK;
    if (device) {
        bool synced = true;
        device = grow(h->bk_lv, (size_t)n, (hipStream_t)-1, &synced) == hipSuccess &&
                 hipMemcpy(h->bk_lv.p, lv.data(), (size_t)n, hipMemcpyHostToDevice) == hipSuccess;
    }
    std::vector<uint32_t> out, stage, new_upper;
    while (i < n && device) {
        uint32_t nb = (uint32_t)std::min<uint64_t>(h->bulk_batch ? h->bulk_batch : h->bulk_b, n - i);
        const uint32_t launch_max = h->max_layer;
        for (uint32_t j = 0; j < nb; j++)
            if (lv[i + j] > launch_max) {  // its commit moves the entry point: the batch ends behind it
                nb = j + 1;
                break;
            }
        bc.batch_no++;
        bc.dirty.clear();
        new_upper.clear();
        auto t0 = std::chrono::steady_clock::now();
        if (bulk_walk(h, have, (uint32_t)(have + i), nb, rd_cap, out) != hipSuccess) {
            device = false;
            break;
        }
        const float walk_ms = (float)ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        const uint32_t layers = launch_max + 1, sel_stride = h->cfg.m0 + launch_max * h->cfg.m;
        const uint32_t* status = out.data();
        const uint32_t* selcnt = status + nb;
        const uint32_t* rdend = selcnt + (size_t)nb * layers;
        const uint32_t* sel = rdend + (size_t)nb * layers;
        const uint32_t* reads = sel + (size_t)nb * sel_stride;
        uint32_t redone = 0;
        for (uint32_t j = 0; j < nb; j++) {
            const uint32_t node = (uint32_t)(have + i + j), level = lv[i + j];
            prelude(i + j);
            if (level > 0) {
                bc.upidx[node] = bc.n_upper++;
                new_upper.push_back(node);
            }
            bool take = status[j] == 0u;
            if (!take) {
                st.overflowed++;
            } else {  // the walk stands iff no list it read has been assigned since the launch
                const uint32_t* rd = reads + (size_t)j * rd_cap;
                uint32_t at = 0;
                for (int layer = (int)launch_max; layer >= 0 && take; layer--) {
                    const uint32_t end = std::min(rdend[(size_t)j * layers + (uint32_t)layer], rd_cap);
                    for (; at < end; at++)
                        if (bc.assigned(rd[at], (uint32_t)layer)) {
                            take = false;
                            break;
                        }
                }
                if (take)
                    st.accepted++;
                else
                    st.conflicts++;
            }
            if (take) {
                host_commit_walked(h, node, level, sel + (size_t)j * sel_stride, selcnt + (size_t)j * layers, bc);
            } else {
                host_insert_node_at(h, node, level, vis, bc);
                redone++;
            }
        }
        st.batches++;
        st.walks += nb;
        i += nb;
        const float commit_ms = (float)ms_since(t0);
        t0 = std::chrono::steady_clock::now();
        if (i < n) {
            if (bulk_patch(h, bc, new_upper, n_final, upper_final, stage) != hipSuccess)
                device = false;
            else
                st.patched_lists += bc.dirty.size();
        }
        if (h->bulk_trace.size() < (5u << 20)) {
            const float rec[5] = {(float)nb, (float)redone, walk_ms, commit_ms, (float)ms_since(t0)};
            h->bulk_trace.insert(h->bulk_trace.end(), rec, rec + 5);
        }
        if (!h->bulk_batch) {  // the adaptive policy: statistics only, never the graph
            if (4 * redone <= nb)
                h->bulk_b = std::min<uint32_t>(2 * h->bulk_b, 256);
            else if (2 * redone >= nb)
                h->bulk_b = std::max<uint32_t>(h->bulk_b / 2, 4);
        }
    }
    if (!device) (void)hipGetLastError();
    for (; i < n; i++) {  // a device error: the rest of the call on the host; whole nodes only, either way
        prelude(i);
        host_insert_node_at(h, (uint32_t)(have + i), lv[i], vis, none);
        st.host_nodes++;
    }
}

}  // namespace

namespace nmn {
namespace hnsw {
// nmn_hnsw_insert, nmn_hnsw_insert_sparse and nmn_hnsw_insert_auto behind their argument checks.  rows_host: the n rows as the
// flat index keeps them (to_dense() of a Sparse node).  sp / sp_row (dense handle only, nullable): row i is EmbeddingStorage::Sparse
// with the entries of sp's vector sp_row[i] when sp_row[i] >= 0, Dense otherwise.
// tt / tt_norms (dense handle only, nullable): row i is EmbeddingStorage::TensorTrain with train i of the batch, rows_host its
// tt_reconstruct() and tt_norms[i] its raw tt_norm.
nmn_status insert_rows(nmn_hnsw* h, const float* rows_host, uint64_t n, const SparseQueries* sp, const int64_t* sp_row,
                       uint64_t* ids_out, bool bulk, const TTBatch* tt, const float* tt_norms) {
    std::unique_lock<std::shared_mutex> g(h->rw);
    const uint64_t have = h->level.size();
    if (h->cfg.max_nodes > 0 && have + n > h->cfg.max_nodes) {  // hnsw.rs:1947-1955, text of 102-107; the batch is all or nothing
        char buf[160];
        snprintf(buf, sizeof buf, "HNSW index at capacity: %llu nodes (limit: %llu)", (unsigned long long)have,
                 (unsigned long long)h->cfg.max_nodes);
        return set_error(NMN_ERR_CAPACITY, buf);
    }
    if (have + n >= (uint64_t)kNone) return set_error(NMN_ERR_CAPACITY, "HNSW: node ids are 32 bits on the device");
    HN_TRY(hipSetDevice(h->device));
    nmn_status st = wait_in_flight(h);
    if (st != NMN_OK) return st;
    {
        std::lock_guard<std::mutex> hl(h->host_mu);
        HN_TRY(hipStreamSynchronize(h->host_stream));
    }
    const bool q8 = h->storage == NMN_HNSW_STORAGE_QUANTIZED, bin = h->storage == NMN_HNSW_STORAGE_BINARY;
    const uint32_t dim = h->dim;
    if (bin) {  // insert_embedding(Binary(from_dense(row, threshold))); what the host keeps as the row is to_dense()
        h->rows.resize((have + n) * dim);
        h->bwords.resize((have + n) * h->bin_w);
        h->mags.resize(have + n, h->sqrt_dim);
        std::vector<float> tmp;
        for (uint64_t r = have; r < have + n; r++)
            h_bin_from_dense(rows_host + (r - have) * dim, dim, h->bin_method, h->bwords.data() + r * h->bin_w, h->rows.data() + r * dim, tmp);
        st = ensure_vectors(h, have + n);
        if (st == NMN_OK && have + n <= h->vec_cap) st = upload_codes(h, have, n);
    } else if (q8) {  // insert_quantized, hnsw.rs:1711-1714: from_dense; what the host keeps as the row is dequantize()
        h->rows.resize((have + n) * dim);
        h->codes.resize((have + n) * dim);
        h->qscale.resize(have + n);
        h->qmin.resize(have + n);
        h->qxsq.resize(have + n);
        h->mags.resize(have + n);
        for (uint64_t r = have; r < have + n; r++) {
            uint8_t* code = h->codes.data() + r * dim;
            h_quantize(rows_host + (r - have) * dim, dim, code, &h->qscale[r], &h->qmin[r]);
            float* v = h->rows.data() + r * dim;
            h_dequantize(code, dim, h->qscale[r], h->qmin[r], v);
            h->mags[r] = sqrtf(h_dot8(v, v, dim));  // magnitude_immutable, hnsw.rs:401-407
            h->qxsq[r] = h_q8_sqmag(code, h->qscale[r], h->qmin[r], dim);
        }
        st = ensure_vectors(h, have + n);
        if (st == NMN_OK && have + n <= h->vec_cap) st = upload_codes(h, have, n);
    } else {
        h->rows.insert(h->rows.end(), rows_host, rows_host + n * dim);
        st = ensure_vectors(h, have + n);
        if (st == NMN_OK) st = nmn_index_upload(h->vectors, rows_host, have, n);
    }
    if (st != NMN_OK) {
        h->rows.resize(have * dim);
        if (bin) {
            h->bwords.resize(have * h->bin_w);
            h->mags.resize(have);
        }
        if (q8) {
            h->codes.resize(have * dim);
            h->qscale.resize(have);
            h->qmin.resize(have);
            h->qxsq.resize(have);
            h->mags.resize(have);
        }
        return st;
    }
    static thread_local HostVisited vis;
    if (bulk) {
        bulk_insert_nodes(h, have, n, vis, ids_out);
        return upload_graph(h);
    }
    for (uint64_t i = 0; i < n; i++) {
        const bool sparse = sp && sp_row[i] >= 0;
        if (sparse || h->n_sparse) {  // a kind per node from the first Sparse one on
            h->sp_nnz.resize(have + i + 1, kNone);
            h->sp_off.resize(have + i + 1, 0);
            h->sp_mag64.resize(have + i + 1, 0.0);
        }
        if (sparse) {
            const uint32_t r = (uint32_t)sp_row[i];
            const uint64_t c = sp->nnz(r);
            h->sp_nnz[have + i] = (uint32_t)c;
            h->sp_off[have + i] = h->sp_pos.size();
            h->sp_pos.insert(h->sp_pos.end(), sp->pos.begin() + sp->off[r], sp->pos.begin() + sp->off[r + 1]);
            h->sp_val.insert(h->sp_val.end(), sp->val.begin() + sp->off[r], sp->val.begin() + sp->off[r + 1]);
            h->sp_mag64[have + i] = h_sparse_mag64(sp->val.data() + sp->off[r], c);
            h->mags.push_back(sp->mag[r]);  // SparseVector::magnitude(): what distance_dense / distance_sparse divide by
            h->n_sparse++;
            if (sp->dup[r]) h->n_sparse_dup++;
        } else if (tt) {  // TTVectorCached::new (hnsw.rs:276-289): the train and norm = tt_norm(tt), the raw value
            const uint32_t q = (uint32_t)i;
            nmn_hnsw::TTNode tn;
            tn.n_cores = tt->n_cores;
            memcpy(tn.shape, tt->shape, sizeof tn.shape);
            const uint32_t* r = tt->ranks_of(q);
            bool big = false;
            for (uint32_t c = 0; c <= tt->n_cores; c++) {
                tn.ranks[c] = r[c];
                h->tt_max_rank = std::max(h->tt_max_rank, r[c]);
                big = big || r[c] > kTTMaxRank;
            }
            tn.storage = tt->storage_of(q);
            tn.off = h->tt_cores.size();
            const float* src = tt->cores + tt->offset_of(q);
            h->tt_cores.insert(h->tt_cores.end(), src, src + tn.storage);
            tn.norm = tt_norms[i];
            const float* v = h->rows.data() + (have + i) * dim;
            tn.row_mag = sqrtf(h_dot8(v, v, dim));  // simd::magnitude of the reconstruction: the T x D pruning arms
            if (big || tn.storage > kTTMaxStorage) h->n_tt_big++;
            h->tt_slot.resize(have + i + 1, kNone);
            h->tt_slot[have + i] = (uint32_t)h->tt_nodes.size();
            h->tt_nodes.push_back(tn);
            h->mags.push_back(tn.norm);  // what cosine_distance_dense / _sparse divide by (hnsw.rs:976, 1023)
        } else if (!q8 && !bin) {
            const float* v = h->rows.data() + (have + i) * dim;
            h->mags.push_back(sqrtf(h_dot8(v, v, dim)));  // simd::magnitude, hnsw.rs:198-229
        }
        host_insert_node(h, (uint32_t)(have + i), vis);
        if (ids_out) ids_out[i] = have + i;
    }
    return upload_graph(h);
}
}  // namespace hnsw
}  // namespace nmn

namespace {
nmn_status refuse_sparse_on_q8(const nmn_hnsw* h) {
    if (h->storage == NMN_HNSW_STORAGE_DENSE) return NMN_OK;
    if (const nmn_status sb = refuse_binary(h, "nmn_hnsw_insert_sparse / nmn_hnsw_insert_auto", kBinNodes); sb != NMN_OK) return sb;
    return set_error(NMN_ERR_CONFIGURATION,
                     "HNSW: sparse nodes are served on a dense handle only (the Quantized x Sparse arms are out of scope)");
}
}  // namespace

extern "C" nmn_status nmn_hnsw_insert(nmn_hnsw* h, const float* rows_host, uint64_t n, uint64_t* ids_out) {
    if (!h || (!rows_host && n)) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return NMN_OK;
    const char* e = getenv("NMN_HNSW_BULK_BUILD");  // read at every call; the graph is the same either way (docs/hnsw.md §19)
    return insert_rows(h, rows_host, n, nullptr, nullptr, ids_out, e && e[0] == '1');
}

extern "C" nmn_status nmn_hnsw_insert_bulk(nmn_hnsw* h, const float* rows_host, uint64_t n, uint64_t* ids_out) {
    if (!h || (!rows_host && n)) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return NMN_OK;
    return insert_rows(h, rows_host, n, nullptr, nullptr, ids_out, true);
}

extern "C" nmn_status nmn_hnsw_set_bulk_policy(nmn_hnsw* h, uint32_t batch, uint32_t min_nodes) {
    if (!h) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (batch > kBulkBatchMax) return set_error(NMN_ERR_INVALID_ARGUMENT, "HNSW: a bulk batch holds 1024 nodes at most");
    std::unique_lock<std::shared_mutex> g(h->rw);
    h->bulk_batch = batch;
    h->bulk_min_nodes = min_nodes;
    return NMN_OK;
}

extern "C" nmn_status nmn_hnsw_get_bulk_stats(nmn_hnsw* h, nmn_hnsw_bulk_stats* out) {
    if (!h || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_lock<std::shared_mutex> g(h->rw);
    *out = h->bulk_stats;
    return NMN_OK;
}

extern "C" nmn_status nmn_hnsw_get_bulk_trace(nmn_hnsw* h, float* out, uint64_t cap, uint64_t* count) {
    if (!h || !count) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_lock<std::shared_mutex> g(h->rw);
    const uint64_t nrec = h->bulk_trace.size() / 5;
    *count = nrec;
    if (out) memcpy(out, h->bulk_trace.data(), (size_t)std::min(cap, nrec) * 5 * sizeof(float));
    return NMN_OK;
}

// HNSWIndex::insert_sparse (hnsw.rs:1660-1662) for each of the n CSR rows, in order.  Every row is made a SparseVector as
// try_from_parts makes it, for the whole batch, before anything is inserted.
extern "C" nmn_status nmn_hnsw_insert_sparse(nmn_hnsw* h, const uint64_t* indptr, const uint32_t* positions, const float* values,
                                             uint64_t n, uint64_t* ids_out) {
    if (!h || (!indptr && n)) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    nmn_status st = refuse_sparse_on_q8(h);
    if (st != NMN_OK) return st;
    if (n == 0) return NMN_OK;
    if (n >= (uint64_t)kNone) return set_error(NMN_ERR_CAPACITY, "HNSW: node ids are 32 bits on the device");
    SparseQueries sv;
    st = canonicalise_sparse(h->dim, indptr, positions, values, (uint32_t)n, &sv);
    if (st != NMN_OK) return st;
    std::vector<float> dense((size_t)n * h->dim);
    std::vector<int64_t> row(n);
    for (uint64_t i = 0; i < n; i++) {
        sv.to_dense((uint32_t)i, h->dim, dense.data() + (size_t)i * h->dim);
        row[i] = (int64_t)i;
    }
    return insert_rows(h, dense.data(), n, &sv, row.data(), ids_out);
}

// HNSWIndex::insert_auto (hnsw.rs:1671-1680) per row: Sparse(from_dense(row)) iff 1 - nnz / dim >= sparsity_threshold, in f32
extern "C" nmn_status nmn_hnsw_insert_auto(nmn_hnsw* h, const float* rows_host, uint64_t n, uint64_t* ids_out) {
    if (!h || (!rows_host && n)) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    nmn_status st = refuse_sparse_on_q8(h);
    if (st != NMN_OK) return st;
    if (n == 0) return NMN_OK;
    const uint32_t dim = h->dim;
    const float threshold = h->cfg.sparsity_threshold;
    SparseQueries sv;
    sv.off.assign(1, 0);
    std::vector<float> dense(rows_host, rows_host + (size_t)n * dim);
    std::vector<int64_t> row(n, -1);
    for (uint64_t i = 0; i < n; i++) {
        float* v = dense.data() + (size_t)i * dim;
        uint32_t nnz = 0;
        for (uint32_t j = 0; j < dim; j++) nnz += v[j] != 0.0f ? 1u : 0u;  // (NaN counts)
        const float ratio = (float)nnz / (float)dim;
        const float sparsity = 1.0f - ratio;
        if (!(sparsity >= threshold)) continue;  // (a NaN threshold: Dense)
        row[i] = (int64_t)sv.mag.size();
        for (uint32_t j = 0; j < dim; j++) {  // try_from_dense, sparse_vector.rs:212-236; the row kept is to_dense(): -0.0 becomes +0.0
            if (v[j] != 0.0f) {
                sv.pos.push_back(j);
                sv.val.push_back(v[j]);
            } else {
                v[j] = 0.0f;
            }
        }
        sv.off.push_back(sv.pos.size());
        sv.mag.push_back(h_sparse_mag(sv.val.data() + sv.off[sv.mag.size()], sv.off.back() - sv.off[sv.mag.size()]));
        sv.dup.push_back(0);
    }
    return insert_rows(h, dense.data(), n, &sv, row.data(), ids_out);
}

// The stored entries of a node: *nnz = their count, UINT32_MAX for a Dense (or Quantized) node; positions_out / values_out nullable
extern "C" nmn_status nmn_hnsw_sparse_row(nmn_hnsw* h, uint64_t node, uint32_t* positions_out, float* values_out, uint32_t cap,
                                          uint32_t* nnz) {
    if (!h || !nnz) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_lock<std::shared_mutex> g(h->rw);
    if (node >= h->level.size()) return set_error(NMN_ERR_NOT_FOUND, "HNSW: no such node");
    if (!node_is_sparse(h, (uint32_t)node)) {
        *nnz = UINT32_MAX;
        return NMN_OK;
    }
    const SpView s = node_entries(h, (uint32_t)node);
    *nnz = (uint32_t)s.nnz;
    if (!positions_out && !values_out) return NMN_OK;
    if (cap < s.nnz) return set_error(NMN_ERR_BUFFER_TOO_SMALL, "nmn_hnsw_sparse_row");
    if (positions_out && s.nnz) memcpy(positions_out, s.pos, s.nnz * 4);
    if (values_out && s.nnz) memcpy(values_out, s.val, s.nnz * 4);
    return NMN_OK;
}
