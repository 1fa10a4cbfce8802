// nmn_hnsw_handle.h — the HNSW handle (struct nmn_hnsw) and what the translation units of the index share of it
// (docs/hnsw.md, "Source layout"): the device buffers, the canonical sparse queries, HN_TRY, the visited set of the host walks,
// the kernel arguments of a handle, and the declarations of what crosses files.  Whatever has external linkage is in nmn::hnsw.
#pragma once
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <vector>

#include "nmn_index.h"
#include "nmn_internal.h"
#include "nmn_hnsw_queue.h"
#include "nmn_hnsw_kernels.h"
#include "nmn_tt.h"

namespace nmn {
namespace hnsw {
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};
}  // namespace hnsw

// The queries of one nmn_hnsw_search_sparse call as SparseVector::try_from_parts leaves them: entries with val == 0.0 (either sign)
// dropped, NaN kept, the rest stably sorted by position (duplicates survive in input order).  (Named in nmn:: because a HostWalk
// carries a pointer to it through the coalescer, nmn_hnsw_queue.h.)
struct SparseQueries {
    std::vector<uint64_t> off;  // [nq + 1]
    std::vector<uint32_t> pos;
    std::vector<float> val;
    std::vector<float> mag;     // Q.magnitude() per query
    std::vector<uint8_t> dup;   // 1: the query holds a duplicated position
    uint64_t nnz(uint32_t q) const { return off[q + 1] - off[q]; }
    void to_dense(uint32_t q, uint32_t dim, float* out) const {  // zeros, then the entries in order: the last of a position wins
        std::fill(out, out + dim, 0.0f);
        for (uint64_t i = off[q]; i < off[q + 1]; i++) out[pos[i]] = val[i];
    }
};
}  // namespace nmn

struct nmn_hnsw {
    using DevBuf = nmn::hnsw::DevBuf;
    nmn_hnsw_config cfg{};
    uint32_t dim = 0;
    int device = 0;
    int storage = NMN_HNSW_STORAGE_DENSE;  // one strategy per handle
    nmn_index* vectors = nullptr;          // dense handle only
    uint64_t vec_cap = 0;                  // rows the flat index (dense) or the code / record arrays (quantized) are allocated for
    // host side: the rows (quantized handle: the DEQUANTIZED rows, what the pruning side computes on), their magnitudes, the graph
    std::vector<float> rows;
    std::vector<float> mags;
    // quantized handle: ScalarQuantizedVector per row — codes [n][dim], scale, min_val, squared_magnitude()
    std::vector<uint8_t> codes;
    std::vector<float> qscale, qmin, qxsq;
    void* d_codes = nullptr;  // [vec_cap][ld8] u8
    void* d_rec = nullptr;    // [vec_cap] float4 {scale, min_val, magnitude, squared_magnitude}
    uint32_t ld8 = 0;
    // binary handle: BinaryVector per row — words [n][bin_w], bin_w = ceil(dim / 64); rows holds to_dense(), the +-1 row (what a
    // quantized handle keeps its dequantized row for: the node's own query and the Euclidean / DotProduct pruning).  On the device
    // d_codes holds the words, ld8 = 16 ceil(dim / 128) bytes apart; d_rec stays null.
    std::vector<uint64_t> bwords;
    uint32_t bin_w = 0;
    int bin_method = NMN_BINARY_SIGN;
    float sqrt_dim = 0.0f;  // (dimension as f32).sqrt(): every Binary row's magnitude, hnsw.rs:981-984
    // EmbeddingStorage::Sparse nodes of a dense handle (docs/hnsw.md §15).  Empty until the first one is inserted; from then on one
    // slot per node: sp_nnz (kNone: a Dense node), sp_off into sp_pos / sp_val (the canonical entries), sp_mag64 = magnitude_f64().
    // rows holds to_dense() of such a node, mags its SparseVector::magnitude() (what the query side divides by).
    std::vector<uint32_t> sp_nnz;
    std::vector<uint64_t> sp_off;
    std::vector<double> sp_mag64;
    std::vector<uint32_t> sp_pos;
    std::vector<float> sp_val;
    uint64_t n_sparse = 0, n_sparse_dup = 0;  // sparse nodes; those of them with a duplicated position
    // EmbeddingStorage::TensorTrain nodes of a dense handle (docs/hnsw.md §24).  Empty until the first one is inserted; from then on
    // one slot per node: tt_slot (kNone: not a TT node) into tt_nodes, whose cores sit back to back in tt_cores.  rows holds
    // tt_reconstruct() of such a node, mags its cached tt_norm — the RAW norm, what the query side divides by — and the record
    // keeps simd::magnitude of the row beside it: what the T x D pruning arms divide by.
    struct TTNode {
        uint64_t off = 0, storage = 0;  // into tt_cores, in floats
        uint32_t n_cores = 0;
        uint32_t shape[nmn::kTTMaxCores] = {};
        uint32_t ranks[nmn::kTTMaxCores + 1] = {};
        float norm = 0.0f, row_mag = 0.0f;
    };
    std::vector<uint32_t> tt_slot;
    std::vector<TTNode> tt_nodes;
    std::vector<float> tt_cores;
    uint64_t n_tt_big = 0;     // TT nodes above nmn_tt_limits (a rank above max_rank, more than max_storage core floats)
    uint32_t tt_max_rank = 0;  // the largest rank of any TT node
    std::vector<uint8_t> level;
    std::vector<std::vector<std::vector<uint32_t>>> nbr;  // [node][layer], id-ascending
    uint64_t entry = ~0ull;
    uint32_t max_layer = 0;
    uint64_t rng = 42;  // hnsw.rs:1584
    // device side
    DevBuf d_l0, d_l0cnt, d_upidx, d_up, d_upcnt;
    DevBuf d_nrec, d_nent;  // a handle with sparse nodes: the record per node and the entries of all sparse nodes (SearchArgs)
    // a handle with TT nodes: the norms the walk divides by (the flat index's, the TT nodes' entries replaced by their tt_norm), the
    // slot per node, the record per TT node and the pool of their cores (SearchArgs)
    DevBuf d_wnorms, d_ttslot, d_ttrec, d_ttcores;
    // the live mask (docs/hnsw.md §16): one bit per node, here and in HBM beside the adjacency.  A new node is live;
    // nmn_hnsw_set_node_mask flips bits.  Only nmn_hnsw_cache_search* read it.  live_n: the nodes that have their bit.
    std::vector<uint32_t> live;
    uint64_t live_n = 0;
    DevBuf d_live;
    uint32_t up_layers = 1, n_upper = 0;
    uint32_t lds_rcap = 0, lds_ccap = 0;  // nmn_hnsw_set_heap_capacity (0 = default)
    // nmn_hnsw_insert_bulk (docs/hnsw.md §19): the policy, the adaptive batch size as the last call left it, the counters, the
    // batches of the last call as {walks, not accepted, walk ms, validation + commit ms, patch ms}, and the device side of a call
    uint32_t bulk_batch = 0, bulk_min_nodes = 0;  // nmn_hnsw_set_bulk_policy (0 = default)
    uint32_t bulk_b = 8;
    nmn_hnsw_bulk_stats bulk_stats{};
    std::vector<float> bulk_trace;
    DevBuf bk_lv, bk_vis, bk_out, bk_patch;
    struct Scratch {
        hipStream_t stream = nullptr;
        std::mutex mu;
        DevBuf vis, flags, evals, spill;
        bool xsort_use = false;  // this call's ordering goes through the large-k sort (xmetric_order_scratch_bytes != 0)
        DevBuf xids, xsc, xcnt, xsim, xsort;  // nmn_hnsw_search_metric*: the walk's nq x c candidate block, its re-rank scores, the sort's scratch
        DevBuf ttq, ttmag, ttkind;  // nmn_hnsw_search_tt*: the reconstructed queries, their magnitudes, kind and candidate limit per query
        // nmn_hnsw_search_sparse_device / nmn_hnsw_cache_search_sparse_device (docs/hnsw.md §22): what the canonicaliser leaves of the
        // call's queries — offsets [nq + 1], packed (position, value bits) pairs, magnitudes, duplicate flags, to_dense() rows, statuses
        DevBuf sq_off, sq_ent, sq_mag, sq_dup, sq_dense, sq_status;
    };
    std::vector<std::unique_ptr<Scratch>> scratch;
    std::vector<hipEvent_t> ev_pending, ev_free;
    std::mutex dev_mu;          // scratch list and events
    std::shared_mutex rw;       // searches shared, insert exclusive
    // the host-buffer search
    std::mutex host_mu;
    hipStream_t host_stream = nullptr;
    DevBuf hq, hids, hsc, hcnt, hkef;
    DevBuf hsp_off, hsp_ent, hqmag;  // sparse slots of a batch: the launch's entry offsets, its (position, value) pairs, Q.magnitude() per query
    DevBuf hxmeta, hxsim, hxoids, hxosc, hxocnt, hxsort;  // a batch's metric slots (docs/hnsw.md §12): what their launches read and answer into
    DevBuf htt_cores, htt_ranks, htt_off, htt_skip;  // nmn_hnsw_search_tt: the call's trains as the preparation kernel reads them
    // ... and what a batch of mixed k / ef passes through on the host (under host_mu): the queries gathered in launch order, k and ef
    // per query, the launch's rows before they are handed to their callers
    std::vector<float> st_q;
    std::vector<uint32_t> st_kef, st_cnt;
    std::vector<uint64_t> st_ids;
    std::vector<float> st_sc;
    std::vector<nmn::XmetricBatchItem> st_xitems;
    std::vector<uint32_t> st_xmeta, st_xocnt;
    std::vector<uint64_t> st_xoids;
    std::vector<float> st_xosc;
    // ... and a batch's sparse slots (docs/hnsw.md §14): the entries of the kind-1 queries as a CSR in launch order, Q.magnitude() per query
    std::vector<uint64_t> st_spoff;
    std::vector<uint2> st_spent;
    std::vector<float> st_mag;
    // the request coalescer in front of it (docs/hnsw.md §11): one batch runs at a time, whoever arrives meanwhile waits here
    nmn::WalkQueue co;
};

#define HN_TRY(expr)                                                  \
    do {                                                              \
        hipError_t _e = (expr);                                       \
        if (_e != hipSuccess) return set_error_hip(_e, #expr);        \
    } while (0)

namespace nmn {
namespace hnsw {

inline hipError_t grow(DevBuf& b, size_t bytes, hipStream_t s, bool* synced) {
    if (bytes <= b.cap) return hipSuccess;
    if (s != (hipStream_t)-1 && !*synced) {  // what is in flight on the stream may read the old buffer
        hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) return e;
        *synced = true;
    }
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
    const size_t want = std::max<size_t>(bytes + bytes / 4, 256);
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) return e;
    b.cap = want;
    return hipSuccess;
}
inline void drop(DevBuf& b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

// What a Binary-storage handle does not serve (refuse_binary, docs/hnsw.md §18)
constexpr const char* kBinNoRows = "it keeps one bit per dimension and no f32 rows on the device";
constexpr const char* kBinQueries = "Binary rows are walked with dense queries only";
constexpr const char* kBinNodes = "a binary handle holds Binary nodes only";

// nmn_hnsw.hip
nmn_status refuse_binary(const nmn_hnsw* h, const char* entry, const char* why);
nmn_status check_cfg(const nmn_hnsw_config* c);
nmn_status create_handle(const nmn_hnsw_config* cfg, int storage, uint32_t dim, uint64_t capacity_hint, int32_t device, nmn_hnsw** out);
// nmn_hnsw_build.hip
nmn_status canonicalise_sparse(uint32_t dim, const uint64_t* indptr, const uint32_t* positions, const float* values, uint32_t nq,
                               SparseQueries* out);
nmn_status wait_in_flight(nmn_hnsw* h);
// nmn_sparse_canon.hip (docs/hnsw.md §22).  The canonicaliser: three launches on s over a CSR in DEVICE memory, max_nnz already
// resolved by sparse_max_nnz; entries_dev holds nnz_total (position, value bits) pairs; dup_dev / dense_dev nullable; refuse_dup: a
// query with a duplicated position gets status 3 and is canonicalised as the entry-less query like every other status.
nmn_status launch_sparse_canon(uint32_t dim, const uint64_t* indptr_dev, const uint32_t* positions_dev, const float* values_dev,
                               uint32_t nq, uint64_t nnz_total, uint32_t max_nnz, bool refuse_dup, uint64_t* off_dev, uint32_t* entries_dev,
                               float* mag_dev, uint32_t* dup_dev, float* dense_dev, uint32_t* status_dev, hipStream_t s);
// One launch: the rows [k] of the queries whose status is not 0 become count 0, ids UINT64_MAX, scores -inf.
nmn_status launch_sparse_status_rows(const uint32_t* status_dev, uint32_t nq, uint32_t k, uint64_t* ids_dev, float* scores_dev,
                                     uint32_t* counts_dev, hipStream_t s);
// max_nnz as the entries take it: above kSparseLdsEntries NMN_ERR_INVALID_ARGUMENT, 0 = min(dim, kSparseLdsEntries)
nmn_status sparse_max_nnz(uint32_t dim, uint32_t max_nnz, uint32_t* out);
nmn_status upload_graph(nmn_hnsw* h, size_t reserve_n = 0, uint32_t reserve_upper = 0, uint32_t layers = 0);
nmn_status upload_codes(nmn_hnsw* h, uint64_t first, uint64_t count);
nmn_status alloc_codes(nmn_hnsw* h, uint64_t cap, uint64_t have);
nmn_status insert_rows(nmn_hnsw* h, const float* rows_host, uint64_t n, const SparseQueries* sp, const int64_t* sp_row,
                       uint64_t* ids_out, bool bulk = false, const TTBatch* tt = nullptr, const float* tt_norms = nullptr);

}  // namespace hnsw

namespace {

struct HostVisited {
    std::vector<uint32_t> stamp;
    uint32_t epoch = 0;
    void begin(size_t n) {
        if (stamp.size() < n) stamp.resize(n, 0);
        if (++epoch == 0) {
            std::fill(stamp.begin(), stamp.end(), 0);
            epoch = 1;
        }
    }
    bool insert(uint32_t id) {
        if (stamp[id] == epoch) return false;
        stamp[id] = epoch;
        return true;
    }
};

inline SearchArgs graph_args(const nmn_hnsw* h, uint32_t n) {
    SearchArgs a{};
    a.g.corpus = h->vectors ? h->vectors->corpus : nullptr;
    a.g.norms = !h->tt_nodes.empty() ? (const float*)h->d_wnorms.p : h->vectors ? h->vectors->norms : nullptr;
    a.g.l0 = (const uint32_t*)h->d_l0.p;
    a.g.l0cnt = (const uint32_t*)h->d_l0cnt.p;
    a.g.up_idx = (const uint32_t*)h->d_upidx.p;
    a.g.up = (const uint32_t*)h->d_up.p;
    a.g.upcnt = (const uint32_t*)h->d_upcnt.p;
    a.g.ld = h->vectors ? h->vectors->ld : 0;
    a.g.codes = (const uint8_t*)h->d_codes;
    a.g.rec = (const float4*)h->d_rec;
    a.g.ld8 = h->ld8;
    a.g.dim = h->dim;
    a.g.m = h->cfg.m;
    a.g.m0 = h->cfg.m0;
    a.g.up_layers = h->up_layers;
    a.g.n = n;
    a.g.entry = n ? (uint32_t)h->entry : kNone;
    a.g.max_layer = h->max_layer;
    a.g.metric = h->cfg.distance_metric;
    return a;
}

inline uint32_t results_need(uint32_t ef_eff, uint32_t n) { return std::min<uint32_t>(ef_eff, std::max<uint32_t>(n, 1)) + 1; }

}  // namespace
}  // namespace nmn
