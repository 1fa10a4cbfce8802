// nmn_hnsw.hip — `tensor_store::HNSWIndex` (tensor_store/src/hnsw.rs:1554-2335) with Dense storage: the graph is built on the
// host in the reference's order and searched on the GPU, one query per wave, the whole walk in one launch.
// THIS TRANSLATION UNIT IS BUILT WITH -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt (build.py), host and device:
// every distance of the index restates the reference's unfused f32 arithmetic and must give its bits.
//
// This file: the handle's life and accessors, the launch code (enqueue_walk_locked), the coalesced host search (run_batch) and every
// search, cache, mask and TT entry point.  Beside it (docs/hnsw.md, "Source layout"), all built with the same two flags:
//   nmn_hnsw_arith.h        constants, the two heaps, the host's reference arithmetic — what host and device both use
//   nmn_hnsw_kernels.h/.hip the kernels' arguments; the device distances, the three kernels and their launchers
//   nmn_hnsw_handle.h       struct nmn_hnsw, and the declarations (namespace nmn::hnsw) of what crosses files
//   nmn_hnsw_host.h         the host's distances to a node and the walk templates that build and search both instantiate
//   nmn_hnsw_build.hip      the host insert, the uploads, the bulk build, the insert entry points
//   nmn_hnsw_file.hip       save, load
//   nmn_sparse_canon.hip    sparse queries in device memory canonicalised on the GPU (free of the handle, like nmn_tt.hip)
//
// Reference order restated here (docs/hnsw.md has the long form):
//   simd::dot_product / sum_of_squares / euclidean_distance (hnsw.rs:168-261): eight accumulator chains over whole chunks of
//       eight elements (acc starts +0.0, product and sum rounded separately), the chains summed left to right from -0.0
//       (`arr.iter().sum()`), the scalar tail added after that, one sqrt.
//   distance_dense (hnsw.rs:1035-1045, 1084-1086, 1136-1138, 1157-1163): 1 - dot / (|v| |q|) (1.0 when a magnitude is 0),
//       euclidean_distance, -dot.  The pruning side (hnsw.rs:2437-2452 and siblings) is the same arithmetic on two rows.
//   Neighbor / MaxNeighbor (hnsw.rs:1380-1430) order by distance alone, so every tie is decided by the array layout of
//       std::collections::BinaryHeap: push = append + sift up from the new slot until a parent is not smaller; pop = last element
//       into the root, the hole sifted down to the bottom following the greater child (the right one when equal: the test is
//       `left <= right`), then sifted up; into_iter = the backing vector's order.  Both heaps are kept as that array algorithm.
//   search_layer (hnsw.rs:2276-2335), search_layer_greedy (2170-2200), search_with_ef (2069-2111), try_insert_embedding
//       (1936-2051), random_level (1631-1651).
//   HNSWStorageStrategy::Quantized (nmn_hnsw_create_with_storage): every row is a ScalarQuantizedVector (hnsw.rs:308-541).  The
//       query side (search_layer* at search AND insert time) is dot_dense / squared_magnitude / euclidean_distance_dense on the
//       codes, closed by one fused multiply-add each (`mul_add` = fmaf, the only fused operations of this file); the pruning
//       side (the (Quantized, Quantized) arms, 2489-2500, 2585-2589, 2662-2666) is the dense arithmetic on the dequantized rows,
//       which the host keeps where a dense handle keeps its rows.  The two sides differ in bits; both are restated.
//   nmn_hnsw_search_metric* (the end of this file): the walk with k = c, then the re-rank of its candidates under an extended
//       metric and their stable ordering (nmn_xmetric.hip) — VectorEngine::search_with_hnsw_and_metric, vector_engine/src/lib.rs:2560-2619.
//   nmn_hnsw_search_sparse: search_sparse_with_ef (hnsw.rs:2118-2166) — the same walk with distance_sparse (1175-1181).  The query
//       is a SparseVector as try_from_parts makes it (sparse_vector.rs:155-193); on a dense handle Cosine / DotProduct score a row
//       with dot_dense (450-466), ONE sequential f64 sum over the query's stored entries (each product exact in f64, each add
//       rounded once, one cast; std's float Sum restated as a left-to-right fold from -0.0), and Cosine takes magnitude() (548-559)
//       through f64; Euclidean, and every metric's dot on a quantized handle, go through to_dense() (400-406).  docs/hnsw.md §13.
//   nmn_hnsw_search_sparse_multi: the same with a k and an ef per query; both ride the request coalescer, a query kind per slot (§14).
//   nmn_hnsw_search_sparse_device / nmn_hnsw_cache_search_sparse_device: the CSR in DEVICE memory, made SparseVectors by
//       nmn_sparse_canon.hip on the caller's stream, then the same walk (and §16's re-rank) with nothing read back.  docs/hnsw.md §22.
//   nmn_hnsw_insert_sparse / nmn_hnsw_insert_auto (hnsw.rs:1660-1680): EmbeddingStorage::Sparse nodes beside Dense ones on a dense
//       handle.  A sparse node is scored by SparseVector's own arithmetic — dot_dense / dot / magnitude / euclidean_distance /
//       cosine_similarity / cosine_distance_dense, f64 chains over the stored entries — on the query side and on the pruning side;
//       the host keeps a kind per node, the kernel a record per node and takes the MIX instantiations.  docs/hnsw.md §15.
//   nmn_hnsw_search_tt / nmn_hnsw_search_tt_device (hnsw.rs:1811-1903, 2238-2272): search_tt_with_ef — the same walk with
//       cosine_distance_tt_with_norm (1196-1221): the query reconstructed and its tt_norm taken by nmn_tt.hip, then Cosine on every
//       handle with that norm as the query's magnitude, the kernel's kind 2.  nmn_hnsw_insert_tt: insert_tt_vector (1755-1759).
//       docs/hnsw.md §17.
//   nmn_hnsw_create_binary: every node is EmbeddingStorage::Binary(BinaryVector::from_dense(v, threshold)) (hnsw.rs:579,
//       binary_quantization.rs:83-99).  The query side is the dense arithmetic on to_dense() — +1.0 for a set bit, -1.0 otherwise
//       (157-166) — with sqrt(dim as f32) as the row's magnitude (hnsw.rs:801-805, 981-984, 1098-1101); the pruning side under
//       Cosine is 1 - similarity() = 1 - (1 - hamming / dim) on the words (2516-2518, binary_quantization.rs:137-142), under
//       Euclidean / DotProduct the dense arithmetic on both to_dense() rows (2605-2609, 2680-2684).  The host keeps the words and
//       the +-1 row per node, the device the words alone; the kernel takes the BIN instantiations.  docs/hnsw.md §18.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "nmn_hnsw_host.h"
#include "nmn_tt.h"

#pragma clang fp contract(off)

using namespace nmn;
using namespace nmn::hnsw;

namespace {

void host_search_one(const nmn_hnsw* h, const float* q, uint32_t k, uint64_t ef, HostVisited& vis, uint64_t* ids, float* scores,
                     uint32_t* count, uint64_t* evals) {
    const HQ qmag = host_query(h, q);
    host_walk_one(h, [&](uint32_t node) { return node_distance(h, node, q, qmag); }, k, ef, vis, ids, scores, count, evals);
}

// ---- SparseVector queries (sparse_vector.rs:155-193, 400-406, 450-466, 548-559; docs/hnsw.md §13) --------------------------------
// dot_dense and magnitude are h_sparse_dot / h_sparse_mag above.

// How a sparse call is served (docs/hnsw.md §13): distance_sparse is the DENSE walk of Q.to_dense() under Euclidean on either
// handle and under DotProduct on a quantized one; under Cosine on a quantized handle it is that walk with Q.magnitude() as the
// query's magnitude; under Cosine / DotProduct on a dense handle it is dot_dense over the stored entries.
enum SparseRoute { kSparseDensify = 0, kSparseGather = 1, kSparseDensifyMag = 2 };  // (the kernel's QK)
SparseRoute sparse_route(const nmn_hnsw* h) {
    const bool q8 = h->storage == NMN_HNSW_STORAGE_QUANTIZED;
    if (h->cfg.distance_metric == NMN_METRIC_EUCLIDEAN) return kSparseDensify;
    if (!q8) return kSparseGather;
    return h->cfg.distance_metric == NMN_METRIC_COSINE ? kSparseDensifyMag : kSparseDensify;
}

// search_sparse_with_ef of query q on the host: the walk of host_search_one with distance_sparse (hnsw.rs:1175-1181)
void host_search_one_sparse(const nmn_hnsw* h, const SparseQueries& sq, uint32_t q, uint32_t k, uint64_t ef, HostVisited& vis,
                            uint64_t* ids, float* scores, uint32_t* count, uint64_t* evals) {
    const SparseRoute route = sparse_route(h);
    if (route == kSparseGather) {
        const uint32_t* pos = sq.pos.data() + sq.off[q];
        const float* val = sq.val.data() + sq.off[q];
        const uint64_t nnz = sq.nnz(q);
        const float qmag = sq.mag[q];
        const int metric = h->cfg.distance_metric;
        const SpView Q{pos, val, nnz};
        const auto dist = [&](uint32_t node) -> float {
            if (node_is_sparse(h, node)) return sparse_node_sparse_query(h, node, Q, qmag);
            const float dot = h_sparse_dot(pos, val, nnz, h->rows.data() + (size_t)node * h->dim);
            if (metric == NMN_METRIC_DOT_PRODUCT) return -dot;
            const float vmag = h->mags[node];
            if (vmag == 0.0f || qmag == 0.0f) return 1.0f;
            const float den = vmag * qmag;
            const float sim = dot / den;
            return 1.0f - sim;
        };
        host_walk_one(h, dist, k, ef, vis, ids, scores, count, evals);
        return;
    }
    std::vector<float> dense(h->dim);
    sq.to_dense(q, h->dim, dense.data());
    HQ hq = host_query(h, dense.data());
    if (route == kSparseDensifyMag) hq.mag = sq.mag[q];
    const float* dq = dense.data();
    if (h->n_sparse && h->cfg.distance_metric == NMN_METRIC_EUCLIDEAN) {  // a Sparse node: s.euclidean_distance(Q), the union merge
        const SpView Q{sq.pos.data() + sq.off[q], sq.val.data() + sq.off[q], sq.nnz(q)};
        const auto dist = [&](uint32_t node) {
            return node_is_sparse(h, node) ? sparse_node_sparse_query(h, node, Q, 0.0f) : node_distance(h, node, dq, hq);
        };
        host_walk_one(h, dist, k, ef, vis, ids, scores, count, evals);
        return;
    }
    host_walk_one(h, [&](uint32_t node) { return node_distance(h, node, dq, hq); }, k, ef, vis, ids, scores, count, evals);
}

// A sparse query the device does not walk on a handle with Sparse nodes (docs/hnsw.md §15): under Euclidean (the union merge), and
// when the query or any Sparse node holds a duplicated position (dot_f64's merge is a lookup only without them).  The host answers.
bool sparse_query_host_only(const nmn_hnsw* h, const SparseQueries& sq, uint32_t q) {
    if (!h->n_sparse) return false;
    return h->cfg.distance_metric == NMN_METRIC_EUCLIDEAN || h->n_sparse_dup > 0 || sq.dup[q] != 0;
}

nmn_status record_search(nmn_hnsw* h, hipStream_t s) {
    std::lock_guard<std::mutex> lk(h->dev_mu);
    for (size_t i = 0; i < h->ev_pending.size();) {
        if (hipEventQuery(h->ev_pending[i]) == hipSuccess) {
            h->ev_free.push_back(h->ev_pending[i]);
            h->ev_pending[i] = h->ev_pending.back();
            h->ev_pending.pop_back();
        } else {
            i++;
        }
    }
    (void)hipGetLastError();
    hipEvent_t e = nullptr;
    if (!h->ev_free.empty()) {
        e = h->ev_free.back();
        h->ev_free.pop_back();
    } else {
        HN_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    const hipError_t he = hipEventRecord(e, s);
    if (he != hipSuccess) {
        h->ev_free.push_back(e);
        return set_error_hip(he, "nmn_hnsw_search_device");
    }
    h->ev_pending.push_back(e);
    return NMN_OK;
}

// The scratch of stream s (created on first use).
nmn_hnsw::Scratch* scratch_of(nmn_hnsw* h, hipStream_t s) {
    std::lock_guard<std::mutex> lk(h->dev_mu);
    for (auto& x : h->scratch)
        if (x->stream == s) return x.get();
    h->scratch.push_back(std::make_unique<nmn_hnsw::Scratch>());
    h->scratch.back()->stream = s;
    return h->scratch.back().get();
}

// What one call of enqueue_walk_locked walks with.  Uniform (qk == qef == nullptr): k and ef (= max(ef, k) already) for every query.
// Per query: DEVICE arrays qk / qef, rows of the outputs kstride apart.  Either way the caller has ORDERED the queries: the first
// n_lds are those whose results heap fits LDS (min(ef_q, n) + 1 <= the LDS limit + 1), the others go straight to the spill launch,
// so no launch mixes queries that would take different first launches.  rcap_lds / ef_lds: the largest results heap and the
// largest ef among the first n_lds; rcap_all: the largest results heap of all.
struct WalkShape {
    uint32_t k = 0, ef = 0;
    const uint32_t* qk = nullptr;
    const uint32_t* qef = nullptr;
    uint32_t kstride = 0, n_lds = 0, rcap_lds = 0, ef_lds = 0, rcap_all = 0;
    // the query kind of hnsw_search_kernel.  1 (uniform launches): no dense queries — DEVICE arrays sp_off [nq + 1] / sp_ent,
    // sp_max = the largest entry count of the call; 1 and 2 (uniform launches): DEVICE array qmag [nq].  3 (per-query launches): all
    // of these, and DEVICE arrays qkinds / qccap [nq], the kind of every query and its own candidate limit.
    int qkind = 0;
    const uint64_t* sp_off = nullptr;
    const uint2* sp_ent = nullptr;
    const float* qmag = nullptr;
    uint32_t sp_max = 0;
    const uint32_t* qkinds = nullptr;
    const uint32_t* qccap = nullptr;
    bool sp_only = false;  // qkind 3: every query is kind 1, so the query region need not hold a dense query
    // TT queries (docs/hnsw.md §17): the launch scores under Cosine whatever the handle's metric is (cosine_distance_tt_with_norm)
    bool cosine = false;
    // TT queries on a handle with TensorTrain nodes (docs/hnsw.md §24): the call's trains in DEVICE memory, the TTN launches
    const struct TTWalkQueries* tt = nullptr;
};

// The trains of one TT-query call as the TTN launches read them (SearchArgs' ttq_* fields): ranks_dev [nq][n_cores + 1] or null
// (ranks_u for every query), off_dev [nq + 1] or null (query i at i * stride); max_rank / max_storage over the call's queries.
struct TTWalkQueries {
    const float* cores_dev = nullptr;
    const uint32_t* ranks_dev = nullptr;
    const uint64_t* off_dev = nullptr;
    uint64_t stride = 0;
    uint32_t n_cores = 0, max_rank = 1, max_storage = 0;
    uint32_t shape[kTTMaxCores] = {};
    uint32_t ranks_u[kTTMaxCores + 1] = {};
};

// The LDS a TTN launch has (docs/hnsw.md §24): the query region, the stage and ctrl, the TT region — the query's ranks and cores
// and two Gram buffers of (largest node rank x largest query rank) floats — and both heaps, 64 KiB in all.  The candidate heap
// takes what is left (no answer depends on its size); a call is walked on the device when at least kTTWalkMinCand entries are.
constexpr uint32_t kTTWalkMinCand = 64;
constexpr size_t kWalkLdsBytes = 64 * 1024;
inline size_t walk_fixed_bytes(uint32_t qlds) { return (size_t)qlds * 4 + 32 * 4 + 32 * 4 + 4 * 4; }
// floats left for (query cores + 2 x node rank x query rank) in a launch of this handle with `ef`; 0: nothing fits
uint32_t tt_walk_lds_floats(const nmn_hnsw* h, uint32_t ef_eff) {
    const uint32_t n = (uint32_t)h->level.size(), dim8 = (h->dim + 7u) & ~7u;
    const uint32_t rmax = h->lds_rcap ? h->lds_rcap : kLdsResultsMax;
    const bool in_lds = n == 0 || results_need(ef_eff, n) <= rmax + 1;  // (results_fit_lds: otherwise the spill launch alone walks)
    const size_t used = walk_fixed_bytes(dim8) + 16 * 4 + 4 * 4 + (in_lds ? ((size_t)results_need(ef_eff, n) + kTTWalkMinCand) * sizeof(Ent) : 0);
    return used >= kWalkLdsBytes ? 0u : (uint32_t)((kWalkLdsBytes - used) / 4);
}
// whether the TTN launches serve a call with these trains on this handle
bool tt_walk_on_device(const nmn_hnsw* h, uint32_t ef_eff, uint32_t q_max_rank, uint64_t q_max_storage) {
    if (h->n_tt_big) return false;  // a node above nmn_tt_limits
    const uint64_t need = q_max_storage + 2ull * h->tt_max_rank * q_max_rank;
    return need <= tt_walk_lds_floats(h, ef_eff);
}

bool results_fit_lds(const nmn_hnsw* h, uint32_t ef_eff, uint32_t n) {
    const uint32_t rmax = h->lds_rcap ? h->lds_rcap : kLdsResultsMax;
    return n == 0 || results_need(ef_eff, n) <= rmax + 1;
}

// Enqueue the walk of nq queries (device buffers) on s.  Caller holds rw (shared) AND sc->mu, sc being scratch_of(h, s): growing
// the scratch, the fills and the launches of one call are one unit, two callers on one stream never interleave.
nmn_status enqueue_walk_locked(nmn_hnsw* h, nmn_hnsw::Scratch* sc, const float* q_dev, uint32_t nq, const WalkShape& w,
                               uint64_t* o_ids, float* o_sc, uint32_t* o_cnt, hipStream_t s) {
    const uint32_t n = (uint32_t)h->level.size();
    const bool perq = w.qk || w.qef;
    const uint32_t kstride = perq ? w.kstride : w.k;
    const uint32_t vwords = std::max<uint32_t>((n + 31) / 32, 1);
    const uint32_t chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nq, (256ull << 20) / ((uint64_t)vwords * 4)));
    // heaps of the first launch (LDS) and of the spill launch (global memory)
    // floats of the query region: the dense query padded to 8, or the stored entries of the longest sparse query, 2 floats each
    // (kSparseLdsEntries at most: no more than a dense query of 8192 dimensions, so cand_cap's rule for long queries carries over
    // with the region's length in place of the dimension)
    // (a launch with a kind per query holds either: the longer of the two — of the entries alone when no query of it is dense, so
    // that a call of kind-1 queries only keeps the region, and with it the candidate limit, it has as a QK = 1 launch)
    const uint32_t dim8 = (h->dim + 7u) & ~7u;
    const uint32_t qlds = w.qkind == 1 || (w.qkind == 3 && w.sp_only) ? std::max<uint32_t>(2u * w.sp_max, 2u)
                          : w.qkind == 3                              ? std::max<uint32_t>(dim8, 2u * w.sp_max)
                                                                      : dim8;
    uint32_t ccap = cand_cap(w.ef_lds, h->lds_ccap, w.qkind == 1 || w.qkind == 3 ? qlds : h->dim, n);
    const uint32_t s_rcap = w.rcap_all, s_ccap = std::max<uint32_t>(n, 1);
    const uint64_t region = (uint64_t)s_rcap + s_ccap;
    const uint32_t regions = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint32_t>(chunk, 64), (256ull << 20) / (region * sizeof(Ent))));
    bool synced = false;
    HN_TRY(grow(sc->vis, (size_t)chunk * vwords * 4, s, &synced));
    HN_TRY(grow(sc->flags, (size_t)nq * 4, s, &synced));
    HN_TRY(grow(sc->evals, (size_t)nq * 4, s, &synced));
    HN_TRY(grow(sc->spill, (size_t)regions * region * sizeof(Ent), s, &synced));
    SearchArgs a = graph_args(h, n);
    const bool q8 = h->storage == NMN_HNSW_STORAGE_QUANTIZED, bin = h->storage == NMN_HNSW_STORAGE_BINARY;
    if (bin && w.qkind != 0) return set_error(NMN_ERR_CONFIGURATION, "HNSW: a Binary-storage handle walks dense queries only");
    a.k = w.k;
    a.ef = w.ef;
    a.kstride = kstride;
    a.ccap_fixed = h->lds_ccap;
    a.qlds = qlds;
    a.vwords = vwords;
    a.visited = (uint32_t*)sc->vis.p;
    a.spill = (Ent*)sc->spill.p;
    // Sparse nodes are scored by their own arithmetic under Cosine / DotProduct only (Euclidean is the dense arithmetic on the rows)
    const int metric = w.cosine ? NMN_METRIC_COSINE : h->cfg.distance_metric;
    a.g.metric = metric;
    const bool mix = !q8 && !bin && h->n_sparse > 0 && metric != NMN_METRIC_EUCLIDEAN;
    a.nrec = mix ? (const uint4*)h->d_nrec.p : nullptr;
    a.nent = mix ? (const uint2*)h->d_nent.p : nullptr;
    a.kind_u = w.qkind == 3 ? 0u : (uint32_t)w.qkind;
    const bool ttn = w.tt != nullptr;
    size_t tt_bytes = 0;
    if (ttn) {  // the caller checked tt_walk_on_device: the TT region and kTTWalkMinCand candidates fit beside the results heap
        a.tt_slot = (const uint32_t*)h->d_ttslot.p;
        a.tt_rec = (const TTNodeDev*)h->d_ttrec.p;
        a.tt_cores = (const float*)h->d_ttcores.p;
        a.tt_pool = h->tt_cores.size();
        a.ttq_ncores = w.tt->n_cores;
        a.ttq_cap = w.tt->max_storage;
        a.tt_gcap = std::max<uint32_t>(h->tt_max_rank * w.tt->max_rank, 1);
        a.ttq_stride = w.tt->stride;
        memcpy(a.ttq_shape, w.tt->shape, sizeof a.ttq_shape);
        memcpy(a.ttq_ranks_u, w.tt->ranks_u, sizeof a.ttq_ranks_u);
        tt_bytes = (size_t)tt_region_floats(a.ttq_cap, a.tt_gcap) * 4;
        if (walk_fixed_bytes(qlds) + tt_bytes > kWalkLdsBytes)
            return set_error(NMN_ERR_INVALID_ARGUMENT, "HNSW: the query's train does not fit the walk's LDS");
        const size_t heaps = kWalkLdsBytes - walk_fixed_bytes(qlds) - tt_bytes;
        if (w.n_lds) {
            if (heaps < ((size_t)w.rcap_lds + 1) * sizeof(Ent))
                return set_error(NMN_ERR_INVALID_ARGUMENT, "HNSW: the TT region leaves no LDS for the heaps");
            ccap = std::min<uint32_t>(ccap, (uint32_t)(heaps / sizeof(Ent) - w.rcap_lds));
        }
    }
    for (uint32_t q0 = 0; q0 < nq; q0 += chunk) {
        const uint32_t nb = std::min<uint32_t>(chunk, nq - q0);
        const uint32_t nl = w.n_lds > q0 ? std::min<uint32_t>(w.n_lds - q0, nb) : 0;  // the chunk's queries that start in LDS: its first nl
        a.queries = q_dev ? q_dev + (size_t)q0 * h->dim : nullptr;
        a.sp_off = w.sp_off ? w.sp_off + q0 : nullptr;
        a.sp_ent = w.sp_ent;
        a.qmag = w.qmag ? w.qmag + q0 : nullptr;
        a.qkind = w.qkinds ? w.qkinds + q0 : nullptr;
        a.qccap = w.qccap ? w.qccap + q0 : nullptr;
        a.qk = w.qk ? w.qk + q0 : nullptr;
        a.qef = w.qef ? w.qef + q0 : nullptr;
        a.flags = (uint32_t*)sc->flags.p + q0;
        a.evals = (uint32_t*)sc->evals.p + q0;
        a.out_ids = o_ids + (size_t)q0 * kstride;
        a.out_scores = o_sc + (size_t)q0 * kstride;
        a.out_counts = o_cnt + q0;
        if (ttn) {
            a.ttq_ranks = w.tt->ranks_dev ? w.tt->ranks_dev + (size_t)q0 * (w.tt->n_cores + 1) : nullptr;
            a.ttq_off = w.tt->off_dev ? w.tt->off_dev + q0 : nullptr;
            a.ttq_cores = w.tt->off_dev ? w.tt->cores_dev : w.tt->cores_dev + (size_t)q0 * w.tt->stride;
        }
        HN_TRY(hipMemsetAsync(sc->vis.p, 0, (size_t)nb * vwords * 4, s));
        const size_t fixed = walk_fixed_bytes(qlds) + tt_bytes;
        if (nl) {
            HN_TRY(hipMemsetAsync(a.flags, 0, (size_t)nl * 4, s));
            a.nq = nl;
            a.rcap = w.rcap_lds;
            a.ccap = ccap;
            const size_t lds = fixed + ((size_t)a.rcap + a.ccap) * sizeof(Ent);
            launch_search(false, q8, bin, perq, w.qkind, mix, ttn, nl, lds, s, a);
            HN_TRY(hipGetLastError());
        }
        if (nl < nb)  // results heaps no wave can keep in LDS: these queries go straight to the spill launch
            HN_TRY(hipMemsetD32Async((hipDeviceptr_t)(a.flags + nl), 1, nb - nl, s));
        a.nq = nb;
        a.rcap = s_rcap;
        a.ccap = s_ccap;
        launch_search(true, q8, bin, perq, w.qkind, mix, ttn, std::min(regions, nb), fixed, s, a);
        HN_TRY(hipGetLastError());
    }
    return NMN_OK;
}

WalkShape uniform_shape(const nmn_hnsw* h, uint32_t nq, uint32_t k, uint32_t ef) {
    const uint32_t n = (uint32_t)h->level.size();
    WalkShape w;
    w.k = k;
    w.ef = std::max<uint32_t>(ef ? ef : h->cfg.ef_search, k);  // hnsw.rs:2102
    w.n_lds = results_fit_lds(h, w.ef, n) ? nq : 0;
    w.rcap_lds = w.rcap_all = results_need(w.ef, n);
    w.ef_lds = w.ef;
    return w;
}

// The same k and ef for every query: the walk as nmn_hnsw_search_device and nmn_hnsw_search_metric* enqueue it.
nmn_status enqueue_search_locked(nmn_hnsw* h, nmn_hnsw::Scratch* sc, const float* q_dev, uint32_t nq, uint32_t k, uint32_t ef,
                                 uint64_t* o_ids, float* o_sc, uint32_t* o_cnt, hipStream_t s) {
    return enqueue_walk_locked(h, sc, q_dev, nq, uniform_shape(h, nq, k, ef), o_ids, o_sc, o_cnt, s);
}

// The same for a caller that holds rw (shared) only.  *sc_out: the stream's scratch, whose flags / evals the host-buffer search
// reads back.
nmn_status enqueue_search(nmn_hnsw* h, const float* q_dev, uint32_t nq, uint32_t k, uint32_t ef, uint64_t* o_ids, float* o_sc,
                          uint32_t* o_cnt, hipStream_t s, nmn_hnsw::Scratch** sc_out) {
    nmn_hnsw::Scratch* sc = scratch_of(h, s);
    if (sc_out) *sc_out = sc;
    std::lock_guard<std::mutex> slk(sc->mu);
    return enqueue_search_locked(h, sc, q_dev, nq, k, ef, o_ids, o_sc, o_cnt, s);
}

}  // namespace

namespace nmn {
namespace hnsw {
// What a Binary-storage handle does not serve (docs/hnsw.md §18): refused before anything is written or enqueued.
nmn_status refuse_binary(const nmn_hnsw* h, const char* entry, const char* why) {
    if (h->storage != NMN_HNSW_STORAGE_BINARY) return NMN_OK;
    char buf[256];
    snprintf(buf, sizeof buf, "HNSW: %s is not served on a handle with Binary storage (%s)", entry, why);
    return set_error(NMN_ERR_CONFIGURATION, buf);
}
}  // namespace hnsw
}  // namespace nmn

namespace {

// search_with_hnsw_and_metric's candidate count (lib.rs:2578), served as min(c, len): search_layer runs with max(ef_search, c) and any
// ef >= len keeps every node the walk reaches (the rule nmn_engine_search_with_hnsw applies to k)
uint64_t metric_candidates(const nmn_hnsw* h, uint32_t top_k) {
    const uint64_t c = std::max<uint64_t>(2ull * top_k, 10);
    return std::min<uint64_t>(c, std::max<uint64_t>(h->level.size(), 1));
}

// CacheIndex::search_with_metric's candidate count (tensor_cache/src/index.rs:204): max(3k, 10) in 64 bits, served as min(c, len) like
// the one above (index.search(query, c) walks layer 0 with max(ef_search, c))
uint64_t cache_candidates(const nmn_hnsw* h, uint32_t top_k) {
    const uint64_t c = std::max<uint64_t>(3ull * top_k, 10);
    return std::min<uint64_t>(c, std::max<uint64_t>(h->level.size(), 1));
}

// What the re-rank and ordering of a cache call read of the handle (docs/hnsw.md §16).  Caller holds rw.
XmetricFilter cache_filter(const nmn_hnsw* h, float threshold) {
    XmetricFilter f;
    f.live = (const uint32_t*)h->d_live.p;
    f.threshold = threshold;
    if (h->n_sparse) {
        f.nrec = (const uint4*)h->d_nrec.p;
        f.nent = (const uint2*)h->d_nent.p;
    }
    return f;
}

// The candidate block of the stream's scratch grown for nq x c.  Caller holds rw (shared) and sc->mu, and keeps sc->mu until the
// last launch that reads the block is enqueued: the block belongs to ONE call at a time (another caller on the same stream would
// overwrite the candidates, or free the block under a launch being prepared).
nmn_status metric_scratch(nmn_hnsw::Scratch* sc, hipStream_t s, uint32_t nq, uint32_t c, uint32_t top_k, bool filtered = false) {
    bool synced = false;
    HN_TRY(grow(sc->xids, (size_t)nq * c * 8, s, &synced));
    HN_TRY(grow(sc->xsc, (size_t)nq * c * 4, s, &synced));
    HN_TRY(grow(sc->xsim, (size_t)nq * c * 4, s, &synced));
    HN_TRY(grow(sc->xcnt, (size_t)nq * 4, s, &synced));
    const size_t sort_bytes = xmetric_order_scratch_bytes(c, top_k, filtered);
    sc->xsort_use = sort_bytes != 0;
    HN_TRY(grow(sc->xsort, sort_bytes, s, &synced));
    return NMN_OK;
}

// The re-rank and the ordering of the candidate block in sc, behind whatever filled it on s.  Caller holds sc->mu.
nmn_status enqueue_rerank(nmn_hnsw* h, nmn_hnsw::Scratch* sc, const float* q_dev, uint32_t nq, uint32_t c, uint32_t top_k,
                          const nmn_xmetric& m, uint64_t* o_ids, float* o_sc, uint32_t* o_cnt, hipStream_t s,
                          const XmetricFilter* filter = nullptr) {
    HN_TRY(launch_xmetric_rerank(h->vectors ? h->vectors->corpus : nullptr, h->vectors ? h->vectors->ld : 0, h->dim, h->level.size(),
                                 q_dev, nq, c, (const uint64_t*)sc->xids.p, (const uint32_t*)sc->xcnt.p, m, top_k, (float*)sc->xsim.p,
                                 o_ids, o_sc, o_cnt, sc->xsort_use ? sc->xsort.p : nullptr, s, filter));
    return NMN_OK;
}

nmn_status check_metric_call(nmn_hnsw* h, uint32_t top_k, const nmn_xmetric* m) {
    if (!h || !m) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (!xmetric_valid(m)) return set_error(NMN_ERR_CONFIGURATION, "unknown extended distance metric");
    if (top_k == 0) return set_error(NMN_ERR_INVALID_TOP_K, "top_k == 0");
    if (const nmn_status sb = refuse_binary(h, "nmn_hnsw_search_metric", kBinNoRows); sb != NMN_OK) return sb;
    if (h->storage != NMN_HNSW_STORAGE_DENSE)
        return set_error(NMN_ERR_CONFIGURATION,
                         "HNSW: nmn_hnsw_search_metric re-ranks with the rows of nmn_hnsw_vectors(h), and a quantized handle keeps no f32 "
                         "rows on the device (re-rank the candidates of nmn_hnsw_search against your own vectors)");
    return NMN_OK;
}

}  // namespace

namespace nmn {
namespace hnsw {
nmn_status check_cfg(const nmn_hnsw_config* c) {
    if (c->storage != NMN_HNSW_STORAGE_DENSE)
        return set_error(NMN_ERR_CONFIGURATION, "HNSW: only HNSWStorageStrategy::Dense is served (Auto / Quantized are out of scope)");
    if (c->distance_metric < NMN_METRIC_COSINE || c->distance_metric > NMN_METRIC_DOT_PRODUCT)
        return set_error(NMN_ERR_CONFIGURATION, "HNSW: distance_metric must be Cosine, Euclidean or DotProduct");
    if (c->m == 0 || c->m0 == 0 || c->m > 4096 || c->m0 > 4096) return set_error(NMN_ERR_CONFIGURATION, "HNSW: m / m0 out of range");
    return NMN_OK;
}
}  // namespace hnsw
}  // namespace nmn

namespace {

void fill_cfg(nmn_hnsw_config* c, uint32_t m, uint32_t efc, uint32_t efs) {
    memset(c, 0, sizeof *c);
    c->m = m;
    c->m0 = 2 * m;
    c->ef_construction = efc;
    c->ef_search = efs;
    c->ml = 1.0 / std::log((double)m);
    c->sparsity_threshold = 0.5f;
    c->max_nodes = 10000000ull;
    c->distance_metric = NMN_METRIC_COSINE;
    c->storage = NMN_HNSW_STORAGE_DENSE;
}

bool host_search_forced() {
    const char* e = getenv("NMN_HNSW_HOST_SEARCH");
    return e && e[0] == '1';
}

}  // namespace

extern "C" void nmn_hnsw_config_default(nmn_hnsw_config* c) {
    if (c) fill_cfg(c, 16, 200, 50);
}
extern "C" void nmn_hnsw_config_high_recall(nmn_hnsw_config* c) {
    if (c) fill_cfg(c, 32, 400, 200);
}
extern "C" void nmn_hnsw_config_high_speed(nmn_hnsw_config* c) {
    if (c) fill_cfg(c, 8, 100, 20);
}

namespace nmn {
namespace hnsw {
nmn_status create_handle(const nmn_hnsw_config* cfg, int storage, uint32_t dim, uint64_t capacity_hint, int32_t device, nmn_hnsw** out) {
    if (dim == 0) return set_error(NMN_ERR_EMPTY_VECTOR, "dim == 0");
    if (dim > kMaxDim) return set_error(NMN_ERR_CONFIGURATION, "HNSW: dimension above 8192 (the query is kept in LDS)");
    nmn_status st = check_cfg(cfg);
    if (st != NMN_OK) return st;
    auto h = std::make_unique<nmn_hnsw>();
    h->cfg = *cfg;
    h->cfg.storage = storage;
    h->storage = storage;
    h->dim = dim;
    h->device = device;
    h->vec_cap = 0;
    const uint64_t cap_rows = cfg->max_nodes > 0 ? std::min<uint64_t>(std::max<uint64_t>(capacity_hint, 1), cfg->max_nodes)
                                                 : std::max<uint64_t>(capacity_hint, 1);
    if (storage != NMN_HNSW_STORAGE_DENSE) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
            (void)hipGetLastError();
            return set_error(NMN_ERR_NO_DEVICE, "no HIP device");
        }
        int dev = device;
        if (dev < 0) HN_TRY(hipGetDevice(&dev));
        if (dev >= ndev) return set_error(NMN_ERR_NO_DEVICE, "device ordinal out of range");
        HN_TRY(hipSetDevice(dev));
        h->device = dev;
        h->ld8 = (dim + 15u) & ~15u;
        if (storage == NMN_HNSW_STORAGE_BINARY) {
            h->bin_w = (dim + 63u) / 64u;
            h->ld8 = 16u * ((dim + 127u) / 128u);  // ldw = bin_w rounded up to 2 words: 16-byte rows
            h->sqrt_dim = sqrtf((float)dim);
        }
        st = alloc_codes(h.get(), cap_rows, 0);
        if (st != NMN_OK) {
            if (h->d_codes) (void)hipFree(h->d_codes);
            if (h->d_rec) (void)hipFree(h->d_rec);
            return st;
        }
    } else {
        // the flat index fixes the device (and fails with NMN_ERR_NO_DEVICE where there is none)
        const uint64_t cap0 = std::max<uint64_t>(capacity_hint, 1);
        h->vec_cap = 0;
        nmn_index_desc d{};
        d.dim = dim;
        d.capacity_rows = cfg->max_nodes > 0 ? std::min<uint64_t>(cap0, cfg->max_nodes) : cap0;
        d.device = device;
        st = nmn_index_create(&d, &h->vectors);
        if (st != NMN_OK) return st;
        h->vec_cap = d.capacity_rows;
        h->device = h->vectors->device;
    }
    hipError_t he = hipSetDevice(h->device);
    if (he == hipSuccess) he = hipStreamCreateWithFlags(&h->host_stream, hipStreamNonBlocking);
    if (he != hipSuccess) {
        if (h->vectors) nmn_index_destroy(h->vectors);
        if (h->d_codes) (void)hipFree(h->d_codes);
        if (h->d_rec) (void)hipFree(h->d_rec);
        return set_error_hip(he, "nmn_hnsw_create");
    }
    *out = h.release();
    return NMN_OK;
}
}  // namespace hnsw
}  // namespace nmn

extern "C" nmn_status nmn_hnsw_create(const nmn_hnsw_config* cfg, uint32_t dim, uint64_t capacity_hint, int32_t device, nmn_hnsw** out) {
    if (!cfg || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    return create_handle(cfg, NMN_HNSW_STORAGE_DENSE, dim, capacity_hint, device, out);
}

// HNSWBuildOptions' storage (vector_engine/src/lib.rs:853-858) applied to the index: cfg->storage is not read
extern "C" nmn_status nmn_hnsw_create_with_storage(const nmn_hnsw_config* cfg, int32_t storage, uint32_t dim, uint64_t capacity_hint,
                                                   int32_t device, nmn_hnsw** out) {
    if (!cfg || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (storage == NMN_HNSW_STORAGE_AUTO)
        return set_error(NMN_ERR_CONFIGURATION, "HNSW: HNSWStorageStrategy::Auto (sparse storage) is not served; Dense and Quantized are");
    if (storage != NMN_HNSW_STORAGE_DENSE && storage != NMN_HNSW_STORAGE_QUANTIZED && storage != NMN_HNSW_STORAGE_BINARY)
        return set_error(NMN_ERR_CONFIGURATION, "HNSW: unknown storage strategy");
    nmn_hnsw_config c = *cfg;
    c.storage = NMN_HNSW_STORAGE_DENSE;  // (the old field plays no part here)
    return create_handle(&c, storage, dim, capacity_hint, device, out);  // (Binary: BinaryThreshold::Sign)
}

// Every node EmbeddingStorage::Binary(BinaryVector::from_dense(row, threshold)), docs/hnsw.md §18
extern "C" nmn_status nmn_hnsw_create_binary(const nmn_hnsw_config* cfg, int32_t binary_threshold, uint32_t dim, uint64_t capacity_hint,
                                             int32_t device, nmn_hnsw** out) {
    if (!cfg || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    *out = nullptr;
    if (binary_threshold < NMN_BINARY_SIGN || binary_threshold > NMN_BINARY_MEDIAN)
        return set_error(NMN_ERR_CONFIGURATION, "HNSW: binary_threshold must be NMN_BINARY_SIGN, _MEAN or _MEDIAN");
    nmn_hnsw_config c = *cfg;
    c.storage = NMN_HNSW_STORAGE_DENSE;
    const nmn_status st = create_handle(&c, NMN_HNSW_STORAGE_BINARY, dim, capacity_hint, device, out);
    if (st == NMN_OK) (*out)->bin_method = binary_threshold;
    return st;
}

extern "C" nmn_status nmn_hnsw_destroy(nmn_hnsw* h) {
    if (!h) return NMN_OK;
    (void)hipSetDevice(h->device);
    {
        std::unique_lock<std::shared_mutex> g(h->rw);
        (void)wait_in_flight(h);
        if (h->host_stream) (void)hipStreamSynchronize(h->host_stream);
    }
    for (hipEvent_t e : h->ev_free) (void)hipEventDestroy(e);
    for (auto& s : h->scratch) {
        drop(s->vis);
        drop(s->flags);
        drop(s->evals);
        drop(s->spill);
        drop(s->xids);
        drop(s->xsc);
        drop(s->xcnt);
        drop(s->xsim);
        drop(s->xsort);
        drop(s->ttq);
        drop(s->ttmag);
        drop(s->ttkind);
        for (DevBuf* b : {&s->sq_off, &s->sq_ent, &s->sq_mag, &s->sq_dup, &s->sq_dense, &s->sq_status}) drop(*b);
    }
    for (DevBuf* b : {&h->d_l0, &h->d_l0cnt, &h->d_upidx, &h->d_up, &h->d_upcnt, &h->d_nrec, &h->d_nent, &h->d_wnorms, &h->d_ttslot, &h->d_ttrec, &h->d_ttcores, &h->d_live, &h->bk_lv, &h->bk_vis, &h->bk_out, &h->bk_patch, &h->hq, &h->hids, &h->hsc, &h->hcnt, &h->hkef,
                       &h->hsp_off, &h->hsp_ent, &h->hqmag,
                       &h->hxmeta, &h->hxsim, &h->hxoids, &h->hxosc, &h->hxocnt, &h->hxsort, &h->htt_cores, &h->htt_ranks, &h->htt_off,
                       &h->htt_skip})
        drop(*b);
    if (h->host_stream) (void)hipStreamDestroy(h->host_stream);
    if (h->vectors) nmn_index_destroy(h->vectors);
    if (h->d_codes) (void)hipFree(h->d_codes);
    if (h->d_rec) (void)hipFree(h->d_rec);
    delete h;
    return NMN_OK;
}

extern "C" uint64_t nmn_hnsw_len(const nmn_hnsw* h) { return h ? h->level.size() : 0; }
extern "C" uint32_t nmn_hnsw_dim(const nmn_hnsw* h) { return h ? h->dim : 0; }
extern "C" uint64_t nmn_hnsw_entry_point(const nmn_hnsw* h) { return h ? h->entry : ~0ull; }
extern "C" uint32_t nmn_hnsw_max_layer(const nmn_hnsw* h) { return h ? h->max_layer : 0; }
extern "C" nmn_index* nmn_hnsw_vectors(nmn_hnsw* h) { return h ? h->vectors : nullptr; }
extern "C" int32_t nmn_hnsw_storage(const nmn_hnsw* h) { return h ? h->storage : -1; }
extern "C" int32_t nmn_hnsw_binary_threshold(const nmn_hnsw* h) {
    return h && h->storage == NMN_HNSW_STORAGE_BINARY ? h->bin_method : -1;
}

extern "C" nmn_status nmn_hnsw_binary_row(nmn_hnsw* h, uint64_t node, uint64_t* words_out, uint32_t cap_words) {
    if (!h) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_lock<std::shared_mutex> g(h->rw);
    if (h->storage != NMN_HNSW_STORAGE_BINARY) return set_error(NMN_ERR_CONFIGURATION, "HNSW: the handle's storage is not Binary");
    if (node >= h->level.size()) return set_error(NMN_ERR_NOT_FOUND, "HNSW: no such node");
    if (!words_out) return NMN_OK;
    if (cap_words < h->bin_w) return set_error(NMN_ERR_BUFFER_TOO_SMALL, "nmn_hnsw_binary_row");
    memcpy(words_out, h->bwords.data() + node * h->bin_w, (size_t)h->bin_w * 8);
    return NMN_OK;
}

extern "C" nmn_status nmn_hnsw_quantized_row(nmn_hnsw* h, uint64_t node, uint8_t* codes_out, float* scale, float* min_val) {
    if (!h) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (const nmn_status sb = refuse_binary(h, "nmn_hnsw_quantized_row", "nmn_hnsw_binary_row returns its words"); sb != NMN_OK) return sb;
    std::shared_lock<std::shared_mutex> g(h->rw);
    if (h->storage != NMN_HNSW_STORAGE_QUANTIZED) return set_error(NMN_ERR_CONFIGURATION, "HNSW: the handle's storage is not Quantized");
    if (node >= h->level.size()) return set_error(NMN_ERR_NOT_FOUND, "HNSW: no such node");
    if (codes_out) memcpy(codes_out, h->codes.data() + node * h->dim, h->dim);
    if (scale) *scale = h->qscale[node];
    if (min_val) *min_val = h->qmin[node];
    return NMN_OK;
}

// HNSWIndex::get_vector: the row as stored (Dense), dequantize() (Quantized), to_dense() (Binary)
extern "C" nmn_status nmn_hnsw_get_vector(nmn_hnsw* h, uint64_t node, float* out) {
    if (!h || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_lock<std::shared_mutex> g(h->rw);
    if (node >= h->level.size()) return set_error(NMN_ERR_NOT_FOUND, "HNSW: no such node");
    memcpy(out, h->rows.data() + node * h->dim, (size_t)h->dim * 4);
    return NMN_OK;
}

// HNSWIndex::memory_stats, hnsw.rs:2733-2768: embedding.memory_bytes() is 4 dim (Dense, 1227) or 16 + dim (Quantized, 381-383)
extern "C" nmn_status nmn_hnsw_memory_stats(nmn_hnsw* h, nmn_hnsw_memstats* out) {
    if (!h || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_lock<std::shared_mutex> g(h->rw);
    memset(out, 0, sizeof *out);
    const uint64_t n = h->level.size();
    out->total_nodes = n;
    if (h->storage == NMN_HNSW_STORAGE_QUANTIZED) {
        out->quantized_count = n;
        out->embedding_bytes = n * (16ull + h->dim);
    } else if (h->storage == NMN_HNSW_STORAGE_BINARY) {  // BinaryVector::memory_bytes, binary_quantization.rs:174-179
        out->binary_count = n;
        out->embedding_bytes = n * 8ull * h->bin_w;
    } else {
        // a Sparse node: SparseVector::memory_bytes (sparse_vector.rs:1064-1068) = size_of::<SparseVector>() (56 on a 64-bit
        // target) + 4 capacity + 4 capacity, the capacities taken as the lengths (what a cloned vector has; docs/hnsw.md §15)
        // a TensorTrain node: 4 storage_size() (hnsw.rs:1230), the sum of its cores' lengths
        const uint64_t n_tt = h->tt_nodes.size();
        out->sparse_count = h->n_sparse;
        out->tt_count = n_tt;
        out->dense_count = n - h->n_sparse - n_tt;
        out->embedding_bytes = (n - h->n_sparse - n_tt) * 4ull * h->dim + h->n_sparse * 56ull + 8ull * h->sp_pos.size() + 4ull * h->tt_cores.size();
    }
    return NMN_OK;
}

extern "C" nmn_status nmn_hnsw_levels(nmn_hnsw* h, uint32_t* out, uint64_t cap) {
    if (!h || !out) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_lock<std::shared_mutex> g(h->rw);
    if (cap < h->level.size()) return set_error(NMN_ERR_BUFFER_TOO_SMALL, "nmn_hnsw_levels");
    for (size_t i = 0; i < h->level.size(); i++) out[i] = h->level[i];
    return NMN_OK;
}

extern "C" nmn_status nmn_hnsw_neighbors(nmn_hnsw* h, uint64_t node, uint32_t layer, uint64_t* out, uint32_t cap, uint32_t* count) {
    if (!h || !count) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_lock<std::shared_mutex> g(h->rw);
    if (node >= h->level.size()) return set_error(NMN_ERR_NOT_FOUND, "HNSW: no such node");
    if (layer > h->level[node]) {
        *count = 0;
        return NMN_OK;
    }
    const auto& l = h->nbr[node][layer];
    *count = (uint32_t)l.size();
    if (!out) return NMN_OK;
    if (cap < l.size()) return set_error(NMN_ERR_BUFFER_TOO_SMALL, "nmn_hnsw_neighbors");
    for (size_t i = 0; i < l.size(); i++) out[i] = l[i];
    return NMN_OK;
}

extern "C" nmn_status nmn_hnsw_set_heap_capacity(nmn_hnsw* h, uint32_t results, uint32_t candidates) {
    if (!h) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (results > kLdsResultsMax || candidates > kLdsCandMax) return set_error(NMN_ERR_INVALID_ARGUMENT, "HNSW: beyond the LDS heaps");
    std::unique_lock<std::shared_mutex> g(h->rw);
    h->lds_rcap = results;
    h->lds_ccap = candidates;
    return NMN_OK;
}

extern "C" uint64_t nmn_hnsw_hbm_bytes(nmn_hnsw* h) {
    if (!h) return 0;
    std::shared_lock<std::shared_mutex> g(h->rw);
    uint64_t t = h->d_l0.cap + h->d_l0cnt.cap + h->d_upidx.cap + h->d_up.cap + h->d_upcnt.cap + h->d_nrec.cap + h->d_nent.cap + h->d_live.cap;
    t += h->d_wnorms.cap + h->d_ttslot.cap + h->d_ttrec.cap + h->d_ttcores.cap;  // (a handle with TensorTrain nodes, docs/hnsw.md §24)
    t += h->bk_lv.cap + h->bk_vis.cap + h->bk_out.cap + h->bk_patch.cap;  // (what nmn_hnsw_insert_bulk keeps between calls)
    uint64_t a = 0, b = 0, c = 0;
    if (h->vectors && nmn_index_hbm_bytes(h->vectors, &a, &b, &c) == NMN_OK) t += a + b + c;
    if (h->d_codes) t += std::max<uint64_t>(h->vec_cap * h->ld8, 256);
    if (h->d_rec) t += std::max<uint64_t>(h->vec_cap * 16, 256);
    return t;
}

extern "C" nmn_status nmn_hnsw_search_device(nmn_hnsw* h, const float* queries_dev, uint32_t nq, uint32_t k, uint32_t ef,
                                             uint64_t* out_ids_dev, float* out_scores_dev, uint32_t* out_counts_dev, void* stream) {
    if (!h) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (k == 0) return set_error(NMN_ERR_INVALID_TOP_K, "k == 0");
    if (nq == 0) return NMN_OK;
    if (!queries_dev || !out_ids_dev || !out_scores_dev || !out_counts_dev) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_lock<std::shared_mutex> g(h->rw);
    HN_TRY(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    nmn_status st = enqueue_search(h, queries_dev, nq, k, ef, out_ids_dev, out_scores_dev, out_counts_dev, s, nullptr);
    if (st != NMN_OK) return st;
    return record_search(h, s);
}

// ---- the host-buffer walk: batches, and the coalescer in front of them (docs/hnsw.md §11) ----------------------------------------
namespace {

bool hnsw_coalesce_enabled() {
    static const bool on = [] {
        const char* e = getenv("NMN_HNSW_NO_COALESCE");
        return !(e && e[0] && e[0] != '0');
    }();
    return on;
}

void pad_row(uint64_t* ids, float* sc, uint32_t from, uint32_t to) {
    for (uint32_t i = from; i < to; i++) {
        ids[i] = ~0ull;
        sc[i] = -INFINITY;
    }
}

struct Slot {
    HostWalk* r;
    uint32_t i, k, ef;       // what the query walks with (a metric query: k = its candidate count c, ef = max(ef_search, c))
    uint32_t top;            // a metric query's top_k
    const nmn_xmetric* xm;   // ... and its metric (nullptr: a plain walk)
    uint32_t kind;           // the kernel's query kind: sparse_route for a query of a sparse call, 0 for every other
    bool filt = false;       // a cache query (docs/hnsw.md §16): k is the 3k rule's count, the ordering is the filtered one ...
    float thr = 0.0f;        // ... with this threshold
};

// The answer of a uniform batch, as it sits in hids / hsc / hcnt: the rows of every caller, `stride` apart, to its own buffers
nmn_status hand_out_rows(nmn_hnsw* h, const std::vector<HostWalk*>& batch, uint32_t stride, hipStream_t s) {
    uint32_t o = 0;
    for (const HostWalk* r : batch) {
        HN_TRY(hipMemcpyAsync(r->out_ids, (uint64_t*)h->hids.p + (size_t)o * stride, (size_t)r->nq * stride * 8, hipMemcpyDeviceToHost, s));
        HN_TRY(hipMemcpyAsync(r->out_scores, (float*)h->hsc.p + (size_t)o * stride, (size_t)r->nq * stride * 4, hipMemcpyDeviceToHost, s));
        HN_TRY(hipMemcpyAsync(r->out_counts, (uint32_t*)h->hcnt.p + o, (size_t)r->nq * 4, hipMemcpyDeviceToHost, s));
        o += r->nq;
    }
    return NMN_OK;
}

// A batch whose slots are all metric slots with one top_k and one metric (a lone nmn_hnsw_search_metric is one): the uniform chain
// it has always been — the walk into the stream's candidate block, xmetric_rerank_kernel, the ordering — straight between the
// callers' buffers and the device.  Caller holds rw (shared) and host_mu.  on_host: the walk on the host (NMN_HNSW_HOST_SEARCH=1).
nmn_status run_metric_uniform(nmn_hnsw* h, const std::vector<HostWalk*>& batch, const std::vector<Slot>& slot, bool on_host) {
    const uint32_t N = (uint32_t)slot.size(), dim = h->dim, top_k = slot[0].top, c = slot[0].k;
    const nmn_xmetric& metric = *slot[0].xm;
    const XmetricFilter flt = cache_filter(h, slot[0].thr);
    const XmetricFilter* filter = slot[0].filt ? &flt : nullptr;
    hipStream_t s = h->host_stream;
    bool synced = true;  // (every earlier host call ended with a wait)
    const hipStream_t none = (hipStream_t)-1;
    HN_TRY(grow(h->hq, (size_t)N * dim * 4, none, &synced));
    HN_TRY(grow(h->hids, (size_t)N * top_k * 8, none, &synced));
    HN_TRY(grow(h->hsc, (size_t)N * top_k * 4, none, &synced));
    HN_TRY(grow(h->hcnt, (size_t)N * 4, none, &synced));
    // host_mu makes this batch the only one on host_stream; sc->mu is held all the same, for the whole batch: the candidate block
    // is read back and, should a query stay flagged, filled again
    nmn_hnsw::Scratch* sc = scratch_of(h, s);
    std::lock_guard<std::mutex> slk(sc->mu);
    nmn_status st = metric_scratch(sc, s, N, c, top_k, filter != nullptr);
    if (st != NMN_OK) return st;
    uint32_t off = 0;
    for (const HostWalk* r : batch) {
        HN_TRY(hipMemcpyAsync((float*)h->hq.p + (size_t)off * dim, r->q, (size_t)r->nq * dim * 4, hipMemcpyHostToDevice, s));
        off += r->nq;
    }
    std::vector<uint64_t> cid;
    std::vector<float> csc;
    std::vector<uint32_t> ccnt(N), fl(N, 0), ev(N, 0);
    auto host_walk = [&](uint32_t q) {  // the walk of query q on the host, its candidates into the staging vectors
        static thread_local HostVisited vis;
        if (cid.empty()) {
            cid.resize((size_t)N * c);
            csc.resize((size_t)N * c);
        }
        uint64_t e2 = 0;
        host_search_one(h, slot[q].r->q + (size_t)slot[q].i * dim, c, h->cfg.ef_search, vis, cid.data() + (size_t)q * c,
                        csc.data() + (size_t)q * c, &ccnt[q], &e2);
        ev[q] = (uint32_t)e2;
    };
    if (on_host) {
        for (uint32_t q = 0; q < N; q++) host_walk(q);
        HN_TRY(hipMemcpyAsync(sc->xids.p, cid.data(), (size_t)N * c * 8, hipMemcpyHostToDevice, s));
        HN_TRY(hipMemcpyAsync(sc->xcnt.p, ccnt.data(), (size_t)N * 4, hipMemcpyHostToDevice, s));
    } else {
        st = enqueue_search_locked(h, sc, (const float*)h->hq.p, N, c, 0, (uint64_t*)sc->xids.p, (float*)sc->xsc.p, (uint32_t*)sc->xcnt.p, s);
        if (st != NMN_OK) return st;
    }
    st = enqueue_rerank(h, sc, (const float*)h->hq.p, N, c, top_k, metric, (uint64_t*)h->hids.p, (float*)h->hsc.p, (uint32_t*)h->hcnt.p, s, filter);
    if (st != NMN_OK) return st;
    if ((st = hand_out_rows(h, batch, top_k, s)) != NMN_OK) return st;
    if (!on_host) {
        HN_TRY(hipMemcpyAsync(ccnt.data(), sc->xcnt.p, (size_t)N * 4, hipMemcpyDeviceToHost, s));
        HN_TRY(hipMemcpyAsync(fl.data(), sc->flags.p, (size_t)N * 4, hipMemcpyDeviceToHost, s));
        HN_TRY(hipMemcpyAsync(ev.data(), sc->evals.p, (size_t)N * 4, hipMemcpyDeviceToHost, s));
    }
    HN_TRY(hipStreamSynchronize(s));
    bool redo = false;
    for (uint32_t q = 0; q < N; q++)
        if (fl[q] == 1u) redo = true;  // the spill launch could not answer it (cannot happen while its heap holds n entries)
    if (redo) {  // ... then the host walks every such query and the device re-ranks again
        cid.resize((size_t)N * c);
        csc.resize((size_t)N * c);
        HN_TRY(hipMemcpy(cid.data(), sc->xids.p, (size_t)N * c * 8, hipMemcpyDeviceToHost));
        for (uint32_t q = 0; q < N; q++)
            if (fl[q] == 1u) host_walk(q);
        HN_TRY(hipMemcpyAsync(sc->xids.p, cid.data(), (size_t)N * c * 8, hipMemcpyHostToDevice, s));
        HN_TRY(hipMemcpyAsync(sc->xcnt.p, ccnt.data(), (size_t)N * 4, hipMemcpyHostToDevice, s));
        st = enqueue_rerank(h, sc, (const float*)h->hq.p, N, c, top_k, metric, (uint64_t*)h->hids.p, (float*)h->hsc.p, (uint32_t*)h->hcnt.p, s, filter);
        if (st != NMN_OK) return st;
        if ((st = hand_out_rows(h, batch, top_k, s)) != NMN_OK) return st;
        HN_TRY(hipStreamSynchronize(s));
    }
    for (uint32_t q = 0; q < N; q++) {
        HostWalk* r = slot[q].r;
        r->evals += ev[q];
        if (fl[q] != 0u) r->spilled++;
        r->rescored = std::max(r->rescored, std::min(ccnt[q], c));
    }
    return NMN_OK;
}

// The calls of `batch`, in order, as ONE walk on the handle's own stream; every call gets its own rows, counts and figures.  A batch
// whose queries all walk with the same k and ef and whose callers' rows are k apart (a lone nmn_hnsw_search is one) is the uniform
// launch, straight between the callers' buffers and the device.  Any other batch is the per-query launch: the queries are gathered in
// launch order (those that start in LDS first), and the launch's rows, kstride = the largest k apart, are handed out on the host.
// Metric calls (docs/hnsw.md §12) ride the same walk with k = their candidate count; behind it, on the same stream, the per-query
// re-rank and ordering run over the metric slots, and one read-back serves everybody.  A batch of metric slots with one top_k and
// one metric is run_metric_uniform.  Sparse calls (§14) bring a query kind per slot, sparse_route's: a kind-0 slot is densified
// here and is a dense query from then on; a batch with other kinds is the per-query launch with QK = 3, except the lone sparse
// call with one k and one ef, which stays the uniform QK = 1 / QK = 2 launch.  Takes rw (shared) and host_mu for the batch.  A
// failure is the whole batch's.
// Cache calls (§16) are metric calls whose candidate count is the 3k rule's and whose slots carry a threshold and the filter flag: the
// merge re-rank of their Sparse-node candidates and the filtered ordering run behind the dense re-rank, per query like it.
// on_host (a metric call under NMN_HNSW_HOST_SEARCH=1, alone): the walks on the host, the re-rank on the device.
nmn_status run_batch(nmn_hnsw* h, const std::vector<HostWalk*>& batch, bool on_host = false) {
    std::shared_lock<std::shared_mutex> g(h->rw);
    std::lock_guard<std::mutex> hl(h->host_mu);  // the insert's upload uses the same stream and staging
    HN_TRY(hipSetDevice(h->device));
    const uint32_t n = (uint32_t)h->level.size(), dim = h->dim;
    const uint32_t route = (uint32_t)sparse_route(h);
    uint32_t N = 0;
    for (const HostWalk* r : batch) N += r->nq;
    std::vector<Slot> slot;  // launch order
    slot.reserve(N);
    auto slot_of = [&](HostWalk* r, uint32_t i) {
        if (r->sp) return Slot{r, i, r->k_of(i), r->ef_of(i, h->cfg.ef_search), 0, nullptr, route};
        if (!r->xm) return Slot{r, i, r->k_of(i), r->ef_of(i, h->cfg.ef_search), 0, nullptr, 0};
        // here, under rw: an insert may have run since the call was checked
        const uint32_t c = (uint32_t)(r->filter ? cache_candidates(h, r->k_of(i)) : metric_candidates(h, r->k_of(i)));
        return Slot{r, i, c, std::max<uint32_t>(h->cfg.ef_search, c), r->k_of(i), &r->metric_of(i), 0, r->filter, r->threshold};
    };
    const Slot s0 = slot_of(batch[0], 0);
    const uint32_t k0 = s0.k, ef0 = s0.ef;
    const uint32_t row0 = s0.xm ? s0.top : k0;  // the callers' row length a uniform batch needs
    bool uniform = true, plain = true;  // plain: every slot is a dense query to the kernel (kind 0)
    uint32_t kmax = 0, M = 0, topmax = 0;
    bool any_filter = false;
    for (HostWalk* r : batch) {
        r->evals = 0;
        r->spilled = 0;
        r->rescored = 0;
        if (r->kstride != row0) uniform = false;
        for (uint32_t i = 0; i < r->nq; i++) {
            const Slot sl = slot_of(r, i);
            if (sl.k != k0 || sl.ef != ef0 || sl.top != s0.top || !sl.xm != !s0.xm || (sl.xm && memcmp(sl.xm, s0.xm, sizeof(nmn_xmetric)) != 0))
                uniform = false;
            if (sl.filt != s0.filt || (sl.filt && memcmp(&sl.thr, &s0.thr, 4) != 0)) uniform = false;  // (thresholds agree bit for bit)
            any_filter = any_filter || sl.filt;
            if (sl.kind != 0u) plain = false;
            kmax = std::max(kmax, sl.k);
            if (sl.xm) {
                M++;
                topmax = std::max(topmax, sl.top);
            }
            slot.push_back(sl);
        }
    }
    if (uniform && M) return run_metric_uniform(h, batch, slot, on_host);
    // one sparse call with one k and one ef keeps the uniform launch of its kind; every other batch with a kind-1 or kind-2 slot in
    // it is the per-query launch, whatever its k and ef
    const bool lone_sparse = uniform && !plain && batch.size() == 1;
    const bool perq = !uniform || (!plain && !lone_sparse);
    hipStream_t s = h->host_stream;
    bool synced = true;  // (every earlier host call ended with a wait)
    const hipStream_t none = (hipStream_t)-1;
    const uint32_t kstride = kmax;  // (a uniform batch: k0)
    HN_TRY(grow(h->hq, (size_t)N * dim * 4, none, &synced));
    HN_TRY(grow(h->hids, (size_t)N * kstride * 8, none, &synced));
    HN_TRY(grow(h->hsc, (size_t)N * kstride * 4, none, &synced));
    HN_TRY(grow(h->hcnt, (size_t)N * 4, none, &synced));
    nmn_hnsw::Scratch* sc = scratch_of(h, s);
    std::vector<uint32_t> fl(N), ev(N);
    static thread_local HostVisited vis;
    // a query with more stored entries than a wave keeps in LDS walks in the launch as an entry-less query and is answered by the host
    // ... and so is a sparse query the device does not walk on a handle with Sparse nodes (sparse_query_host_only)
    auto too_long = [&](const Slot& x) {
        return (x.kind == 1u && x.r->sp->nnz(x.i) > kSparseLdsEntries) || (x.r->sp && sparse_query_host_only(h, *x.r->sp, x.i));
    };
    auto host_one = [&](const Slot& x, uint64_t* ids, float* scs, uint32_t* cnt, uint64_t* e2) {
        if (x.r->sp)
            host_search_one_sparse(h, *x.r->sp, x.i, x.k, x.ef, vis, ids, scs, cnt, e2);
        else
            host_search_one(h, x.r->q + (size_t)x.i * dim, x.k, x.ef, vis, ids, scs, cnt, e2);
    };
    // The queries of the slots, in launch order, into the host staging and up: the dense form of every slot that is not kind 1
    // (a sparse call's by to_dense) into hq, and, when a slot is not kind 0, the CSR of the kind-1 slots and Q.magnitude() of
    // every sparse slot.  w gets what the kernel reads of them.
    auto stage_queries = [&](WalkShape& w) -> nmn_status {
        bool any_dense = false;  // (a launch of kind-1 queries only reads no dense query: nothing to fill or send)
        for (const Slot& x : slot) any_dense = any_dense || x.kind != 1u;
        if (any_dense) h->st_q.resize((size_t)N * dim);
        h->st_spoff.assign(1, 0);
        h->st_spent.clear();
        h->st_mag.assign(N, 0.0f);
        for (uint32_t j = 0; j < N; j++) {
            const Slot& x = slot[j];
            float* dq = h->st_q.data() + (size_t)j * dim;
            if (x.kind == 1u) {
                const SparseQueries& sq = *x.r->sp;
                const uint64_t c = sq.nnz(x.i);
                if (!too_long(x)) {
                    for (uint64_t e = sq.off[x.i]; e < sq.off[x.i + 1]; e++) {
                        uint32_t bits;
                        memcpy(&bits, &sq.val[e], 4);
                        h->st_spent.push_back(make_uint2(sq.pos[e], bits));
                    }
                    w.sp_max = std::max<uint32_t>(w.sp_max, (uint32_t)c);
                }
                if (any_dense) std::fill(dq, dq + dim, 0.0f);  // (not read: the launch takes this query from its entries)
            } else if (x.r->sp) {
                x.r->sp->to_dense(x.i, dim, dq);
            } else {
                memcpy(dq, x.r->q + (size_t)x.i * dim, (size_t)dim * 4);
            }
            if (x.kind != 0u) h->st_mag[j] = x.r->sp->mag[x.i];
            h->st_spoff.push_back(h->st_spent.size());
        }
        if (any_dense) HN_TRY(hipMemcpyAsync(h->hq.p, h->st_q.data(), (size_t)N * dim * 4, hipMemcpyHostToDevice, s));
        w.sp_only = !any_dense;
        if (plain) return NMN_OK;
        if (route == kSparseGather) {
            HN_TRY(grow(h->hsp_off, h->st_spoff.size() * 8, none, &synced));
            HN_TRY(grow(h->hsp_ent, std::max<size_t>(h->st_spent.size(), 1) * 8, none, &synced));
            HN_TRY(hipMemcpyAsync(h->hsp_off.p, h->st_spoff.data(), h->st_spoff.size() * 8, hipMemcpyHostToDevice, s));
            if (!h->st_spent.empty())
                HN_TRY(hipMemcpyAsync(h->hsp_ent.p, h->st_spent.data(), h->st_spent.size() * 8, hipMemcpyHostToDevice, s));
            w.sp_off = (const uint64_t*)h->hsp_off.p;
            w.sp_ent = (const uint2*)h->hsp_ent.p;
        }
        HN_TRY(grow(h->hqmag, (size_t)N * 4, none, &synced));
        HN_TRY(hipMemcpyAsync(h->hqmag.p, h->st_mag.data(), (size_t)N * 4, hipMemcpyHostToDevice, s));
        w.qmag = (const float*)h->hqmag.p;
        return NMN_OK;
    };
    XmetricBatchPlan plan;
    const XmetricFilter flt = cache_filter(h, 0.0f);  // (a threshold per item)
    auto metric_chain = [&]() -> nmn_status {  // behind whatever filled the walk's rows on s; the answers on their way back
        if (!M) return NMN_OK;
        HN_TRY(launch_xmetric_rerank_batch(h->vectors ? h->vectors->corpus : nullptr, h->vectors ? h->vectors->ld : 0, dim, n,
                                           (const float*)h->hq.p, kstride, (const uint64_t*)h->hids.p, (const uint32_t*)h->hcnt.p, plan,
                                           (const uint32_t*)h->hxmeta.p, (float*)h->hxsim.p, topmax, (uint64_t*)h->hxoids.p,
                                           (float*)h->hxosc.p, (uint32_t*)h->hxocnt.p, h->hxsort.p, s, any_filter ? &flt : nullptr));
        HN_TRY(hipMemcpyAsync(h->st_xoids.data(), h->hxoids.p, (size_t)M * topmax * 8, hipMemcpyDeviceToHost, s));
        HN_TRY(hipMemcpyAsync(h->st_xosc.data(), h->hxosc.p, (size_t)M * topmax * 4, hipMemcpyDeviceToHost, s));
        HN_TRY(hipMemcpyAsync(h->st_xocnt.data(), h->hxocnt.p, (size_t)M * 4, hipMemcpyDeviceToHost, s));
        return NMN_OK;
    };
    if (!perq) {
        if (lone_sparse) {  // the launch of the call's kind, k and ef in the arguments
            WalkShape w = uniform_shape(h, N, k0, ef0);
            w.qkind = (int)route;
            nmn_status st = stage_queries(w);
            if (st != NMN_OK) return st;
            std::lock_guard<std::mutex> slk(sc->mu);
            st = enqueue_walk_locked(h, sc, route == kSparseGather ? nullptr : (const float*)h->hq.p, N, w, (uint64_t*)h->hids.p,
                                     (float*)h->hsc.p, (uint32_t*)h->hcnt.p, s);
            if (st != NMN_OK) return st;
        } else {
            bool densify = false;
            for (const HostWalk* r : batch) densify = densify || r->sp;
            if (densify) h->st_q.resize((size_t)N * dim);
            uint32_t off = 0;
            for (const HostWalk* r : batch) {
                const float* src = r->q;
                if (r->sp) {  // (kind 0: the dense walk of Q.to_dense())
                    float* dq = h->st_q.data() + (size_t)off * dim;
                    for (uint32_t i = 0; i < r->nq; i++) r->sp->to_dense(i, dim, dq + (size_t)i * dim);
                    src = dq;
                }
                HN_TRY(hipMemcpyAsync((float*)h->hq.p + (size_t)off * dim, src, (size_t)r->nq * dim * 4, hipMemcpyHostToDevice, s));
                off += r->nq;
            }
            std::lock_guard<std::mutex> slk(sc->mu);
            nmn_status st = enqueue_search_locked(h, sc, (const float*)h->hq.p, N, k0, ef0, (uint64_t*)h->hids.p, (float*)h->hsc.p,
                                                  (uint32_t*)h->hcnt.p, s);
            if (st != NMN_OK) return st;
        }
        if (const nmn_status st = hand_out_rows(h, batch, k0, s); st != NMN_OK) return st;
    } else {
        // the grid must not mix queries that would take different first launches: those whose results heap fits LDS come first
        std::stable_partition(slot.begin(), slot.end(), [&](const Slot& x) { return results_fit_lds(h, x.ef, n); });
        WalkShape w;
        w.kstride = kstride;
        // k and ef per query; with a kind per query (QK = 3) also the kind and the candidate limit the query has in a launch of its
        // own: a kind-1 query alone sizes its query region by its entries (enqueue_walk_locked), every other by the dimension
        const uint32_t per = plain ? 2u : 4u;
        h->st_kef.resize((size_t)per * N);
        h->st_xitems.clear();
        for (uint32_t j = 0; j < N; j++) {
            const Slot& x = slot[j];
            h->st_kef[j] = x.k;
            h->st_kef[N + j] = x.ef;
            if (!plain) {
                uint32_t region = dim;
                if (x.kind == 1u) region = too_long(x) ? 2u : std::max<uint32_t>(2u * (uint32_t)x.r->sp->nnz(x.i), 2u);
                h->st_kef[2 * N + j] = x.kind;
                h->st_kef[3 * N + j] = cand_cap(x.ef, h->lds_ccap, region, n);
            }
            if (x.xm) h->st_xitems.push_back(XmetricBatchItem{j, x.k, x.top, *x.xm, x.thr, x.filt ? 1u : 0u});
            const uint32_t need = results_need(x.ef, n);
            w.rcap_all = std::max(w.rcap_all, need);
            if (results_fit_lds(h, x.ef, n)) {
                w.n_lds = j + 1;
                w.rcap_lds = std::max(w.rcap_lds, need);
                w.ef_lds = std::max(w.ef_lds, x.ef);
            }
        }
        HN_TRY(grow(h->hkef, (size_t)per * N * 4, none, &synced));
        w.qk = (const uint32_t*)h->hkef.p;
        w.qef = w.qk + N;
        if (!plain) {
            w.qkind = 3;
            w.qkinds = w.qk + 2 * (size_t)N;
            w.qccap = w.qk + 3 * (size_t)N;
        }
        nmn_status stq = stage_queries(w);
        if (stq != NMN_OK) return stq;
        HN_TRY(hipMemcpyAsync(h->hkef.p, h->st_kef.data(), (size_t)per * N * 4, hipMemcpyHostToDevice, s));
        // the metric slots: what the re-rank and ordering launches read, and the rows they answer into (row m = the m-th metric slot)
        if (M) {
            xmetric_batch_plan(h->st_xitems.data(), M, N, h->st_xmeta, plan);
            HN_TRY(grow(h->hxmeta, h->st_xmeta.size() * 4, none, &synced));
            HN_TRY(grow(h->hxsim, (size_t)N * kstride * 4, none, &synced));
            HN_TRY(grow(h->hxoids, (size_t)M * topmax * 8, none, &synced));
            HN_TRY(grow(h->hxosc, (size_t)M * topmax * 4, none, &synced));
            HN_TRY(grow(h->hxocnt, (size_t)M * 4, none, &synced));
            HN_TRY(grow(h->hxsort, plan.sort_bytes, none, &synced));
            HN_TRY(hipMemcpyAsync(h->hxmeta.p, h->st_xmeta.data(), h->st_xmeta.size() * 4, hipMemcpyHostToDevice, s));
            h->st_xoids.resize((size_t)M * topmax);
            h->st_xosc.resize((size_t)M * topmax);
            h->st_xocnt.resize(M);
        }
        h->st_ids.resize((size_t)N * kstride);
        h->st_sc.resize((size_t)N * kstride);
        h->st_cnt.resize(N);
        if (!on_host) {
            {
                std::lock_guard<std::mutex> slk(sc->mu);
                nmn_status st = enqueue_walk_locked(h, sc, (const float*)h->hq.p, N, w, (uint64_t*)h->hids.p, (float*)h->hsc.p,
                                                    (uint32_t*)h->hcnt.p, s);
                if (st != NMN_OK) return st;
            }
            nmn_status st = metric_chain();
            if (st != NMN_OK) return st;
            if (M < N) {  // (a metric slot's walk rows stay on the device)
                HN_TRY(hipMemcpyAsync(h->st_ids.data(), h->hids.p, (size_t)N * kstride * 8, hipMemcpyDeviceToHost, s));
                HN_TRY(hipMemcpyAsync(h->st_sc.data(), h->hsc.p, (size_t)N * kstride * 4, hipMemcpyDeviceToHost, s));
            }
            HN_TRY(hipMemcpyAsync(h->st_cnt.data(), h->hcnt.p, (size_t)N * 4, hipMemcpyDeviceToHost, s));
        } else {
            std::fill(fl.begin(), fl.end(), 1u);  // every walk is the host's
            std::fill(ev.begin(), ev.end(), 0u);
        }
    }
    if (!on_host) {
        HN_TRY(hipMemcpyAsync(fl.data(), sc->flags.p, (size_t)N * 4, hipMemcpyDeviceToHost, s));
        HN_TRY(hipMemcpyAsync(ev.data(), sc->evals.p, (size_t)N * 4, hipMemcpyDeviceToHost, s));
        HN_TRY(hipStreamSynchronize(s));
    }
    // a metric slot the spill launch could not answer (cannot happen while its heap holds n entries), or every one under on_host: the
    // host walks it into the launch's row, the rows go up again, and the device re-ranks again
    uint32_t redo = 0;
    for (uint32_t j = 0; j < N && M; j++) {
        const Slot& x = slot[j];
        if (!x.xm || fl[j] != 1u) continue;
        uint64_t* ids = h->st_ids.data() + (size_t)j * kstride;
        float* scs = h->st_sc.data() + (size_t)j * kstride;
        uint64_t e2 = 0;
        host_one(x, ids, scs, &h->st_cnt[j], &e2);
        pad_row(ids, scs, x.k, kstride);
        ev[j] = (uint32_t)e2;
        HN_TRY(hipMemcpyAsync((uint64_t*)h->hids.p + (size_t)j * kstride, ids, (size_t)kstride * 8, hipMemcpyHostToDevice, s));
        redo++;
    }
    if (redo) {
        HN_TRY(hipMemcpyAsync(h->hcnt.p, h->st_cnt.data(), (size_t)N * 4, hipMemcpyHostToDevice, s));
        const nmn_status st = metric_chain();
        if (st != NMN_OK) return st;
        HN_TRY(hipStreamSynchronize(s));
    }
    for (uint32_t j = 0, m = 0; j < N; j++) {
        const Slot& x = slot[j];
        HostWalk* r = x.r;
        uint64_t* ids = r->out_ids + (size_t)x.i * r->kstride;
        float* scs = r->out_scores + (size_t)x.i * r->kstride;
        if (x.xm) {  // row m of the ordering's answers; the large-k sort wrote only the first top_k slots of its rows
            const uint32_t c = std::min(x.top, r->kstride);
            memcpy(ids, h->st_xoids.data() + (size_t)m * topmax, (size_t)c * 8);
            memcpy(scs, h->st_xosc.data() + (size_t)m * topmax, (size_t)c * 4);
            pad_row(ids, scs, c, r->kstride);
            r->out_counts[x.i] = h->st_xocnt[m];
            r->rescored = std::max(r->rescored, std::min(h->st_cnt[j], x.k));
            if (!on_host && fl[j] != 0u) r->spilled++;
            m++;
        } else if (fl[j] == 1u || too_long(x)) {
            // the spill launch could not answer it (cannot happen while its heap holds n entries), or its entries did not fit LDS:
            // the host walk does, into the caller's row
            uint64_t e2 = 0;
            host_one(x, ids, scs, r->out_counts + x.i, &e2);
            pad_row(ids, scs, x.k, r->kstride);
            ev[j] = (uint32_t)e2;
            // (a query the device does not walk on a handle with sparse nodes keeps the dense handle's count: the kernel carries
            // the entry's distance from layer to layer, one evaluation fewer per upper layer than the reference makes)
            if (x.r->sp && sparse_query_host_only(h, *x.r->sp, x.i) && n) ev[j] -= h->max_layer;
            if (!too_long(x)) r->spilled++;
        } else {
            if (fl[j] == 2u) r->spilled++;
            if (perq) {  // slots [count, kstride) of the launch's row hold the sentinels already; the caller's row may be longer
                const uint32_t c = std::min(kstride, r->kstride);
                memcpy(ids, h->st_ids.data() + (size_t)j * kstride, (size_t)c * 8);
                memcpy(scs, h->st_sc.data() + (size_t)j * kstride, (size_t)c * 4);
                pad_row(ids, scs, c, r->kstride);
                r->out_counts[x.i] = h->st_cnt[j];
            }
        }
        r->evals += ev[j];
    }
    return NMN_OK;
}

// queue / lead / ride (coalesce_walk, nmn_hnsw_queue.h) around run_batch
nmn_status submit_walk(nmn_hnsw* h, HostWalk& me) {
    if (!hnsw_coalesce_enabled()) return run_batch(h, std::vector<HostWalk*>{&me});  // callers take turns on host_mu, as they always have
    const nmn_status st = coalesce_walk(
        h->co, me, [&](const std::vector<HostWalk*>& batch) { return run_batch(h, batch); }, [] { return std::string(nmn_last_error()); });
    if (st != NMN_OK && me.done) return set_error(st, me.err.c_str());  // rode in a batch that failed: the leader's text, on this thread
    return st;
}

// nmn_hnsw_search, nmn_hnsw_search_multi, nmn_hnsw_search_sparse and nmn_hnsw_search_sparse_multi behind their argument checks
nmn_status host_walk_call(nmn_hnsw* h, HostWalk& me, nmn_search_stats* stats) {
    const bool on_host = host_search_forced();
    if (on_host) {  // no turn to take: every caller walks on its own thread
        std::shared_lock<std::shared_mutex> g(h->rw);
        static thread_local HostVisited vis;
        for (uint32_t q = 0; q < me.nq; q++) {
            uint64_t* ids = me.out_ids + (size_t)q * me.kstride;
            float* scs = me.out_scores + (size_t)q * me.kstride;
            if (me.sp)
                host_search_one_sparse(h, *me.sp, q, me.k_of(q), me.ef_of(q, h->cfg.ef_search), vis, ids, scs, me.out_counts + q, &me.evals);
            else
                host_search_one(h, me.q + (size_t)q * h->dim, me.k_of(q), me.ef_of(q, h->cfg.ef_search), vis, ids, scs, me.out_counts + q, &me.evals);
            pad_row(ids, scs, me.k_of(q), me.kstride);
        }
    } else {
        nmn_status st = submit_walk(h, me);
        if (st != NMN_OK) return st;
    }
    if (stats) {
        stats->rows_scanned = me.evals;
        stats->bytes_scanned = h->storage == NMN_HNSW_STORAGE_QUANTIZED ? me.evals * (h->dim + 16ull)
                               : h->storage == NMN_HNSW_STORAGE_BINARY  ? me.evals * 8ull * h->bin_w
                                                                         : me.evals * h->dim * 4;
        stats->fallback_queries = me.spilled;
        std::shared_lock<std::shared_mutex> g(h->rw);
        stats->sweep_kind = h->level.empty() ? NMN_SWEEP_NONE : NMN_SWEEP_GRAPH;
        stats->sweep_launches = on_host ? 0 : 2;
    }
    return NMN_OK;
}

// nmn_hnsw_search_metric, nmn_hnsw_search_metric_multi and nmn_hnsw_cache_search behind their argument checks
nmn_status metric_walk_call(nmn_hnsw* h, HostWalk& me, nmn_search_stats* stats) {
    const bool on_host = host_search_forced();
    bool empty;
    {
        std::shared_lock<std::shared_mutex> g(h->rw);
        empty = h->level.empty();
        for (uint32_t i = 0; i < me.nq && !me.alone; i++)
            me.alone = (me.filter ? cache_candidates(h, me.k_of(i)) : metric_candidates(h, me.k_of(i))) > kShareCandMax;
    }
    // the host walk has no turn to take at the queue, but the re-rank runs on the handle's own stream: run_batch, alone
    const nmn_status st = on_host ? run_batch(h, std::vector<HostWalk*>{&me}, true) : submit_walk(h, me);
    if (st != NMN_OK) return st;
    if (stats) {
        stats->rows_scanned = me.evals;
        stats->bytes_scanned = me.evals * h->dim * 4;
        stats->candidates_rescored = me.rescored;
        stats->fallback_queries = me.spilled;
        stats->sweep_kind = empty ? NMN_SWEEP_NONE : NMN_SWEEP_GRAPH;
        stats->sweep_launches = on_host ? 0 : 2;
    }
    return NMN_OK;
}

void clear_stats(nmn_search_stats* stats) {
    if (!stats) return;
    memset(stats, 0, sizeof *stats);
    stats->scan_ms = stats->total_ms = -1.0f;
}

// The k of every query of a _multi call, checked before the call joins a batch: a bad call fails alone, and nothing is written
nmn_status check_k_per_query(const uint32_t* k, uint32_t nq, uint32_t kstride) {
    for (uint32_t i = 0; i < nq; i++) {
        if (k[i] == 0) return set_error(NMN_ERR_INVALID_TOP_K, "k == 0");
        if (k[i] > kstride) return set_error(NMN_ERR_INVALID_ARGUMENT, "HNSW: k[i] above kstride, the row stride of the outputs");
    }
    return NMN_OK;
}

// nmn_hnsw_search_metric_device and nmn_hnsw_cache_search_device behind their argument checks: the walk for the rule's candidate
// count, the re-rank and the ordering, enqueued on the caller's stream.  cache: the 3k rule and the filtered ordering (docs/hnsw.md §16).
nmn_status metric_device_call(nmn_hnsw* h, const float* queries_dev, uint32_t nq, uint32_t top_k, const nmn_xmetric& metric, bool cache,
                              float threshold, uint64_t* out_ids_dev, float* out_scores_dev, uint32_t* out_counts_dev, void* stream) {
    std::shared_lock<std::shared_mutex> g(h->rw);
    const uint32_t c = (uint32_t)(cache ? cache_candidates(h, top_k) : metric_candidates(h, top_k));
    HN_TRY(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    nmn_hnsw::Scratch* sc = scratch_of(h, s);
    const XmetricFilter flt = cache_filter(h, threshold);
    const XmetricFilter* filter = cache ? &flt : nullptr;
    {
        std::lock_guard<std::mutex> slk(sc->mu);  // grow, walk, re-rank (both of a cache call) and ordering as one unit on this stream
        nmn_status st = metric_scratch(sc, s, nq, c, top_k, cache);
        if (st != NMN_OK) return st;
        st = enqueue_search_locked(h, sc, queries_dev, nq, c, 0, (uint64_t*)sc->xids.p, (float*)sc->xsc.p, (uint32_t*)sc->xcnt.p, s);
        if (st != NMN_OK) return st;
        st = enqueue_rerank(h, sc, queries_dev, nq, c, top_k, metric, out_ids_dev, out_scores_dev, out_counts_dev, s, filter);
        if (st != NMN_OK) return st;
    }
    return record_search(h, s);
}

}  // namespace

extern "C" nmn_status nmn_hnsw_search(nmn_hnsw* h, const float* queries, uint32_t nq, uint32_t k, uint32_t ef, uint64_t* out_ids,
                                      float* out_scores, uint32_t* out_counts, nmn_search_stats* stats) {
    if (!h) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (k == 0) return set_error(NMN_ERR_INVALID_TOP_K, "k == 0");
    clear_stats(stats);
    if (nq == 0) return NMN_OK;
    if (!queries || !out_ids || !out_scores || !out_counts) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    HostWalk me;
    me.q = queries;
    me.nq = nq;
    me.k1 = me.kstride = k;
    me.ef1 = ef;
    me.out_ids = out_ids;
    me.out_scores = out_scores;
    me.out_counts = out_counts;
    return host_walk_call(h, me, stats);
}

extern "C" nmn_status nmn_hnsw_search_multi(nmn_hnsw* h, const float* queries, uint32_t nq, const uint32_t* k, const uint32_t* ef,
                                            uint32_t kstride, uint64_t* out_ids, float* out_scores, uint32_t* out_counts,
                                            nmn_search_stats* stats) {
    if (!h) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (kstride == 0) return set_error(NMN_ERR_INVALID_TOP_K, "kstride == 0");
    clear_stats(stats);
    if (nq == 0) return NMN_OK;
    if (!queries || !k || !out_ids || !out_scores || !out_counts) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (const nmn_status sk = check_k_per_query(k, nq, kstride); sk != NMN_OK) return sk;
    HostWalk me;
    me.q = queries;
    me.nq = nq;
    me.k = k;
    me.ef = ef;
    me.kstride = kstride;
    me.out_ids = out_ids;
    me.out_scores = out_scores;
    me.out_counts = out_counts;
    return host_walk_call(h, me, stats);
}

namespace {
// A sparse call shares a batch only where that leaves every rider's candidate limit what it is alone (docs/hnsw.md §14): the query
// region of a batch holds the longer of a dense query and the longest entry list, and cand_cap halves the limit above 4096 floats.
// A kind-1 call alone sizes the region by its entries; so it rides alone when the dimension is above 4096 (the batch's region would
// be long where its own may be short) or when one of its queries has more than 2048 entries (its region would be long for everybody).
bool sparse_rides_alone(const nmn_hnsw* h, const SparseQueries& sq, uint32_t nq) {
    if (sparse_route(h) != kSparseGather) return false;
    if (h->dim > 4096u) return true;
    for (uint32_t q = 0; q < nq; q++)
        if (sq.nnz(q) > 2048u) return true;
    return false;
}
}  // namespace

// HNSWIndex::search_sparse_with_ef (hnsw.rs:2118-2166), docs/hnsw.md §13.  Through the coalescer like nmn_hnsw_search (§14).
extern "C" nmn_status nmn_hnsw_search_sparse(nmn_hnsw* h, const uint64_t* indptr, const uint32_t* positions, const float* values,
                                             uint32_t nq, uint32_t k, uint32_t ef, uint64_t* out_ids, float* out_scores,
                                             uint32_t* out_counts, nmn_search_stats* stats) {
    if (!h) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (const nmn_status sb = refuse_binary(h, "nmn_hnsw_search_sparse", kBinQueries); sb != NMN_OK) return sb;
    if (k == 0) return set_error(NMN_ERR_INVALID_TOP_K, "k == 0");
    clear_stats(stats);
    if (nq == 0) return NMN_OK;
    if (!indptr || !out_ids || !out_scores || !out_counts) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    SparseQueries sq;  // every query as try_from_parts leaves it, before the call joins a batch or anything is written
    const nmn_status st = canonicalise_sparse(h->dim, indptr, positions, values, nq, &sq);
    if (st != NMN_OK) return st;
    HostWalk me;
    me.sp = &sq;
    me.nq = nq;
    me.k1 = me.kstride = k;
    me.ef1 = ef;
    me.alone = sparse_rides_alone(h, sq, nq);
    me.out_ids = out_ids;
    me.out_scores = out_scores;
    me.out_counts = out_counts;
    return host_walk_call(h, me, stats);
}

// The same with a k and an ef per query, as nmn_hnsw_search_multi has them: answer i is nmn_hnsw_search_sparse(q_i, 1, k[i], ef[i]).
extern "C" nmn_status nmn_hnsw_search_sparse_multi(nmn_hnsw* h, const uint64_t* indptr, const uint32_t* positions, const float* values,
                                                   uint32_t nq, const uint32_t* k, const uint32_t* ef, uint32_t kstride,
                                                   uint64_t* out_ids, float* out_scores, uint32_t* out_counts, nmn_search_stats* stats) {
    if (!h) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (const nmn_status sb = refuse_binary(h, "nmn_hnsw_search_sparse_multi", kBinQueries); sb != NMN_OK) return sb;
    if (kstride == 0) return set_error(NMN_ERR_INVALID_TOP_K, "kstride == 0");
    clear_stats(stats);
    if (nq == 0) return NMN_OK;
    if (!indptr || !k || !out_ids || !out_scores || !out_counts) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (const nmn_status sk = check_k_per_query(k, nq, kstride); sk != NMN_OK) return sk;
    SparseQueries sq;
    const nmn_status st = canonicalise_sparse(h->dim, indptr, positions, values, nq, &sq);
    if (st != NMN_OK) return st;
    HostWalk me;
    me.sp = &sq;
    me.nq = nq;
    me.k = k;
    me.ef = ef;
    me.kstride = kstride;
    me.alone = sparse_rides_alone(h, sq, nq);
    me.out_ids = out_ids;
    me.out_scores = out_scores;
    me.out_counts = out_counts;
    return host_walk_call(h, me, stats);
}

extern "C" nmn_status nmn_hnsw_coalesce_stats(nmn_hnsw* h, uint64_t* batches, uint64_t* calls) {
    if (!h) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lk(h->co.mu);
    if (batches) *batches = h->co.batches;
    if (calls) *calls = h->co.calls;
    return NMN_OK;
}

extern "C" nmn_status nmn_hnsw_search_metric_device(nmn_hnsw* h, const float* queries_dev, uint32_t nq, uint32_t top_k,
                                                    const nmn_xmetric* metric, uint64_t* out_ids_dev, float* out_scores_dev,
                                                    uint32_t* out_counts_dev, void* stream) {
    nmn_status st = check_metric_call(h, top_k, metric);
    if (st != NMN_OK) return st;
    if (nq == 0) return NMN_OK;
    if (!queries_dev || !out_ids_dev || !out_scores_dev || !out_counts_dev) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    return metric_device_call(h, queries_dev, nq, top_k, *metric, false, 0.0f, out_ids_dev, out_scores_dev, out_counts_dev, stream);
}

extern "C" nmn_status nmn_hnsw_search_metric(nmn_hnsw* h, const float* queries, uint32_t nq, uint32_t top_k, const nmn_xmetric* metric,
                                             uint64_t* out_ids, float* out_scores, uint32_t* out_counts, nmn_search_stats* stats) {
    nmn_status st = check_metric_call(h, top_k, metric);
    if (st != NMN_OK) return st;
    clear_stats(stats);
    if (nq == 0) return NMN_OK;
    if (!queries || !out_ids || !out_scores || !out_counts) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    HostWalk me;  // through the coalescer like nmn_hnsw_search (docs/hnsw.md §12); a lone call is the uniform chain it always was
    me.q = queries;
    me.nq = nq;
    me.k1 = me.kstride = top_k;
    me.xm = metric;
    me.out_ids = out_ids;
    me.out_scores = out_scores;
    me.out_counts = out_counts;
    return metric_walk_call(h, me, stats);
}

extern "C" nmn_status nmn_hnsw_search_metric_multi(nmn_hnsw* h, const float* queries, uint32_t nq, const uint32_t* top_k,
                                                   const nmn_xmetric* metrics, uint32_t kstride, uint64_t* out_ids, float* out_scores,
                                                   uint32_t* out_counts, nmn_search_stats* stats) {
    if (!h) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (h->storage != NMN_HNSW_STORAGE_DENSE) {
        nmn_xmetric any{NMN_XMETRIC_COSINE, 0.0f, 0.0f, 0.0f};
        return check_metric_call(h, 1, &any);  // the quantized handle's refusal, in nmn_hnsw_search_metric's words
    }
    if (kstride == 0) return set_error(NMN_ERR_INVALID_TOP_K, "kstride == 0");
    if (nq && (!queries || !top_k || !metrics || !out_ids || !out_scores || !out_counts)) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    for (uint32_t i = 0; i < nq; i++) {  // before the call joins a batch: a bad call fails alone, and nothing is written
        if (top_k[i] == 0) return set_error(NMN_ERR_INVALID_TOP_K, "top_k == 0");
        if (top_k[i] > kstride) return set_error(NMN_ERR_INVALID_ARGUMENT, "HNSW: top_k[i] above kstride, the row stride of the outputs");
        if (!xmetric_valid(&metrics[i])) return set_error(NMN_ERR_CONFIGURATION, "unknown extended distance metric");
    }
    clear_stats(stats);
    if (nq == 0) return NMN_OK;
    HostWalk me;
    me.q = queries;
    me.nq = nq;
    me.k = top_k;
    me.xm = metrics;
    me.xm_stride = 1;
    me.kstride = kstride;
    me.out_ids = out_ids;
    me.out_scores = out_scores;
    me.out_counts = out_counts;
    return metric_walk_call(h, me, stats);
}

// ---- CacheIndex::search_with_metric behind the walk (tensor_cache/src/index.rs:186-375; docs/hnsw.md §16) ---------------------------
namespace {
nmn_status check_cache_call(nmn_hnsw* h, uint32_t k, const nmn_xmetric* m) {
    if (!h || !m) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (const nmn_status sb = refuse_binary(h, "nmn_hnsw_cache_search", kBinNoRows); sb != NMN_OK) return sb;
    if (h->storage != NMN_HNSW_STORAGE_DENSE)
        return set_error(NMN_ERR_CONFIGURATION,
                         "HNSW: nmn_hnsw_cache_search re-scores the stored form of its candidates, and a CacheIndex never holds "
                         "quantized nodes (a dense-strategy handle only)");
    if (!xmetric_valid(m)) return set_error(NMN_ERR_CONFIGURATION, "unknown extended distance metric");
    if (k == 0) return set_error(NMN_ERR_INVALID_TOP_K, "k == 0");
    return NMN_OK;
}
}  // namespace

extern "C" nmn_status nmn_hnsw_set_node_mask(nmn_hnsw* h, const uint64_t* nodes, uint64_t n, int32_t live) {
    if (!h || (!nodes && n)) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (const nmn_status sb = refuse_binary(h, "nmn_hnsw_set_node_mask", "only nmn_hnsw_cache_search reads the mask"); sb != NMN_OK) return sb;
    if (n == 0) return NMN_OK;
    std::unique_lock<std::shared_mutex> g(h->rw);
    for (uint64_t i = 0; i < n; i++)  // before anything is flipped: the call is all or nothing
        if (nodes[i] >= h->live_n) return set_error(NMN_ERR_NOT_FOUND, "HNSW: node out of range");
    HN_TRY(hipSetDevice(h->device));
    nmn_status st = wait_in_flight(h);  // the searches in flight read the words about to change
    if (st != NMN_OK) return st;
    {
        std::lock_guard<std::mutex> hl(h->host_mu);
        HN_TRY(hipStreamSynchronize(h->host_stream));
    }
    std::vector<uint64_t> words(n);
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t w = nodes[i] >> 5;
        const uint32_t bit = 1u << (nodes[i] & 31);
        if (live)
            h->live[w] |= bit;
        else
            h->live[w] &= ~bit;
        words[i] = w;
    }
    std::sort(words.begin(), words.end());
    words.erase(std::unique(words.begin(), words.end()), words.end());
    for (size_t i = 0; i < words.size();) {  // the touched words again, run by run
        size_t j = i + 1;
        while (j < words.size() && words[j] == words[j - 1] + 1) j++;
        HN_TRY(hipMemcpy((uint32_t*)h->d_live.p + words[i], h->live.data() + words[i], (j - i) * 4, hipMemcpyHostToDevice));
        i = j;
    }
    return NMN_OK;
}

extern "C" int32_t nmn_hnsw_node_live(nmn_hnsw* h, uint64_t node) {
    if (!h) return -1;
    std::shared_lock<std::shared_mutex> g(h->rw);
    if (node >= h->live_n) return -1;
    return (int32_t)((h->live[node >> 5] >> (node & 31)) & 1u);
}

extern "C" nmn_status nmn_hnsw_cache_search(nmn_hnsw* h, const float* queries, uint32_t nq, uint32_t k, float threshold,
                                            const nmn_xmetric* metric, uint64_t* out_ids, float* out_scores, uint32_t* out_counts,
                                            nmn_search_stats* stats) {
    nmn_status st = check_cache_call(h, k, metric);
    if (st != NMN_OK) return st;
    clear_stats(stats);
    if (nq == 0) return NMN_OK;
    if (!queries || !out_ids || !out_scores || !out_counts) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    HostWalk me;  // through the coalescer like nmn_hnsw_search_metric; a lone call is the uniform chain with the filtered ordering
    me.q = queries;
    me.nq = nq;
    me.k1 = me.kstride = k;
    me.xm = metric;
    me.filter = true;
    me.threshold = threshold;
    me.out_ids = out_ids;
    me.out_scores = out_scores;
    me.out_counts = out_counts;
    return metric_walk_call(h, me, stats);
}

extern "C" nmn_status nmn_hnsw_cache_search_device(nmn_hnsw* h, const float* queries_dev, uint32_t nq, uint32_t k, float threshold,
                                                   const nmn_xmetric* metric, uint64_t* out_ids_dev, float* out_scores_dev,
                                                   uint32_t* out_counts_dev, void* stream) {
    nmn_status st = check_cache_call(h, k, metric);
    if (st != NMN_OK) return st;
    if (nq == 0) return NMN_OK;
    if (!queries_dev || !out_ids_dev || !out_scores_dev || !out_counts_dev) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    return metric_device_call(h, queries_dev, nq, k, *metric, true, threshold, out_ids_dev, out_scores_dev, out_counts_dev, stream);
}

// CacheIndex::search_sparse_with_metric (index.rs:291-375).  An `alone` call in two steps: the walk is nmn_hnsw_search_sparse's own
// for c candidates (on the device or, where §15 says so, on the host), whose ids then go up for the device re-rank and the filtered
// ordering.  The dense re-rank runs on Q.to_dense(); a query with a duplicated position is scored by the merge kernel on its entries.
extern "C" nmn_status nmn_hnsw_cache_search_sparse(nmn_hnsw* h, const uint64_t* indptr, const uint32_t* positions, const float* values,
                                                   uint32_t nq, uint32_t k, float threshold, const nmn_xmetric* metric,
                                                   uint64_t* out_ids, float* out_scores, uint32_t* out_counts, nmn_search_stats* stats) {
    nmn_status st = check_cache_call(h, k, metric);
    if (st != NMN_OK) return st;
    clear_stats(stats);
    if (nq == 0) return NMN_OK;
    if (!indptr || !out_ids || !out_scores || !out_counts) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    SparseQueries sq;  // every query as try_from_parts leaves it, before anything is walked or written
    st = canonicalise_sparse(h->dim, indptr, positions, values, nq, &sq);
    if (st != NMN_OK) return st;
    uint32_t c;
    {
        std::shared_lock<std::shared_mutex> g(h->rw);
        c = (uint32_t)cache_candidates(h, k);
    }
    std::vector<uint64_t> cid((size_t)nq * c);
    std::vector<float> csc((size_t)nq * c);
    std::vector<uint32_t> ccnt(nq);
    HostWalk me;
    me.sp = &sq;
    me.nq = nq;
    me.k1 = me.kstride = c;
    me.alone = true;
    me.out_ids = cid.data();
    me.out_scores = csc.data();
    me.out_counts = ccnt.data();
    nmn_search_stats ws;
    st = host_walk_call(h, me, &ws);
    if (st != NMN_OK) return st;
    const uint32_t dim = h->dim;
    uint32_t rescored = 0;
    {
        std::shared_lock<std::shared_mutex> g(h->rw);
        std::lock_guard<std::mutex> hl(h->host_mu);
        HN_TRY(hipSetDevice(h->device));
        hipStream_t s = h->host_stream;
        bool synced = true;  // (every earlier host call ended with a wait)
        const hipStream_t none = (hipStream_t)-1;
        HN_TRY(grow(h->hq, (size_t)nq * dim * 4, none, &synced));
        HN_TRY(grow(h->hids, (size_t)nq * k * 8, none, &synced));
        HN_TRY(grow(h->hsc, (size_t)nq * k * 4, none, &synced));
        HN_TRY(grow(h->hcnt, (size_t)nq * 4, none, &synced));
        nmn_hnsw::Scratch* sc = scratch_of(h, s);
        std::lock_guard<std::mutex> slk(sc->mu);
        st = metric_scratch(sc, s, nq, c, k, true);
        if (st != NMN_OK) return st;
        h->st_q.resize((size_t)nq * dim);
        h->st_spoff.assign(1, 0);
        h->st_spent.clear();
        h->st_kef.assign(nq, 0u);
        bool any_dup = false;
        for (uint32_t q = 0; q < nq; q++) {
            sq.to_dense(q, dim, h->st_q.data() + (size_t)q * dim);
            if (sq.dup[q]) {  // its own entries go up: the merge kernel scores every candidate of it
                any_dup = true;
                h->st_kef[q] = 1u;
                for (uint64_t e = sq.off[q]; e < sq.off[q + 1]; e++) {
                    uint32_t bits;
                    memcpy(&bits, &sq.val[e], 4);
                    h->st_spent.push_back(make_uint2(sq.pos[e], bits));
                }
            }
            h->st_spoff.push_back(h->st_spent.size());
            rescored = std::max(rescored, std::min(ccnt[q], c));
        }
        XmetricFilter flt = cache_filter(h, threshold);
        HN_TRY(hipMemcpyAsync(h->hq.p, h->st_q.data(), (size_t)nq * dim * 4, hipMemcpyHostToDevice, s));
        HN_TRY(hipMemcpyAsync(sc->xids.p, cid.data(), (size_t)nq * c * 8, hipMemcpyHostToDevice, s));
        HN_TRY(hipMemcpyAsync(sc->xcnt.p, ccnt.data(), (size_t)nq * 4, hipMemcpyHostToDevice, s));
        if (any_dup) {
            HN_TRY(grow(h->hsp_off, h->st_spoff.size() * 8, none, &synced));
            HN_TRY(grow(h->hsp_ent, std::max<size_t>(h->st_spent.size(), 1) * 8, none, &synced));
            HN_TRY(grow(h->hkef, (size_t)nq * 4, none, &synced));
            HN_TRY(hipMemcpyAsync(h->hsp_off.p, h->st_spoff.data(), h->st_spoff.size() * 8, hipMemcpyHostToDevice, s));
            HN_TRY(hipMemcpyAsync(h->hsp_ent.p, h->st_spent.data(), h->st_spent.size() * 8, hipMemcpyHostToDevice, s));
            HN_TRY(hipMemcpyAsync(h->hkef.p, h->st_kef.data(), (size_t)nq * 4, hipMemcpyHostToDevice, s));
            flt.q_off = (const uint64_t*)h->hsp_off.p;
            flt.q_ent = (const uint2*)h->hsp_ent.p;
            flt.q_use = (const uint32_t*)h->hkef.p;
        }
        st = enqueue_rerank(h, sc, (const float*)h->hq.p, nq, c, k, *metric, (uint64_t*)h->hids.p, (float*)h->hsc.p, (uint32_t*)h->hcnt.p, s, &flt);
        if (st != NMN_OK) return st;
        HN_TRY(hipMemcpyAsync(out_ids, h->hids.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost, s));
        HN_TRY(hipMemcpyAsync(out_scores, h->hsc.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
        HN_TRY(hipMemcpyAsync(out_counts, h->hcnt.p, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
        HN_TRY(hipStreamSynchronize(s));
    }
    if (stats) {
        *stats = ws;
        stats->candidates_rescored = rescored;
    }
    return NMN_OK;
}

// ---- sparse queries in DEVICE memory (docs/hnsw.md §22) ------------------------------------------------------------------------------
namespace {

// What the host entries route to the host's walk (sparse_query_host_only) and a stream-ordered entry therefore cannot serve: known
// from the handle alone, refused before anything is enqueued.  (The third case, a QUERY with a duplicated position on a handle with
// sparse nodes, only the device sees: status 3.)  Caller holds rw.
nmn_status refuse_sparse_device(const nmn_hnsw* h, const char* entry) {
    if (!h->n_sparse) return NMN_OK;
    char buf[320];
    if (h->cfg.distance_metric == NMN_METRIC_EUCLIDEAN) {
        snprintf(buf, sizeof buf,
                 "HNSW: %s is not served on a handle with sparse nodes under Euclidean (the union merge is walked on the host: the "
                 "host-buffer entry serves it)", entry);
        return set_error(NMN_ERR_CONFIGURATION, buf);
    }
    if (h->n_sparse_dup > 0) {
        snprintf(buf, sizeof buf,
                 "HNSW: %s is not served on a handle with a sparse node that holds a duplicated position (the merge with it is walked "
                 "on the host: the host-buffer entry serves it)", entry);
        return set_error(NMN_ERR_CONFIGURATION, buf);
    }
    return NMN_OK;
}

// The canonicaliser on s into the stream's scratch: offsets, entries, magnitudes, duplicate flags, with `dense` the to_dense() rows,
// the statuses into status_dev (null: the scratch's own; *status: where they are).  Caller holds rw (shared) and sc->mu.
nmn_status enqueue_canon_locked(nmn_hnsw* h, nmn_hnsw::Scratch* sc, const uint64_t* indptr_dev, const uint32_t* positions_dev,
                                const float* values_dev, uint32_t nq, uint64_t nnz_total, uint32_t max_nnz, bool dense,
                                uint32_t* status_dev, const uint32_t** status, hipStream_t s) {
    bool synced = false;
    HN_TRY(grow(sc->sq_off, ((size_t)nq + 1) * 8, s, &synced));
    HN_TRY(grow(sc->sq_ent, std::max<size_t>(nnz_total, 1) * 8, s, &synced));
    HN_TRY(grow(sc->sq_mag, (size_t)nq * 4, s, &synced));
    HN_TRY(grow(sc->sq_dup, (size_t)nq * 4, s, &synced));
    if (dense) HN_TRY(grow(sc->sq_dense, (size_t)nq * h->dim * 4, s, &synced));
    if (!status_dev) {
        HN_TRY(grow(sc->sq_status, (size_t)nq * 4, s, &synced));
        status_dev = (uint32_t*)sc->sq_status.p;
    }
    *status = status_dev;
    // on a handle with sparse nodes (Cosine / DotProduct by now) a query with a duplicated position is not walked: status 3
    return launch_sparse_canon(h->dim, indptr_dev, positions_dev, values_dev, nq, nnz_total, max_nnz, h->n_sparse > 0,
                               (uint64_t*)sc->sq_off.p, (uint32_t*)sc->sq_ent.p, (float*)sc->sq_mag.p, (uint32_t*)sc->sq_dup.p,
                               dense ? (float*)sc->sq_dense.p : nullptr, status_dev, s);
}

// The walk of the canonical queries in the stream's scratch, routed as sparse_route says: the launch a lone nmn_hnsw_search_sparse
// call makes, its query region sized by the caller's bound instead of the call's largest count (no answer depends on it: cand_cap).
nmn_status enqueue_sparse_walk_locked(nmn_hnsw* h, nmn_hnsw::Scratch* sc, uint32_t nq, uint32_t k, uint32_t ef, uint32_t max_nnz,
                                      uint64_t* o_ids, float* o_sc, uint32_t* o_cnt, hipStream_t s) {
    const SparseRoute route = sparse_route(h);
    WalkShape w = uniform_shape(h, nq, k, ef);
    w.qkind = (int)route;
    if (route != kSparseDensify) w.qmag = (const float*)sc->sq_mag.p;
    if (route == kSparseGather) {
        w.sp_off = (const uint64_t*)sc->sq_off.p;
        w.sp_ent = (const uint2*)sc->sq_ent.p;
        w.sp_max = max_nnz;
    }
    return enqueue_walk_locked(h, sc, route == kSparseGather ? nullptr : (const float*)sc->sq_dense.p, nq, w, o_ids, o_sc, o_cnt, s);
}

bool sparse_csr_null(const uint64_t* indptr_dev, const uint32_t* positions_dev, const float* values_dev, uint64_t nnz_total) {
    return !indptr_dev || (nnz_total && (!positions_dev || !values_dev));
}

}  // namespace

// nmn_hnsw_search_sparse with the CSR and every output in DEVICE memory (docs/hnsw.md §22): the canonicaliser's three launches, the
// walk's two per chunk, and one that gives the queries with a status their sentinel rows.
extern "C" nmn_status nmn_hnsw_search_sparse_device(nmn_hnsw* h, const uint64_t* indptr_dev, const uint32_t* positions_dev,
                                                    const float* values_dev, uint32_t nq, uint64_t nnz_total, uint32_t max_nnz, uint32_t k,
                                                    uint32_t ef, uint64_t* out_ids_dev, float* out_scores_dev, uint32_t* out_counts_dev,
                                                    uint32_t* out_status_dev, void* stream) {
    uint32_t mx = 0;
    if (const nmn_status sm = sparse_max_nnz(h ? h->dim : 0, max_nnz, &mx); sm != NMN_OK) return sm;
    if (!h) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (const nmn_status sb = refuse_binary(h, "nmn_hnsw_search_sparse_device", kBinQueries); sb != NMN_OK) return sb;
    if (k == 0) return set_error(NMN_ERR_INVALID_TOP_K, "k == 0");
    if (nq == 0) return NMN_OK;
    if (sparse_csr_null(indptr_dev, positions_dev, values_dev, nnz_total) || !out_ids_dev || !out_scores_dev || !out_counts_dev)
        return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_lock<std::shared_mutex> g(h->rw);
    if (const nmn_status sr = refuse_sparse_device(h, "nmn_hnsw_search_sparse_device"); sr != NMN_OK) return sr;
    HN_TRY(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    nmn_hnsw::Scratch* sc = scratch_of(h, s);
    {
        std::lock_guard<std::mutex> slk(sc->mu);  // grow, canonicalise, walk and the status rows as one unit on this stream
        const uint32_t* status = nullptr;
        nmn_status st = enqueue_canon_locked(h, sc, indptr_dev, positions_dev, values_dev, nq, nnz_total, mx,
                                             sparse_route(h) != kSparseGather, out_status_dev, &status, s);
        if (st != NMN_OK) return st;
        st = enqueue_sparse_walk_locked(h, sc, nq, k, ef, mx, out_ids_dev, out_scores_dev, out_counts_dev, s);
        if (st != NMN_OK) return st;
        st = launch_sparse_status_rows(status, nq, k, out_ids_dev, out_scores_dev, out_counts_dev, s);
        if (st != NMN_OK) return st;
    }
    return record_search(h, s);
}

// nmn_hnsw_cache_search_sparse as one stream-ordered chain (docs/hnsw.md §22): canonicalise, the sparse walk for c candidates into
// the stream's candidate block, the re-rank on the to_dense() rows — a query with a duplicated position on its own entries, where
// the canonicaliser left them — the filtered ordering, the status rows.
extern "C" nmn_status nmn_hnsw_cache_search_sparse_device(nmn_hnsw* h, const uint64_t* indptr_dev, const uint32_t* positions_dev,
                                                          const float* values_dev, uint32_t nq, uint64_t nnz_total, uint32_t max_nnz,
                                                          uint32_t k, float threshold, const nmn_xmetric* metric, uint64_t* out_ids_dev,
                                                          float* out_scores_dev, uint32_t* out_counts_dev, uint32_t* out_status_dev,
                                                          void* stream) {
    uint32_t mx = 0;
    if (const nmn_status sm = sparse_max_nnz(h ? h->dim : 0, max_nnz, &mx); sm != NMN_OK) return sm;
    nmn_status st = check_cache_call(h, k, metric);
    if (st != NMN_OK) return st;
    if (nq == 0) return NMN_OK;
    if (sparse_csr_null(indptr_dev, positions_dev, values_dev, nnz_total) || !out_ids_dev || !out_scores_dev || !out_counts_dev)
        return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_lock<std::shared_mutex> g(h->rw);
    if (const nmn_status sr = refuse_sparse_device(h, "nmn_hnsw_cache_search_sparse_device"); sr != NMN_OK) return sr;
    const uint32_t c = (uint32_t)cache_candidates(h, k);
    HN_TRY(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    nmn_hnsw::Scratch* sc = scratch_of(h, s);
    {
        std::lock_guard<std::mutex> slk(sc->mu);
        st = metric_scratch(sc, s, nq, c, k, true);
        if (st != NMN_OK) return st;
        const uint32_t* status = nullptr;
        st = enqueue_canon_locked(h, sc, indptr_dev, positions_dev, values_dev, nq, nnz_total, mx, true, out_status_dev, &status, s);
        if (st != NMN_OK) return st;
        st = enqueue_sparse_walk_locked(h, sc, nq, c, 0, mx, (uint64_t*)sc->xids.p, (float*)sc->xsc.p, (uint32_t*)sc->xcnt.p, s);
        if (st != NMN_OK) return st;
        XmetricFilter flt = cache_filter(h, threshold);
        flt.q_off = (const uint64_t*)sc->sq_off.p;
        flt.q_ent = (const uint2*)sc->sq_ent.p;
        flt.q_use = (const uint32_t*)sc->sq_dup.p;
        st = enqueue_rerank(h, sc, (const float*)sc->sq_dense.p, nq, c, k, *metric, out_ids_dev, out_scores_dev, out_counts_dev, s, &flt);
        if (st != NMN_OK) return st;
        st = launch_sparse_status_rows(status, nq, k, out_ids_dev, out_scores_dev, out_counts_dev, s);
        if (st != NMN_OK) return st;
    }
    return record_search(h, s);
}

// ---- tensor-train queries and insert_tt_vector (hnsw.rs:1196-1221, 1755-1759, 1811-1903, 2238-2272; docs/hnsw.md §17) ---------------
namespace {

// cosine_distance_tt_with_norm on a node that is not stored as TT (hnsw.rs:1210-1219): q = tt_reconstruct(query), qmag = the
// walk's magnitude of the query (tt_norm, 0.0 when it is below 1e-10: the `== 0.0` tests below then return the reference's 1.0).
// Dense: simd::dot_product and simd::magnitude; Sparse: dot_dense and SparseVector::magnitude(); Quantized: dot_dense and
// magnitude_immutable — Cosine on every handle.
// A TensorTrain node (1201-1209; docs/hnsw.md §24): tt_dot_product(node, query) — node first — over the product of the cached norm
// and the query's, 1.0 when the shapes differ or the node's norm is below 1e-10; nothing is reconstructed.  (qmag == 0.0 stands
// for a query norm below 1e-10, which is 1.0 for every node: the first test of the reference.)
struct TTHostQuery {
    const uint32_t* shape;
    uint32_t n_cores;
    const uint32_t* ranks;
    const float* cores;
};
inline float tt_node_distance(const nmn_hnsw* h, uint32_t node, const float* q, float qmag, float qsum, const TTHostQuery& tq) {
    if (node_is_tt(h, node)) {
        if (qmag == 0.0f) return 1.0f;
        const nmn_hnsw::TTNode& t = node_train(h, node);
        if (t.n_cores != tq.n_cores || memcmp(t.shape, tq.shape, (size_t)t.n_cores * 4) != 0) return 1.0f;
        const float dot = tt_dot_host(t.shape, t.n_cores, t.ranks, h->tt_cores.data() + t.off, tq.ranks, tq.cores);
        if (t.norm < 1e-10f) return 1.0f;
        const float den = t.norm * qmag;
        const float sim = dot / den;
        return 1.0f - sim;
    }
    if (h->storage == NMN_HNSW_STORAGE_QUANTIZED) {
        HQ hq;
        hq.mag = qmag;
        hq.sum = qsum;
        return h_q8_distance(NMN_METRIC_COSINE, h->codes.data() + (size_t)node * h->dim, h->qscale[node], h->qmin[node], h->mags[node],
                             h->qxsq[node], q, hq, h->dim);
    }
    if (node_is_sparse(h, node)) {
        const SpView s = node_entries(h, node);
        const float dot = h_sparse_dot(s.pos, s.val, s.nnz, q);
        if (h->mags[node] == 0.0f || qmag == 0.0f) return 1.0f;
        const float den = h->mags[node] * qmag;
        const float sim = dot / den;
        return 1.0f - sim;
    }
    return h_distance(NMN_METRIC_COSINE, h->rows.data() + (size_t)node * h->dim, h->mags[node], q, qmag, h->dim);
}

// search_tt_with_ef of one prepared train on the host
void host_search_one_tt(const nmn_hnsw* h, const float* q, float norm, const TTHostQuery& tq, uint32_t k, uint64_t ef, HostVisited& vis,
                        uint64_t* ids, float* scores, uint32_t* count, uint64_t* evals) {
    const float qmag = tt_walk_magnitude(norm);
    const float qsum = h->storage == NMN_HNSW_STORAGE_QUANTIZED ? h_sum8(q, h->dim) : 0.0f;
    host_walk_one(h, [&](uint32_t node) { return tt_node_distance(h, node, q, qmag, qsum, tq); }, k, ef, vis, ids, scores, count, evals,
                  NMN_METRIC_COSINE);
}

// The walk of nq prepared TT queries on s: q_dev [nq][dim] the reconstructions, mag_dev [nq] their magnitudes.  The kernel already
// knows "a dense query whose Cosine magnitude is given": kind 2.  A quantized handle takes the QK = 2 launch; a handle with Sparse
// nodes the MIX launch with kind 2 for every query (mix_dense_query with the given magnitude), under every metric of the handle;
// a dense handle the per-query form QK = 3 on dense rows with a kind array of 2s (entries = false, mag_given = true) — no
// instantiation is added.  A handle with TensorTrain nodes (tt set; the caller checked tt_walk_on_device): the same per-query form
// with the TTN launches, sparse nodes or not (docs/hnsw.md §24).  Caller holds rw (shared) and sc->mu.
nmn_status enqueue_tt_walk_locked(nmn_hnsw* h, nmn_hnsw::Scratch* sc, const float* q_dev, const float* mag_dev, uint32_t nq, uint32_t k,
                                  uint32_t ef, uint64_t* o_ids, float* o_sc, uint32_t* o_cnt, hipStream_t s,
                                  const TTWalkQueries* tt = nullptr) {
    WalkShape w = uniform_shape(h, nq, k, ef);
    w.cosine = true;
    w.qmag = mag_dev;
    w.tt = tt;
    if (!tt && (h->storage == NMN_HNSW_STORAGE_QUANTIZED || h->n_sparse > 0)) {
        w.qkind = 2;
    } else {
        bool synced = false;
        HN_TRY(grow(sc->ttkind, (size_t)nq * 8, s, &synced));
        uint32_t* kinds = (uint32_t*)sc->ttkind.p;
        const uint32_t dim8 = (h->dim + 7u) & ~7u;
        const uint32_t ccap = cand_cap(w.ef_lds, h->lds_ccap, dim8, (uint32_t)h->level.size());  // (enqueue_walk_locked's own)
        HN_TRY(hipMemsetD32Async((hipDeviceptr_t)kinds, 2, nq, s));
        HN_TRY(hipMemsetD32Async((hipDeviceptr_t)(kinds + nq), (int)ccap, nq, s));
        w.qkind = 3;
        w.kstride = k;
        w.qkinds = kinds;
        w.qccap = kinds + nq;
    }
    return enqueue_walk_locked(h, sc, q_dev, nq, w, o_ids, o_sc, o_cnt, s);
}

nmn_status tt_dim_check(const nmn_hnsw* h, const TTBatch& b) {
    if (b.dim == h->dim) return NMN_OK;
    char buf[160];
    snprintf(buf, sizeof buf, "TT: the product of the shape is %llu, the index holds vectors of dimension %u", (unsigned long long)b.dim,
             h->dim);
    return set_error(NMN_ERR_DIMENSION_MISMATCH, buf);
}

}  // namespace

extern "C" nmn_status nmn_hnsw_search_tt(nmn_hnsw* h, const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks,
                                         const uint64_t* core_off, const float* cores, uint32_t nq, uint32_t k, uint32_t ef,
                                         uint64_t* out_ids, float* out_scores, uint32_t* out_counts, nmn_search_stats* stats) {
    if (!h) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (const nmn_status sb = refuse_binary(h, "nmn_hnsw_search_tt", kBinQueries); sb != NMN_OK) return sb;
    if (k == 0) return set_error(NMN_ERR_INVALID_TOP_K, "k == 0");
    clear_stats(stats);
    if (nq == 0) return NMN_OK;
    if (!core_off || !out_ids || !out_scores || !out_counts) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    TTBatch b;
    nmn_status st = tt_check(shape, n_cores, ranks, true, core_off, nq, true, &b);
    if (st != NMN_OK) return st;
    if (core_off[nq] > core_off[0] && !cores) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if ((st = tt_dim_check(h, b)) != NMN_OK) return st;
    b.cores = cores;
    bool on_host = host_search_forced();
    const uint32_t dim = h->dim;
    uint64_t evals = 0;
    uint32_t spilled = 0;
    static thread_local HostVisited vis;
    std::vector<float> hrow(dim);
    auto host_one = [&](uint32_t q) {  // preparation and walk of train q on the host, into the caller's row
        tt_reconstruct_host(shape, n_cores, b.ranks_of(q), cores + core_off[q], hrow.data());
        const float norm = tt_norm_host(shape, n_cores, b.ranks_of(q), cores + core_off[q]);
        const TTHostQuery tq{shape, n_cores, b.ranks_of(q), cores + core_off[q]};
        host_search_one_tt(h, hrow.data(), norm, tq, k, ef ? ef : h->cfg.ef_search, vis, out_ids + (size_t)q * k,
                           out_scores + (size_t)q * k, out_counts + q, &evals);
    };
    std::shared_lock<std::shared_mutex> g(h->rw);
    // a handle with TensorTrain nodes (docs/hnsw.md §24): the TTN launches when every node and every train of the call is within the
    // walk's LDS, the host walk — same bits — otherwise
    TTWalkQueries tw;
    const bool tt_nodes = !h->tt_nodes.empty();
    if (tt_nodes && !on_host) {
        tw.n_cores = n_cores;
        memcpy(tw.shape, b.shape, sizeof tw.shape);
        uint64_t smax = 0;
        for (uint32_t q = 0; q < nq; q++) {
            smax = std::max(smax, b.storage_of(q));
            for (uint32_t c = 0; c <= n_cores; c++) tw.max_rank = std::max(tw.max_rank, b.ranks_of(q)[c]);
        }
        const uint32_t ef_eff = std::max<uint32_t>(ef ? ef : h->cfg.ef_search, k);
        if (tt_walk_on_device(h, ef_eff, tw.max_rank, smax))
            tw.max_storage = (uint32_t)smax;
        else
            on_host = true;
    }
    if (on_host) {
        for (uint32_t q = 0; q < nq; q++) host_one(q);
    } else {
        std::lock_guard<std::mutex> hl(h->host_mu);  // callers take turns, as NMN_HNSW_NO_COALESCE=1 callers do
        HN_TRY(hipSetDevice(h->device));
        hipStream_t s = h->host_stream;
        bool synced = true;  // (every earlier host call ended with a wait)
        const hipStream_t none = (hipStream_t)-1;
        const uint64_t c0 = core_off[0], cn = core_off[nq] - c0;
        const size_t rk = (size_t)nq * (n_cores + 1);
        std::vector<uint64_t> off(core_off, core_off + nq + 1);
        for (uint64_t& o : off) o -= c0;
        HN_TRY(grow(h->htt_cores, std::max<size_t>(cn * 4, 4), none, &synced));
        HN_TRY(grow(h->htt_ranks, rk * 4, none, &synced));
        HN_TRY(grow(h->htt_off, (size_t)(nq + 1) * 8, none, &synced));
        HN_TRY(grow(h->htt_skip, nq, none, &synced));
        HN_TRY(grow(h->hids, (size_t)nq * k * 8, none, &synced));
        HN_TRY(grow(h->hsc, (size_t)nq * k * 4, none, &synced));
        HN_TRY(grow(h->hcnt, (size_t)nq * 4, none, &synced));
        if (cn) HN_TRY(hipMemcpyAsync(h->htt_cores.p, cores + c0, cn * 4, hipMemcpyHostToDevice, s));
        HN_TRY(hipMemcpyAsync(h->htt_ranks.p, ranks, rk * 4, hipMemcpyHostToDevice, s));
        HN_TRY(hipMemcpyAsync(h->htt_off.p, off.data(), (size_t)(nq + 1) * 8, hipMemcpyHostToDevice, s));
        HN_TRY(hipMemcpyAsync(h->htt_skip.p, b.on_host.data(), nq, hipMemcpyHostToDevice, s));
        nmn_hnsw::Scratch* sc = scratch_of(h, s);
        std::vector<float> mags(nq), big_rows;
        std::vector<uint32_t> fl(nq), ev(nq);
        {
            std::lock_guard<std::mutex> slk(sc->mu);
            bool ssynced = false;
            HN_TRY(grow(sc->ttq, (size_t)nq * dim * 4, s, &ssynced));
            HN_TRY(grow(sc->ttmag, (size_t)nq * 4, s, &ssynced));
            HN_TRY(launch_tt_prepare(b, (const float*)h->htt_cores.p, (const uint32_t*)h->htt_ranks.p, (const uint64_t*)h->htt_off.p,
                                     (const uint8_t*)h->htt_skip.p, (float*)sc->ttq.p, nullptr, (float*)sc->ttmag.p, s));
            if (b.n_on_host) {  // trains above the LDS limits: the host restatement, behind the launch into the rows it skipped
                big_rows.resize((size_t)b.n_on_host * dim);
                uint32_t j = 0;
                for (uint32_t q = 0; q < nq; q++) {
                    if (!b.on_host[q]) continue;
                    float* row = big_rows.data() + (size_t)j++ * dim;
                    tt_reconstruct_host(shape, n_cores, b.ranks_of(q), cores + core_off[q], row);
                    mags[q] = tt_walk_magnitude(tt_norm_host(shape, n_cores, b.ranks_of(q), cores + core_off[q]));
                    HN_TRY(hipMemcpyAsync((float*)sc->ttq.p + (size_t)q * dim, row, (size_t)dim * 4, hipMemcpyHostToDevice, s));
                    HN_TRY(hipMemcpyAsync((float*)sc->ttmag.p + q, &mags[q], 4, hipMemcpyHostToDevice, s));
                }
            }
            if (tt_nodes) {  // the trains as they were sent for the preparation: the kernel reads them again
                tw.cores_dev = (const float*)h->htt_cores.p;
                tw.ranks_dev = (const uint32_t*)h->htt_ranks.p;
                tw.off_dev = (const uint64_t*)h->htt_off.p;
            }
            st = enqueue_tt_walk_locked(h, sc, (const float*)sc->ttq.p, (const float*)sc->ttmag.p, nq, k, ef, (uint64_t*)h->hids.p,
                                        (float*)h->hsc.p, (uint32_t*)h->hcnt.p, s, tt_nodes ? &tw : nullptr);
            if (st != NMN_OK) return st;
            HN_TRY(hipMemcpyAsync(out_ids, h->hids.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost, s));
            HN_TRY(hipMemcpyAsync(out_scores, h->hsc.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
            HN_TRY(hipMemcpyAsync(out_counts, h->hcnt.p, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
            HN_TRY(hipMemcpyAsync(mags.data(), sc->ttmag.p, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
            HN_TRY(hipMemcpyAsync(fl.data(), sc->flags.p, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
            HN_TRY(hipMemcpyAsync(ev.data(), sc->evals.p, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
            HN_TRY(hipStreamSynchronize(s));
        }
        for (uint32_t q = 0; q < nq; q++) {
            // a NaN norm gives NaN distances, which the kernel's rank sort does not place: the host walk answers (its heaps and its
            // stable sort are the ones every walk is held to); so it does for a query the spill launch could not answer
            if (fl[q] == 1u || std::isnan(mags[q])) {
                host_one(q);
                if (fl[q] == 1u) spilled++;
            } else {
                evals += ev[q];
                if (fl[q] == 2u) spilled++;
            }
        }
    }
    if (stats) {
        stats->rows_scanned = evals;
        stats->bytes_scanned = h->storage == NMN_HNSW_STORAGE_QUANTIZED ? evals * (h->dim + 16ull) : evals * h->dim * 4;
        stats->fallback_queries = spilled;
        stats->sweep_kind = h->level.empty() ? NMN_SWEEP_NONE : NMN_SWEEP_GRAPH;
        stats->sweep_launches = on_host ? 0 : 3;  // the preparation and the walk's two
    }
    return NMN_OK;
}

extern "C" nmn_status nmn_hnsw_search_tt_device(nmn_hnsw* h, const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks,
                                                const float* cores_dev, uint32_t nq, uint32_t k, uint32_t ef, uint64_t* out_ids_dev,
                                                float* out_scores_dev, uint32_t* out_counts_dev, void* stream) {
    if (!h) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (const nmn_status sb = refuse_binary(h, "nmn_hnsw_search_tt_device", kBinQueries); sb != NMN_OK) return sb;
    if (k == 0) return set_error(NMN_ERR_INVALID_TOP_K, "k == 0");
    if (nq == 0) return NMN_OK;
    if (!cores_dev || !out_ids_dev || !out_scores_dev || !out_counts_dev) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    TTBatch b;
    nmn_status st = tt_check(shape, n_cores, ranks, false, nullptr, nq, false, &b);
    if (st != NMN_OK) return st;
    if (b.n_on_host)
        return set_error(NMN_ERR_INVALID_ARGUMENT,
                         "TT: the train is above the LDS limits of the device path (nmn_tt_limits); nmn_hnsw_search_tt prepares it on the host");
    if ((st = tt_dim_check(h, b)) != NMN_OK) return st;
    std::shared_lock<std::shared_mutex> g(h->rw);
    TTWalkQueries tw;
    const bool tt_nodes = !h->tt_nodes.empty();
    if (tt_nodes) {  // docs/hnsw.md §24: the TTN launches, or a refusal — there is no host to fall back to
        tw.n_cores = n_cores;
        memcpy(tw.shape, b.shape, sizeof tw.shape);
        memcpy(tw.ranks_u, ranks, (size_t)(n_cores + 1) * 4);
        for (uint32_t c = 0; c <= n_cores; c++) tw.max_rank = std::max(tw.max_rank, ranks[c]);
        tw.stride = b.storage_of(0);
        tw.max_storage = (uint32_t)tw.stride;
        tw.cores_dev = cores_dev;
        if (!tt_walk_on_device(h, std::max<uint32_t>(ef ? ef : h->cfg.ef_search, k), tw.max_rank, tw.stride))
            return set_error(NMN_ERR_INVALID_ARGUMENT,
                             "TT: the index holds TensorTrain nodes and the call is above the LDS limits of their device walk "
                             "(nmn_hnsw_tt_walk_limits); nmn_hnsw_search_tt walks it on the host");
    }
    HN_TRY(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    nmn_hnsw::Scratch* sc = scratch_of(h, s);
    {
        std::lock_guard<std::mutex> slk(sc->mu);
        bool synced = false;
        HN_TRY(grow(sc->ttq, (size_t)nq * h->dim * 4, s, &synced));
        HN_TRY(grow(sc->ttmag, (size_t)nq * 4, s, &synced));
        HN_TRY(launch_tt_prepare(b, cores_dev, nullptr, nullptr, nullptr, (float*)sc->ttq.p, nullptr, (float*)sc->ttmag.p, s));
        st = enqueue_tt_walk_locked(h, sc, (const float*)sc->ttq.p, (const float*)sc->ttmag.p, nq, k, ef, out_ids_dev, out_scores_dev,
                                    out_counts_dev, s, tt_nodes ? &tw : nullptr);
        if (st != NMN_OK) return st;
    }
    return record_search(h, s);
}

extern "C" nmn_status nmn_hnsw_insert_tt(nmn_hnsw* h, const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks,
                                         const uint64_t* core_off, const float* cores, uint64_t n, uint64_t* ids_out) {
    if (!h || (!core_off && n)) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (const nmn_status sb = refuse_binary(h, "nmn_hnsw_insert_tt", kBinNodes); sb != NMN_OK) return sb;
    if (h->storage != NMN_HNSW_STORAGE_DENSE)
        return set_error(NMN_ERR_CONFIGURATION,
                         "HNSW: insert_tt_vector makes Dense nodes, which are served on a dense handle only (insert the reconstruction "
                         "with nmn_hnsw_insert to quantize it)");
    if (n == 0) return NMN_OK;
    if (n >= (uint64_t)kNone) return set_error(NMN_ERR_CAPACITY, "HNSW: node ids are 32 bits on the device");
    TTBatch b;
    nmn_status st = tt_check(shape, n_cores, ranks, true, core_off, (uint32_t)n, true, &b);
    if (st != NMN_OK) return st;
    if ((st = tt_dim_check(h, b)) != NMN_OK) return st;
    HN_TRY(hipSetDevice(h->device));
    std::vector<float> rows((size_t)n * h->dim);
    st = nmn_tt_reconstruct(shape, n_cores, ranks, core_off, cores, (uint32_t)n, rows.data());
    if (st != NMN_OK) return st;
    return insert_rows(h, rows.data(), n, nullptr, nullptr, ids_out);
}

// insert_embedding(EmbeddingStorage::from(tt)) (hnsw.rs:1256-1259, 1913-2051) for each of the n trains in order: TensorTrain nodes.
// The reconstruction (the row of the flat index, the insert-time query) and the raw tt_norm come from nmn_tt_reconstruct /
// nmn_tt_norm — the preparation kernel, the host restatement above nmn_tt_limits.  Like nmn_hnsw_insert, no row is tested for
// finiteness: a train whose reconstruction holds a NaN or an infinity is inserted as it is.
extern "C" nmn_status nmn_hnsw_insert_embedding_tt(nmn_hnsw* h, const uint32_t* shape, uint32_t n_cores, const uint32_t* ranks,
                                                   const uint64_t* core_off, const float* cores, uint64_t n, uint64_t* ids_out) {
    if (!h || (!core_off && n)) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (const nmn_status sb = refuse_binary(h, "nmn_hnsw_insert_embedding_tt", kBinNodes); sb != NMN_OK) return sb;
    if (h->storage != NMN_HNSW_STORAGE_DENSE)
        return set_error(NMN_ERR_CONFIGURATION,
                         "HNSW: TensorTrain nodes are served on a dense handle only (the Quantized x TensorTrain arms are out of scope)");
    if (n == 0) return NMN_OK;
    if (n >= (uint64_t)kNone) return set_error(NMN_ERR_CAPACITY, "HNSW: node ids are 32 bits on the device");
    TTBatch b;
    nmn_status st = tt_check(shape, n_cores, ranks, true, core_off, (uint32_t)n, true, &b);
    if (st != NMN_OK) return st;
    if ((st = tt_dim_check(h, b)) != NMN_OK) return st;
    HN_TRY(hipSetDevice(h->device));
    std::vector<float> rows((size_t)n * h->dim), norms(n);
    st = nmn_tt_reconstruct(shape, n_cores, ranks, core_off, cores, (uint32_t)n, rows.data());
    if (st == NMN_OK) st = nmn_tt_norm(shape, n_cores, ranks, core_off, cores, (uint32_t)n, norms.data());
    if (st != NMN_OK) return st;
    b.cores = cores;
    return insert_rows(h, rows.data(), n, nullptr, nullptr, ids_out, false, &b, norms.data());
}

// get_embedding of a TensorTrain node: *storage = its core floats, UINT64_MAX for a node of another kind; every array nullable,
// shape_out [8], ranks_out [9], cores_out [cap] (cap >= *storage: NMN_ERR_BUFFER_TOO_SMALL otherwise)
extern "C" nmn_status nmn_hnsw_tt_row(nmn_hnsw* h, uint64_t node, uint32_t* shape_out, uint32_t* n_cores_out, uint32_t* ranks_out,
                                      float* cores_out, uint64_t cap, uint64_t* storage) {
    if (!h || !storage) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_lock<std::shared_mutex> g(h->rw);
    if (node >= h->level.size()) return set_error(NMN_ERR_NOT_FOUND, "HNSW: no such node");
    if (!node_is_tt(h, (uint32_t)node)) {
        *storage = UINT64_MAX;
        return NMN_OK;
    }
    const nmn_hnsw::TTNode& t = node_train(h, (uint32_t)node);
    *storage = t.storage;
    if (n_cores_out) *n_cores_out = t.n_cores;
    if (shape_out) memcpy(shape_out, t.shape, (size_t)t.n_cores * 4);
    if (ranks_out) memcpy(ranks_out, t.ranks, (size_t)(t.n_cores + 1) * 4);
    if (cores_out) {
        if (cap < t.storage) return set_error(NMN_ERR_BUFFER_TOO_SMALL, "nmn_hnsw_tt_row");
        if (t.storage) memcpy(cores_out, h->tt_cores.data() + t.off, (size_t)t.storage * 4);
    }
    return NMN_OK;
}

// The limits of the device walk of TT queries on a handle with TensorTrain nodes (docs/hnsw.md §24), each output nullable: the
// largest rank of any TT node, the TT nodes above nmn_tt_limits (any: TT queries walk on the host), and the floats a call with this
// ef (0: the config's ef_search) may spend on its largest train's cores + 2 x max_node_rank x its largest rank.
extern "C" nmn_status nmn_hnsw_tt_walk_limits(nmn_hnsw* h, uint32_t ef, uint32_t* max_node_rank, uint64_t* nodes_above_limits,
                                              uint32_t* lds_floats) {
    if (!h) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    std::shared_lock<std::shared_mutex> g(h->rw);
    if (max_node_rank) *max_node_rank = h->tt_max_rank;
    if (nodes_above_limits) *nodes_above_limits = h->n_tt_big;
    if (lds_floats) *lds_floats = tt_walk_lds_floats(h, ef ? ef : h->cfg.ef_search);
    return NMN_OK;
}

namespace {

nmn_status dense_dim_check(const nmn_hnsw* h, uint64_t dim) {
    if (dim == h->dim) return NMN_OK;
    char buf[160];
    snprintf(buf, sizeof buf, "HNSW: the vectors have %llu dimensions, the index holds vectors of dimension %u", (unsigned long long)dim,
             h->dim);
    return set_error(NMN_ERR_DIMENSION_MISMATCH, buf);
}

}  // namespace

extern "C" nmn_status nmn_hnsw_search_tt_dense(nmn_hnsw* h, const float* queries, uint32_t nq, uint64_t dim, const uint32_t* shape,
                                               uint32_t n_cores, uint32_t max_rank, float tolerance, uint32_t k, uint64_t* out_ids,
                                               float* out_scores, uint32_t* out_counts, nmn_search_stats* stats) {
    if (!h) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (const nmn_status sb = refuse_binary(h, "nmn_hnsw_search_tt_dense", kBinQueries); sb != NMN_OK) return sb;
    if (k == 0) return set_error(NMN_ERR_INVALID_TOP_K, "k == 0");
    clear_stats(stats);
    if (nq == 0) return NMN_OK;
    if (!queries || !out_ids || !out_scores || !out_counts) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    nmn_status st = dense_dim_check(h, dim);
    if (st != NMN_OK) return st;
    TTDecConfig c;
    if (tt_dec_config(dim, shape, n_cores, max_rank, tolerance, &c, nullptr, 0) != NMN_OK)  // Err for every query: search(query, k)
        return nmn_hnsw_search(h, queries, nq, k, 0, out_ids, out_scores, out_counts, stats);
    HN_TRY(hipSetDevice(h->device));
    std::vector<uint32_t> status(nq), ranks((size_t)nq * (n_cores + 1));
    std::vector<uint64_t> off(nq + 1);
    std::vector<float> cores((size_t)nq * c.slot);
    st = nmn_tt_decompose(queries, nq, dim, shape, n_cores, max_rank, tolerance, status.data(), ranks.data(), off.data(), cores.data(),
                          cores.size());
    if (st != NMN_OK) return st;
    std::vector<uint32_t> tt_q, dense_q;
    for (uint32_t q = 0; q < nq; q++) {
        if (status[q] != kTTStatusOk) {
            dense_q.push_back(q);
            continue;
        }
        for (uint32_t i = 1; i < n_cores; i++)
            if (ranks[(size_t)q * (n_cores + 1) + i] < 1) {
                char buf[120];
                snprintf(buf, sizeof buf, "TT: query %u: every rank must be >= 1", q);
                return set_error(NMN_ERR_INVALID_ARGUMENT, buf);
            }
        tt_q.push_back(q);
    }
    nmn_search_stats part{}, sum{};
    auto add = [&](bool first) {
        sum.rows_scanned += part.rows_scanned;
        sum.bytes_scanned += part.bytes_scanned;
        sum.fallback_queries += part.fallback_queries;
        sum.sweep_launches += part.sweep_launches;
        if (first || sum.sweep_kind == NMN_SWEEP_NONE) sum.sweep_kind = part.sweep_kind;
    };
    const size_t m1 = tt_q.size(), m2 = dense_q.size();
    std::vector<uint64_t> ids(std::max(m1, m2) * k);
    std::vector<float> sc(std::max(m1, m2) * k);
    std::vector<uint32_t> cnt(std::max(m1, m2));
    auto scatter = [&](const std::vector<uint32_t>& which) {
        for (size_t j = 0; j < which.size(); j++) {
            memcpy(out_ids + (size_t)which[j] * k, ids.data() + j * k, (size_t)k * 8);
            memcpy(out_scores + (size_t)which[j] * k, sc.data() + j * k, (size_t)k * 4);
            out_counts[which[j]] = cnt[j];
        }
    };
    if (m1) {  // the Ok queries: search_tt_with_ef of their trains, the ranks and core ranges of those queries gathered
        std::vector<uint32_t> r1(m1 * (n_cores + 1));
        std::vector<uint64_t> o1(m1 + 1, 0);
        std::vector<float> c1;
        for (size_t j = 0; j < m1; j++) {
            const uint32_t q = tt_q[j];
            memcpy(r1.data() + j * (n_cores + 1), ranks.data() + (size_t)q * (n_cores + 1), (n_cores + 1) * 4);
            c1.insert(c1.end(), cores.begin() + off[q], cores.begin() + off[q + 1]);
            o1[j + 1] = c1.size();
        }
        st = nmn_hnsw_search_tt(h, shape, n_cores, r1.data(), o1.data(), c1.data(), (uint32_t)m1, k, 0, ids.data(), sc.data(), cnt.data(),
                                &part);
        if (st != NMN_OK) return st;
        add(true);
        scatter(tt_q);
    }
    if (m2) {  // the Err queries: search(query, k) under the handle's metric
        std::vector<float> rows(m2 * dim);
        for (size_t j = 0; j < m2; j++) memcpy(rows.data() + j * dim, queries + (size_t)dense_q[j] * dim, dim * 4);
        st = nmn_hnsw_search(h, rows.data(), (uint32_t)m2, k, 0, ids.data(), sc.data(), cnt.data(), &part);
        if (st != NMN_OK) return st;
        add(m1 == 0);
        scatter(dense_q);
    }
    if (stats) *stats = sum;
    return NMN_OK;
}

namespace {

// insert_tt / insert_batch_tt: every vector decomposed for its status, then nmn_hnsw_insert's path
nmn_status insert_dense_validated(nmn_hnsw* h, const char* entry, const char* prefix, bool batch, const float* vectors, uint64_t n,
                                  uint64_t dim, const uint32_t* shape, uint32_t n_cores, uint32_t max_rank, float tolerance,
                                  uint64_t* ids_out) {
    if (!h) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (const nmn_status sb = refuse_binary(h, entry, kBinNodes); sb != NMN_OK) return sb;
    if (h->storage != NMN_HNSW_STORAGE_DENSE)
        return set_error(NMN_ERR_CONFIGURATION,
                         "HNSW: insert_tt makes Dense nodes, which are served on a dense handle only (nmn_hnsw_insert quantizes a row)");
    if (n == 0) return NMN_OK;
    if (!vectors) return set_error(NMN_ERR_INVALID_ARGUMENT, "null argument");
    if (n >= (uint64_t)kNone) return set_error(NMN_ERR_CAPACITY, "HNSW: node ids are 32 bits on the device");
    char text[600], debug[400];
    auto failed = [&](uint64_t q) {
        if (batch)
            snprintf(text, sizeof text, "%s: %s (vector %llu)", prefix, debug, (unsigned long long)q);
        else
            snprintf(text, sizeof text, "%s: %s", prefix, debug);
        return set_error(NMN_ERR_INVALID_ARGUMENT, text);
    };
    TTDecConfig c;
    if (tt_dec_config(dim, shape, n_cores, max_rank, tolerance, &c, debug, sizeof debug) != NMN_OK) return failed(0);
    nmn_status st = dense_dim_check(h, dim);
    if (st != NMN_OK) return st;
    HN_TRY(hipSetDevice(h->device));
    std::vector<uint32_t> status(n), ranks((size_t)n * (n_cores + 1));
    st = nmn_tt_decompose(vectors, n, dim, shape, n_cores, max_rank, tolerance, status.data(), ranks.data(), nullptr, nullptr, 0);
    if (st != NMN_OK) return st;
    for (uint64_t q = 0; q < n; q++)
        if (status[q] != kTTStatusOk) {
            snprintf(debug, sizeof debug, "Decompose(EmptyMatrix)");
            return failed(q);
        }
    return insert_rows(h, vectors, n, nullptr, nullptr, ids_out);
}

}  // namespace

extern "C" nmn_status nmn_hnsw_insert_tt_dense(nmn_hnsw* h, const float* vector, uint64_t dim, const uint32_t* shape, uint32_t n_cores,
                                               uint32_t max_rank, float tolerance, uint64_t* id_out) {
    return insert_dense_validated(h, "nmn_hnsw_insert_tt_dense", "TT decomposition failed", false, vector, 1, dim, shape, n_cores, max_rank,
                                  tolerance, id_out);
}

extern "C" nmn_status nmn_hnsw_insert_batch_tt(nmn_hnsw* h, const float* vectors, uint64_t n, uint64_t dim, const uint32_t* shape,
                                               uint32_t n_cores, uint32_t max_rank, float tolerance, uint64_t* ids_out) {
    return insert_dense_validated(h, "nmn_hnsw_insert_batch_tt", "Batch TT decomposition failed", true, vectors, n, dim, shape, n_cores,
                                  max_rank, tolerance, ids_out);
}
