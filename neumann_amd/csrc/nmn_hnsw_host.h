// nmn_hnsw_host.h — the host's walk of the HNSW graph (docs/hnsw.md): SparseVector's arithmetic on stored entries, the distance
// of a query to a node and of two nodes, and the walk templates (host_greedy, host_search_layer, host_walk_one) that the build
// (nmn_hnsw_build.hip) and the search side (nmn_hnsw.hip) both instantiate.  Internal linkage throughout: a distance and the walk
// that calls it are compiled, and inlined, together in each of the two.
// EVERY TRANSLATION UNIT THAT INCLUDES THIS HEADER IS BUILT WITH -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "nmn_hnsw_handle.h"

#pragma clang fp contract(off)

namespace nmn {
namespace {

// ---- SparseVector arithmetic on stored entries (sparse_vector.rs; docs/hnsw.md §13, §15) ------------------------------------------
// dot_dense (450-466): Iterator::sum::<f64>() of f64(val) * f64(dense[pos]) over the stored entries in order — a left-to-right
// fold from -0.0 (the convention of docs/hnsw.md §1 for std's float Sum); the caller casts
inline double h_sparse_dot64(const uint32_t* pos, const float* val, uint64_t nnz, const float* dense) {
    double acc = -0.0;
    for (uint64_t i = 0; i < nnz; i++) {
        const double p = (double)val[i] * (double)dense[pos[i]];
        acc = acc + p;
    }
    return acc;
}
inline float h_sparse_dot(const uint32_t* pos, const float* val, uint64_t nnz, const float* dense) {
    return (float)h_sparse_dot64(pos, val, nnz, dense);
}
// magnitude_f64 (554-559): the same fold over f64(v) * f64(v), an f64 sqrt; magnitude (548-551) is its cast
inline double h_sparse_mag64(const float* val, uint64_t nnz) {
    double acc = -0.0;
    for (uint64_t i = 0; i < nnz; i++) {
        const double p = (double)val[i] * (double)val[i];
        acc = acc + p;
    }
    return std::sqrt(acc);
}
inline float h_sparse_mag(const float* val, uint64_t nnz) { return (float)h_sparse_mag64(val, nnz); }
struct SpView {
    const uint32_t* pos;
    const float* val;
    uint64_t nnz;
};
// dot_f64 (419-443): the two-pointer merge, the accumulator from +0.0 (`0.0_f64`, no Sum)
inline double h_sparse_merge_dot64(const SpView& a, const SpView& b) {
    double r = 0.0;
    uint64_t i = 0, j = 0;
    while (i < a.nnz && j < b.nnz) {
        if (a.pos[i] == b.pos[j]) {
            const double p = (double)a.val[i] * (double)b.val[j];
            r = r + p;
            i++;
            j++;
        } else if (a.pos[i] < b.pos[j]) {
            i++;
        } else {
            j++;
        }
    }
    return r;
}
// euclidean_distance (942-1006): the f64 union merge, sqrt, clamped to f32::MAX, cast
inline float h_sparse_eucl(const SpView& a, const SpView& b) {
    double sum = 0.0;
    uint64_t i = 0, j = 0;
    while (i < a.nnz || j < b.nnz) {
        double d;
        if (i >= a.nnz) {
            d = (double)b.val[j++];
        } else if (j >= b.nnz) {
            d = (double)a.val[i++];
        } else if (a.pos[i] == b.pos[j]) {
            d = (double)a.val[i++] - (double)b.val[j++];
        } else if (a.pos[i] < b.pos[j]) {
            d = (double)a.val[i++];
        } else {
            d = -(double)b.val[j++];
        }
        const double p = d * d;
        sum = sum + p;
    }
    const double dist = std::sqrt(sum);
    return dist > (double)3.40282346638528859811704183484516925e+38f ? 3.40282346638528859811704183484516925e+38f : (float)dist;
}

inline bool node_is_sparse(const nmn_hnsw* h, uint32_t node) { return node < h->sp_nnz.size() && h->sp_nnz[node] != kNone; }
inline SpView node_entries(const nmn_hnsw* h, uint32_t node) {
    return SpView{h->sp_pos.data() + h->sp_off[node], h->sp_val.data() + h->sp_off[node], h->sp_nnz[node]};
}

inline bool node_is_tt(const nmn_hnsw* h, uint32_t node) { return node < h->tt_slot.size() && h->tt_slot[node] != kNone; }
inline const nmn_hnsw::TTNode& node_train(const nmn_hnsw* h, uint32_t node) { return h->tt_nodes[h->tt_slot[node]]; }

// the query side: distance_dense(stored row `node`, q).  A Sparse node (hnsw.rs:1035-1045, 1084-1091, 1136-1138): s.dot_dense(q)
// with s.magnitude() under Cosine / DotProduct, simd::euclidean_distance(s.to_dense(), q) — the row kept here — under Euclidean.
// A TensorTrain node (793-796, 1035-1045, 1093-1096; docs/hnsw.md §24): the Dense arithmetic on tt_reconstruct() — the row kept
// here — with the cached tt_norm as mag_self under Cosine: h->mags holds that norm, so the last line below is the rule.
inline float node_distance(const nmn_hnsw* h, uint32_t node, const float* q, const HQ& hq) {
    if (h->storage == NMN_HNSW_STORAGE_QUANTIZED)
        return h_q8_distance(h->cfg.distance_metric, h->codes.data() + (size_t)node * h->dim, h->qscale[node], h->qmin[node],
                             h->mags[node], h->qxsq[node], q, hq, h->dim);
    const int metric = h->cfg.distance_metric;
    if (h->storage == NMN_HNSW_STORAGE_BINARY)
        return h_bin_distance(metric, h->rows.data() + (size_t)node * h->dim, h->sqrt_dim, q, hq.mag, h->dim);
    if (metric != NMN_METRIC_EUCLIDEAN && node_is_sparse(h, node)) {
        const SpView s = node_entries(h, node);
        const float dot = h_sparse_dot(s.pos, s.val, s.nnz, q);
        if (metric == NMN_METRIC_DOT_PRODUCT) return -dot;
        if (h->mags[node] == 0.0f || hq.mag == 0.0f) return 1.0f;
        const float den = h->mags[node] * hq.mag;
        const float sim = dot / den;
        return 1.0f - sim;
    }
    return h_distance(metric, h->rows.data() + (size_t)node * h->dim, h->mags[node], q, hq.mag, h->dim);
}
// the query side for a SparseVector query Q on a Sparse node (hnsw.rs:1069-1079, 1108-1114, 1143-1145): s.dot(Q) with both
// magnitude()s, s.euclidean_distance(Q)
inline float sparse_node_sparse_query(const nmn_hnsw* h, uint32_t node, const SpView& Q, float qmag) {
    const int metric = h->cfg.distance_metric;
    const SpView s = node_entries(h, node);
    if (metric == NMN_METRIC_EUCLIDEAN) return h_sparse_eucl(s, Q);
    const float dot = (float)h_sparse_merge_dot64(s, Q);
    if (metric == NMN_METRIC_DOT_PRODUCT) return -dot;
    if (h->mags[node] == 0.0f || qmag == 0.0f) return 1.0f;
    const float den = h->mags[node] * qmag;
    const float sim = dot / den;
    return 1.0f - sim;
}
// the pruning side: try_*_distance on two stored rows — dense arithmetic on the rows the host keeps (a quantized handle keeps the
// dequantized rows and their simd::magnitude there: the (Quantized, Quantized) arms).  With a Sparse node in the pair
// (hnsw.rs:2453-2459, 2558-2565, 2641-2643): Sparse x Sparse is cosine_similarity (583-600) / euclidean_distance / dot; Dense x
// Sparse, either order, is cosine_distance_dense (606-632) / simd::euclidean_distance on to_dense() / dot_dense.
// Binary x Binary: Cosine is 1.0 - ba.similarity(bb) = 1.0 - (1.0 - hamming as f32 / dimension as f32) on the words (hnsw.rs:2516-2518,
// binary_quantization.rs:137-142) — NOT the query side's formula; Euclidean / DotProduct are the dense arithmetic on the +-1 rows.
inline float pair_of_nodes_distance(const nmn_hnsw* h, uint32_t a, uint32_t b) {
    const int metric = h->cfg.distance_metric;
    if (h->storage == NMN_HNSW_STORAGE_BINARY && metric == NMN_METRIC_COSINE) {
        const uint32_t hd = h_bin_hamming(h->bwords.data() + (size_t)a * h->bin_w, h->bwords.data() + (size_t)b * h->bin_w, h->bin_w);
        const float ratio = (float)hd / (float)h->dim;
        const float sim = 1.0f - ratio;
        return 1.0f - sim;
    }
    const bool sa = node_is_sparse(h, a), sb = node_is_sparse(h, b);
    if (sa && sb) {
        const SpView x = node_entries(h, a), y = node_entries(h, b);
        if (metric == NMN_METRIC_EUCLIDEAN) return h_sparse_eucl(x, y);
        const double dot = h_sparse_merge_dot64(x, y);
        if (metric == NMN_METRIC_DOT_PRODUCT) return -(float)dot;
        float sim = 0.0f;
        const double ma = h->sp_mag64[a], mb = h->sp_mag64[b];
        if (!(ma == 0.0 || mb == 0.0)) {
            const double den = ma * mb;
            const double r = dot / den;
            if (!(std::isnan(r) || std::isinf(r))) sim = (float)(r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r));
        }
        return 1.0f - sim;
    }
    if ((sa || sb) && metric != NMN_METRIC_EUCLIDEAN) {
        const uint32_t sn = sa ? a : b, dn = sa ? b : a;
        const SpView s = node_entries(h, sn);
        const float* v = h->rows.data() + (size_t)dn * h->dim;
        const double dot = h_sparse_dot64(s.pos, s.val, s.nnz, v);
        if (metric == NMN_METRIC_DOT_PRODUCT) return -(float)dot;
        const double ms = h->sp_mag64[sn];
        double acc = -0.0;  // the dense magnitude: a sequential f64 sum over every element
        for (uint32_t i = 0; i < h->dim; i++) {
            const double p = (double)v[i] * (double)v[i];
            acc = acc + p;
        }
        const double md = std::sqrt(acc);
        if (ms == 0.0 || md == 0.0) return 1.0f;
        const double den = ms * md;
        const double r = dot / den;
        if (std::isnan(r) || std::isinf(r)) return 1.0f;
        const double c = r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r);
        return (float)(1.0 - c);
    }
    // A TensorTrain node in the pair (docs/hnsw.md §24).  T x T under Cosine (hnsw.rs:2460-2468): 1.0 when a cached norm is below
    // 1e-10, else simd::dot_product of the two reconstructions over the product of the cached norms, no `== 0.0` test.  T x D under
    // Cosine (2469-2480): the Dense arm with simd::magnitude of the reconstruction, NOT the cached norm.  T x S was the arm above
    // (2481-2485: cosine_distance_dense on the reconstruction); Euclidean and DotProduct read no magnitude (2566-2581, 2644-2658).
    float mag_a = h->mags[a], mag_b = h->mags[b];
    if (metric == NMN_METRIC_COSINE && !h->tt_slot.empty()) {
        const bool ta = node_is_tt(h, a), tb = node_is_tt(h, b);
        if (ta && tb) {
            if (mag_a < 1e-10f || mag_b < 1e-10f) return 1.0f;
            const float dot = h_dot8(h->rows.data() + (size_t)a * h->dim, h->rows.data() + (size_t)b * h->dim, h->dim);
            const float den = mag_a * mag_b;
            const float sim = dot / den;
            return 1.0f - sim;
        }
        if (ta) mag_a = node_train(h, a).row_mag;
        if (tb) mag_b = node_train(h, b).row_mag;
    }
    return h_distance(metric, h->rows.data() + (size_t)b * h->dim, mag_b, h->rows.data() + (size_t)a * h->dim, mag_a, h->dim);
}
HQ host_query(const nmn_hnsw* h, const float* q) {
    HQ hq;
    const int metric = h->cfg.distance_metric;
    const bool q8 = h->storage == NMN_HNSW_STORAGE_QUANTIZED;
    if (metric == NMN_METRIC_COSINE || (q8 && metric == NMN_METRIC_EUCLIDEAN)) {
        hq.sq = h_dot8(q, q, h->dim);
        if (metric == NMN_METRIC_COSINE) hq.mag = sqrtf(hq.sq);
    }
    if (q8) hq.sum = h_sum8(q, h->dim);
    return hq;
}

// The walk below is written over `dist(node)`, the query side's distance to a stored row: node_distance for a dense query,
// sparse_node_distance for a SparseVector query (nmn_hnsw_search_sparse).
template <class Dist>
uint32_t host_greedy(const nmn_hnsw* h, const Dist& dist, uint32_t entry, uint32_t layer, uint64_t* evals) {
    uint32_t cur = entry;
    float cur_d = dist(cur);
    (*evals)++;
    for (;;) {
        const std::vector<uint32_t>& ids = h->nbr[cur][layer];  // (the list of the node the round started from)
        bool changed = false;
        uint32_t best = cur;
        for (uint32_t id : ids) {
            const float d = dist(id);
            (*evals)++;
            if (d < cur_d) {
                best = id;
                cur_d = d;
                changed = true;
            }
        }
        cur = best;
        if (!changed) break;
    }
    return cur;
}

// search_layer: the results in the order the reference returns them (stable sort by distance of the heap's vector)
template <class Dist>
void host_search_layer(const nmn_hnsw* h, const Dist& dist, uint32_t entry, uint64_t ef, uint32_t layer, HostVisited& vis,
                       std::vector<Ent>& out, uint64_t* evals) {
    static thread_local std::vector<Ent> cand, res;  // grown on demand, kept: a walk touches a few thousand entries of a graph of millions
    vis.begin(h->level.size());
    if (cand.size() < 1024) cand.resize(1024);
    if (res.size() < 1024) res.resize(1024);
    uint32_t cn = 0, rn = 0;
    const float ed = dist(entry);
    (*evals)++;
    vis.insert(entry);
    heap_push<false>(cand.data(), cn, Ent{ed, entry});
    heap_push<true>(res.data(), rn, Ent{ed, entry});
    while (cn > 0) {
        const Ent cur = heap_pop<false>(cand.data(), cn);
        if (rn >= ef && cur.d > res[0].d) break;
        for (uint32_t id : h->nbr[cur.id][layer]) {
            if (!vis.insert(id)) continue;
            const float d = dist(id);
            (*evals)++;
            const bool should_add = rn < ef || d < res[0].d;
            if (should_add) {
                if (cn == cand.size()) cand.resize(2 * cand.size());
                if (rn == res.size()) res.resize(2 * res.size());
                heap_push<false>(cand.data(), cn, Ent{d, id});
                heap_push<true>(res.data(), rn, Ent{d, id});
                while (rn > ef) (void)heap_pop<true>(res.data(), rn);
            }
        }
    }
    out.assign(res.begin(), res.begin() + rn);
    std::stable_sort(out.begin(), out.end(), [](const Ent& a, const Ent& b) { return a.d < b.d; });
}

// search_with_ef / search_sparse_with_ef (hnsw.rs:2069-2111, 2118-2166): one walk, the distance supplied
template <class Dist>
void host_walk_one(const nmn_hnsw* h, const Dist& dist, uint32_t k, uint64_t ef, HostVisited& vis, uint64_t* ids, float* scores,
                   uint32_t* count, uint64_t* evals, int score_metric = -1) {  // (score_metric -1: the handle's)
    uint32_t c = 0;
    if (h->entry != ~0ull) {
        uint32_t cur = (uint32_t)h->entry;
        for (uint32_t layer = h->max_layer; layer >= 1; layer--) cur = host_greedy(h, dist, cur, layer, evals);
        std::vector<Ent> found;
        host_search_layer(h, dist, cur, std::max<uint64_t>(ef, k), 0, vis, found, evals);
        for (; c < found.size() && c < k; c++) {
            ids[c] = found[c].id;
            scores[c] = to_similarity(score_metric < 0 ? h->cfg.distance_metric : score_metric, found[c].d);
        }
    }
    *count = c;
    for (uint32_t i = c; i < k; i++) {
        ids[i] = ~0ull;
        scores[i] = -INFINITY;
    }
}

}  // namespace
}  // namespace nmn
